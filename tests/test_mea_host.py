"""The numpy mirror of the MEA recursion (tests/_mea_np.py) against brute force, and the host-pure part of the MEA drivers - no GPU.
On random matrices with L <= 14 the mirror's mea is the maximum of expected_accuracy over EVERY non-crossing set of non-zero
cells, and the mirror's row attains it.  Tolerance 1e-9: a value is a sum of at most 14 terms of at most 16 each (2 gamma P with
gamma <= 8), so two orders of summation differ by less than 14 * 224 * 2^-53 < 1e-12."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rafft_amd import _native, mccaskill
from conftest import ROOT
import _mea_np as M

TOL = 1e-9


def random_matrix(rng, L, dyadic, min_gap, density):
    P = np.zeros((L, L))
    for i in range(L):
        for j in range(i + min_gap, L):
            if rng.random() < density:
                P[i, j] = rng.integers(1, 9) / 8.0 if dyadic else rng.random()
    if not dyadic:                                         # rows of probabilities: no position above a total of 1 (q stays informative)
        for _ in range(3):
            tot = P.sum(axis=0) + P.sum(axis=1)
            scale = np.where(tot > 1.0, 1.0 / np.maximum(tot, 1e-300), 1.0)
            P *= np.minimum.outer(scale, scale)
    return P


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for L, dyadic, gap, dens in ((1, True, 4, 1.0), (4, True, 4, 1.0), (5, True, 4, 1.0), (9, True, 4, 0.8), (12, True, 1, 0.5), (14, True, 4, 0.7), (14, True, 4, 1.0),
                                 (8, False, 1, 0.9), (11, False, 2, 0.6), (13, False, 4, 0.8), (14, False, 4, 1.0), (14, False, 4, 0.5)):
        for gamma in (0.5, 1.0, 8.0):
            out.append((random_matrix(rng, L, dyadic, gap, dens), gamma, dyadic))
    return out


def test_mirror_equals_the_maximum_over_every_structure():
    n_paired = 0
    for P, gamma, dyadic in cases():
        # frequencies of crossing rows may sum above 1 (dyadic cases do): q is clamped there, as the definition says
        q = M.unpaired(P)
        assert (q >= 0.0).all() and (q <= 1.0).all()
        rows = M.structures_over(P)
        assert len(set(rows)) == len(rows) and "." * len(q) in rows
        best = max(M.expected_accuracy(r, P, q, gamma) for r in rows)
        row, mea = M.mea(P, q, gamma)
        assert abs(mea - best) <= TOL, (len(q), gamma, mea, best)
        assert row in rows and abs(M.expected_accuracy(row, P, q, gamma) - mea) <= TOL
        last_row, last_mea = M.mea(P, q, gamma, last=True)
        assert last_mea == mea and abs(M.expected_accuracy(last_row, P, q, gamma) - mea) <= TOL
        n_paired += "(" in row
    assert n_paired >= 20                                  # the cases are not all-dot rows


def test_mirror_on_known_answers():
    P = np.zeros((12, 12))
    for i, j in ((0, 11), (1, 10), (2, 9)):
        P[i, j] = 1.0
    q = M.unpaired(P)
    assert q.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    for gamma in (0.5, 1.0, 4.0):
        assert M.mea(P, q, gamma) == ("(((......)))", 2 * gamma * 3 + 6)
    assert M.diversity(P) == 0.0 and M.expected_accuracy("(((......)))", P, q, 2.0) == 18.0
    assert M.mea(np.zeros((3, 3)), np.ones(3), 1.0) == ("...", 3.0)
    # a tie: (0,5) and (1,5) weigh the same and position 0 / 1 is as likely unpaired - the first k ascending wins, the last differs
    T = np.zeros((6, 6))
    T[0, 5] = T[1, 5] = 0.5
    qt = M.unpaired(T)
    assert M.mea(T, qt, 1.0)[0] == "(....)" and M.mea(T, qt, 1.0, last=True)[0] == ".(...)"
    assert M.diversity(T) == 1.0


def test_pair_frequencies():
    F = mccaskill.pair_frequencies(["((....))", "(......)", "........", b".(....)."])
    assert F.shape == (8, 8) and F[0, 7] == 0.5 and F[1, 6] == 0.5 and np.count_nonzero(F) == 2
    F = mccaskill.pair_frequencies(["(....)", "......"], weights=[3, 1])
    assert F[0, 5] == 0.75
    for bad in ([], ["(...", "(...)"], ["(.x.)"], ["(...))"]):
        with pytest.raises(ValueError):
            mccaskill.pair_frequencies(bad)
    with pytest.raises(ValueError):
        mccaskill.pair_frequencies(["(...)"], weights=[-1.0])


def test_host_pure_part_builds_and_passes_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "hostcheck", "mea_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("mea_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and " checks, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr


def test_mea_records_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    for name, cls, size in (("rafft_mea_seq", _native.MeaSeq, 48), ("rafft_mea_probs_seq", _native.MeaProbsSeq, 32)):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", hdr).group(1), flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_] and ctypes.sizeof(cls) == size
    assert "rafft_mea_batch" in _native.EXPORTS and "rafft_mea_probs_batch" in _native.EXPORTS


# ---- the command line, with stand-ins for the device calls

def test_cli_mea_lines_scores_and_exclusions(tmp_path, capsys):
    from rafft_amd import cli
    from rafft_amd.mccaskill import MeaResult
    a = cli.parse_arguments(["-s", "GGGAAACCC", "--mea"])
    assert a.mea == 1.0 and cli.parse_arguments(["-s", "GGGAAACCC", "--mea", "2.5"]).mea == 2.5 and cli.parse_arguments(["-s", "GGGAAACCC"]).mea is None
    calls = []

    def stub(seqs, gamma, temp):
        calls.append((list(seqs), gamma, temp))
        return [MeaResult("(((...)))", 8.25, -3.07, -3.456, 1.5, np.zeros(9)) if len(s) == 9 else MeaResult("." * len(s), float(len(s)), 0.0, 0.0, 0.0, np.ones(len(s)))
                for s in seqs]

    cli.main(["-s", "GGGAAACCC", "--mea"], mea_batch=stub)
    assert capsys.readouterr().out == "GGGAAACCC 9 (((...))) -3.07 8.2500 1.5000\n"
    fa = tmp_path / "s.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nAAAA\n")
    out = tmp_path / "o.txt"
    cli.main(["-sf", str(fa), "--batch", "--mea", "4", "-o", str(out)], mea_batch=stub)
    assert out.read_text().splitlines() == ["GGGAAACCC 9 (((...))) -3.07 8.2500 1.5000", "AAAA 4 .... 0.00 4.0000 0.0000"]
    assert calls[-1] == (["GGGAAACCC", "AAAA"], 4.0, 37.0)
    csvf = tmp_path / "k.csv"
    csvf.write_text("GGGAAACCC,((.....)),x1\nAAAA,....,x2\n")
    seen = {}

    def scorer(beams, known):
        seen["beams"], seen["known"] = [[st.str_struct for st in b] for b in beams], list(known)
        z = np.zeros(2, dtype=np.int32)
        return dict(pick_ppv=z, pick_first=z, row0=np.array([0, 1]), n_known=np.array([2, 0]), seq_status=z, n_pred=np.array([3, 0]),
                    hit_pred=np.array([2, 0]), hit_known=np.array([2, 0]))

    sc = tmp_path / "scores.csv"
    cli.main(["-sf", str(csvf), "--batch", "--mea", "--scores", str(sc)], mea_batch=stub, scorer=scorer)
    assert seen == {"beams": [["(((...)))"], ["...."]], "known": ["((.....))", "...."]}
    # the energy column is the row's energy, not the ensemble's
    assert sc.read_text().splitlines() == ["seq,len_seq,struct,nrj,nbp,pvv,sens,name", "GGGAAACCC,9,(((...))),-3.07,3,66.67,100.0,x1", "AAAA,4,....,0.0,0,0.0,0.0,x2"]
    for extra in (["--pf"], ["--mfe"], ["--traj"], ["--subopt", "1.0"], ["--kin", str(tmp_path / "kin.txt")]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-sf", str(fa), "--batch", "--mea"] + extra, mea_batch=stub)
        assert str(e.value) == cli.MEA_EXCLUSIVE
    for gamma in ("0", "-1", "nan"):
        with pytest.raises(SystemExit):
            cli.main(["-s", "GGGAAACCC", "--mea", gamma], mea_batch=stub)
