"""The host side of the MFE folds (rafft_mfe_batch, rafft_amd.mfe_batch, `rafft --mfe`) and the tests' own mirror of the
recurrences: the mirror equals the minimum of the oracle's energy over every structure of a short sequence, its traceback returns
rows of the co-optimal set - another one in the reversed candidate order wherever the tables tie -, the record's layout, the option
surface, and the errors that need no device.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from rafft_amd import _native, cli, params
import rafft_amd
from conftest import ROOT
import _loops as LP
import _mfe_np as MF
import _par_reader as PR


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def short_sequences():
    rng = np.random.default_rng(930)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (5, 6, 7, 8, 9, 10, 11, 12, 12, 13, 14, 14, 15, 16, 16, 17, 18, 18)]
    seqs += ["".join(rng.choice(list("GC"), n)) for n in (9, 12, 14)]                       # many pairs, many structures
    seqs += ["GGGGAAAACCCC", "GACAC", "GGACACC", "GGACCACC", "GGACACCACC", "GUGUGUGUGUGUGU", "GGGUUUGGGUUUCCC", "NGGGAAACCCN",
             "GCGCAAAGCGCAAAGC"]
    return seqs + LP.N_SEQS


def test_enumeration_counts():
    assert len(MF.enumerate_structures("G" * 10 + "U" * 10)) == 51766
    assert MF.enumerate_structures("GAAAC") == [".....", "(...)"]
    assert MF.enumerate_structures("GAAC") == ["...."]
    rows = MF.enumerate_structures("GGGAAACCCU")
    assert len(set(rows)) == len(rows) and all(len(r) == 10 for r in rows)
    for r in rows:                                            # canonical pairs, hairpins of at least 3
        pt = LP.pair_table(r)
        assert all(j < 0 or ("GGGAAACCCU"[min(i, j)] + "GGGAAACCCU"[max(i, j)]) in MF.PAIRS for i, j in enumerate(pt))
        assert all(j < 0 or abs(j - i) > 3 for i, j in enumerate(pt))


@pytest.mark.parametrize("which", ["builtin", "index_sensitive", "multiloops_win"])
def test_mirror_is_the_minimum_of_the_oracle_over_every_structure(which):
    par = LP.builtin_par()
    if which != "builtin":
        par = LP.index_sensitive_par(par)
        if which == "multiloops_win":
            par.update(ml_closing=-700, ml_intern=-300)
        oracle.set_tables(PR.tables_at(par, 37.0))
    mirror = MF.Mirror(PR.tables_at(par, 37.0))
    n_multi = 0
    for s in short_sequences():
        rows = MF.enumerate_structures(s)
        en = [oracle.eval_structure(s, r) for r in rows]
        assert mirror.mfe(s) == min(en), (which, s)
        best = rows[int(np.argmin(en))]
        n_multi += "(" in best and any(len(LP.branches_of(best, [k])) > 1 for k in range(len(s)) if best[k] == "." and 0 < k < len(s) - 1)
    if which == "multiloops_win":
        assert n_multi > 0                                   # the M / M1 recurrences decide some of these minima


def tie_tables(which):
    par = LP.builtin_par()
    if which != "builtin":
        par = LP.tie_par(par, LP.TIE_ML[int(which[-1])])
        oracle.set_tables(PR.tables_at(par, 37.0))
    return PR.tables_at(par, 37.0)


@pytest.mark.parametrize("which", ["builtin", "tie0", "tie1"])
def test_fold_returns_rows_of_the_cooptimal_set_and_the_tie_tables_tie(which):
    """both candidate orders trace back to a structure of minimum energy; under the flat tables most sequences have several such
    structures and the two orders return different ones - so a device row equal to fold(..., "first") pins the order"""
    mirror = MF.Mirror(tie_tables(which))
    seqs = LP.tie_short_sequences()
    assert len(seqs) == 20 and max(map(len, seqs)) == 20 and sum("N" in s for s in seqs) == 4
    n_cooptimal = n_differ = 0
    for s in seqs:
        rows = MF.enumerate_structures(s)
        en = [oracle.eval_structure(s, r) for r in rows]
        best = {r for r, e in zip(rows, en) if e == min(en)}
        first, last = mirror.fold(s, "first"), mirror.fold(s, "last")
        assert first[0] == last[0] == min(en) == mirror.mfe(s), (which, s)
        assert first[1] in best and last[1] in best, (which, s)
        n_cooptimal += len(best) >= 2
        n_differ += first[1] != last[1]
    print(f"\n{which}: {n_cooptimal} of {len(seqs)} sequences with two or more co-optimal structures, first and last rows differ on {n_differ}")
    if which != "builtin":
        assert n_cooptimal >= 6 and n_differ >= 6


def test_long_tie_list_reaches_the_later_rounds_of_every_ballot():
    """the traceback takes 64 candidates per round; on the long tie list the mirror takes an exterior stem at i >= 64, an M split and
    a C split 64 and more candidates into their ranges, and an interior loop with candidate number >= 64 - under the variant without
    multiloop terms; every row evaluates to the reported energy, and the two orders give different rows on most sequences under
    both variants"""
    seqs = LP.tie_long_sequences()
    assert 40 <= min(map(len, seqs)) and max(map(len, seqs)) <= 105
    reached = {}
    for which in ("tie0", "tie1"):
        mirror = MF.Mirror(tie_tables(which))
        off = dict(F=-1, M=-1, C=-1, I=-1)
        n_differ = 0
        for s in seqs:
            first = mirror.fold(s, "first")
            off = {k: max(v, mirror.offsets[k]) for k, v in off.items()}
            last = mirror.fold(s, "last")
            assert oracle.eval_structure(s, first[1]) == first[0] == last[0] == oracle.eval_structure(s, last[1]), (which, s)
            n_differ += first[1] != last[1]
        print(f"\n{which}: largest candidate offsets taken in the documented order {off}; first and last rows differ on {n_differ} of {len(seqs)}")
        assert n_differ >= 6
        reached[which] = off
    assert all(reached["tie0"][k] >= 64 for k in "FMCI"), reached


def test_mfe_record_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*rafft_mfe_seq;", hdr).group(1)
    fields = re.findall(r"\b(int32_t)\s+([\w, ]+);", body)
    names = [n.strip() for _, group in fields for n in group.split(",")]
    assert names == [n for n, _ in _native.MfeSeq._fields_] == ["status", "length", "dcal", "n_pairs"]
    assert ctypes.sizeof(_native.MfeSeq) == 16
    assert int(re.search(r"#define RAFFT_MFE_MAX_LEN (\d+)", hdr).group(1)) == _native.MFE_MAX_LEN == 4096
    assert {"rafft_mfe_batch", "rafft_mfe_lds_len"} <= set(_native.EXPORTS)
    proto = re.search(r"int rafft_mfe_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_mfe_batch.argtypes)
    assert "vrna_mfe.py:25" in hdr and "bench_mfe.py:11-15" in hdr and "dangles=2" in hdr


def test_lds_bound_and_bad_arguments_need_no_device():
    L = _native.lib()
    lc = L.rafft_mfe_lds_len()
    # three triangular int32 tables, the exterior array and the bases in 128 KiB - and not one position more
    need = lambda n: (3 * (n * (n + 1) // 2) + n + 1) * 4 + ((n + 15) & ~15)
    assert need(lc) <= 128 * 1024 < need(lc + 1)
    buf = ctypes.create_string_buffer(16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.MfeSeq * 1)()
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    assert L.rafft_mfe_batch(-1, seq, ln, 37.0, 0, 0, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_batch(1, None, ln, 37.0, 0, 0, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_batch(1, seq, ln, 37.0, 0, 0, None, out) == _native.ERR_PARAM
    assert L.rafft_mfe_batch(1, seq, ln, 37.0, lc + 1, 0, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_batch(1, seq, ln, 37.0, 0, -1, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_batch(0, None, None, 37.0, 0, 0, None, None) == _native.OK


def test_errors_of_a_sequence_without_a_device():
    """a batch of nothing but erroneous sequences never reaches the device: the fold's codes, the fold's exceptions"""
    from rafft_amd import zuker as M
    rows, dcal, n_pairs, status = M.mfe_batch_raw(["", "GGGTAACCC", "gggaaaccc", "A" * (_native.MFE_MAX_LEN + 1)])
    assert status == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG]
    assert rows == ["", "." * 9, "." * 9, "." * (_native.MFE_MAX_LEN + 1)] and dcal == [0] * 4 and n_pairs == [0] * 4
    assert _native.lib().rafft_last_error().decode().startswith("sequence 0")
    with pytest.raises(np.exceptions.AxisError):
        rafft_amd.mfe("")
    with pytest.raises(KeyError):
        rafft_amd.mfe("GGGTAACCC")
    with pytest.raises(ValueError, match="4096 nt"):
        rafft_amd.mfe("A" * (_native.MFE_MAX_LEN + 1))
    with pytest.raises(_native.RafftError) as e:             # the temperature is checked first, as the fold checks it
        M.mfe_batch_raw(["", "GGGXAACCC"], temp=25.0)
    assert e.value.code == _native.ERR_TEMP
    assert rafft_amd.mfe_batch(["", "GGGXAACCC"], raise_errors=False) == [None, None]


def test_cli_parses_mfe():
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--mfe", "-o", "out.txt"])
    assert a.mfe and a.batch and a.output == "out.txt"
    assert cli.parse_arguments(["-s", "GGGAAACCC", "--mfe"]).mfe
    assert not cli.parse_arguments(["-s", "GGGAAACCC"]).mfe


def test_cli_mfe_prints_the_line_of_vrna_mfe(tmp_path, capsys):
    from rafft_amd.utils import Structure
    calls = []

    def stub(seqs, temp):
        calls.append((list(seqs), temp))
        return [Structure("(((...)))"[:len(s)] if len(s) == 9 else "." * len(s), -3070 if len(s) == 9 else 0) for s in seqs]

    cli.main(["-s", "GGGAAACCC", "--mfe"], mfe_batch=stub)
    assert capsys.readouterr().out == "GGGAAACCC 9 (((...))) -30.700000762939453 3\n"       # print(float32 -30.7), vrna_mfe.py:26
    fa = tmp_path / "s.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nAAAA\n")
    out = tmp_path / "o.txt"
    cli.main(["-sf", str(fa), "--batch", "--mfe", "-o", str(out)], mfe_batch=stub)
    assert out.read_text().splitlines() == ["GGGAAACCC 9 (((...))) -30.700000762939453 3", "AAAA 4 .... 0.0 0"]
    assert calls[-1] == (["GGGAAACCC", "AAAA"], 37.0)
    # --scores: one row per sequence through the scorer, the table of mfe_scores.csv
    csvf = tmp_path / "k.csv"
    csvf.write_text("GGGAAACCC,((.....)),x1\nAAAA,....,x2\n")
    seen = {}

    def scorer(beams, known):
        seen["beams"], seen["known"] = [[st.str_struct for st in b] for b in beams], list(known)
        z = np.zeros(2, dtype=np.int32)
        return dict(pick_ppv=z, pick_first=z, row0=np.array([0, 1]), n_known=np.array([2, 0]), seq_status=z, n_pred=np.array([3, 0]),
                    hit_pred=np.array([2, 0]), hit_known=np.array([2, 0]))

    sc = tmp_path / "scores.csv"
    cli.main(["-sf", str(csvf), "--batch", "--mfe", "--scores", str(sc)], mfe_batch=stub, scorer=scorer)
    assert seen == {"beams": [["(((...)))"], ["...."]], "known": ["((.....))", "...."]}
    assert sc.read_text().splitlines() == ["seq,len_seq,struct,nrj,nbp,pvv,sens,name", "GGGAAACCC,9,(((...))),-30.700000762939453,3,66.67,100.0,x1",
                                           "AAAA,4,....,0.0,0,0.0,0.0,x2"]
    with pytest.raises(SystemExit):
        cli.main(["-s", "GGGAAACCC", "--mfe", "--traj"], mfe_batch=stub)
