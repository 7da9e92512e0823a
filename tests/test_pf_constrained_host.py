"""The host side of the partition function under constraints and soft terms (rafft_pf_constrained_batch,
rafft_amd.pf_constrained_batch, `rafft --pf -C`, `rafft --pf --shape FILE`) and the tests' mirror of it: the
mirror equals the sum over every enumerated structure that satisfies the constraint, with the soft terms in the weights - energy,
every P, the unpaired probabilities and the share of the optimum - and its Z is 0 exactly when there is none; a mirror with one
free() test dropped fails the same check; the record and the symbol, every error the host detects, the option surface.  No GPU."""
import ctypes
import io
import math
import os
import re
import sys

import numpy as np
import pytest

import oracle
from rafft_amd import _native, cli, mccaskill, params
import rafft_amd
from conftest import ROOT
import _mfe_con_np as MC
import _pf_np as PF
import _pf_con_np as PC
from test_mfe_constrained_host import table_set, enumerated, MALFORMED

SEED = 79                                   # of the drawn constraints, as tests/test_mfe_constrained_host.py
E_TOL, P_TOL, F_TOL = 1e-8, 1e-9, 1e-9      # kcal/mol, probability, share (relative): those of tests/test_gpu_pf.py


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def errors(mirror, which, case):
    """None for an infeasible case the mirror calls infeasible; else the mirror's errors (energy, P, unpaired, share) against exact_con"""
    s, con, u, b = case
    rows, en = enumerated(which, s)
    Z, P, best = PC.exact_con(s, con, u, b, rows, en, mirror.kt)
    z, p, un = mirror.run(s, con, u, b)
    if best is None or z == 0.0:
        return None if best is None and z == 0.0 else (math.inf,) * 4
    share = lambda zz: math.exp(-best / (100.0 * mirror.kt)) / zz
    return (abs(-mirror.kt * math.log(z) + mirror.kt * math.log(Z)), float(np.abs(p - P).max()), float(np.abs(un - PC.unpaired_of(P)).max()),
            abs(share(z) / share(Z) - 1.0))


def within(err):
    return err[0] <= E_TOL and err[1] <= P_TOL and err[2] <= P_TOL and err[3] <= F_TOL


def test_mirror_is_the_sum_over_every_structure_that_satisfies_the_constraint():
    """the exhaustive cases, plain and with soft terms.  The defective mirror is put to the same check - an error within the bounds
    where the set is not empty, Z = 0 where it is - and fails it on 4 plain and 5 soft cases under the committed seed: on most of
    them it gives an infeasible case a weight, a multiloop leaving a position unpaired that has to pair"""
    which = "builtin"
    tables = table_set(which)
    mirror, broken = PC.PfConMirror(tables), PC.PfConMirror(tables, drop_free=True)
    n_broken = 0
    for soft in (False, True):
        cases = MC.exhaustive_cases(SEED, soft=soft)
        assert len(cases) == (24 * 7 if soft else 144)
        worst, n_feasible, n_infeasible = [0.0] * 4, 0, 0
        for case in cases:
            err = errors(mirror, which, case)
            rows, en = enumerated(which, case[0])
            empty = not any(MC.satisfies(r, case[1]) for r in rows)
            assert (err is None) == empty, case                                     # Z is 0 exactly when the filtered set is empty
            bad = errors(broken, which, case)
            n_broken += (bad is None) != empty or (bad is not None and not within(bad))
            if err is None:
                n_infeasible += 1
                continue
            n_feasible += 1
            worst = [max(a, b) for a, b in zip(worst, err)]
            assert within(err), (case, err)
        print(f"\nsoft={soft}: {n_feasible} feasible, {n_infeasible} infeasible; the mirror's worst errors: energy {worst[0]:.3g} kcal/mol, P {worst[1]:.3g}, "
              f"unpaired {worst[2]:.3g}, share {worst[3]:.3g}; the mirror without free() in M has failed on {n_broken} so far")
        if not soft:
            assert (n_feasible, n_infeasible) == (64, 80)
        assert n_feasible >= 40 and n_infeasible >= 10
    assert n_broken >= 5


def test_mirror_without_constraints_is_pf_mirror():
    tables = table_set("builtin")
    for s in MC.short_sequences()[8:14]:
        Z, P = PF.PfMirror(tables).run(s)
        for con, u, b in ((None, None, None), ("." * len(s), np.zeros(len(s), int), np.zeros(len(s), int))):
            z, p, un = PC.PfConMirror(tables).run(s, con, u, b)
            assert z == Z and (p == P).all() and np.abs(un - PC.unpaired_of(P)).max() == 0


def test_record_and_entry_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    assert "rafft_pf_constrained_batch" in _native.EXPORTS
    proto = re.search(r"int rafft_pf_constrained_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_pf_constrained_batch.argtypes) == 13
    assert "rafft_pf_seq *seq_out" in proto and ctypes.sizeof(_native.PfSeq) == 32
    assert {"pf_constrained", "pf_constrained_batch", "pf_constrained_batch_raw"} <= set(dir(rafft_amd))
    assert "unpaired" in mccaskill.PfResult.__slots__
    assert "need NOT satisfy" in hdr                                                # the centroid and `|`


def test_bad_arguments_need_no_device():
    L = _native.lib()
    buf = ctypes.create_string_buffer(16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.PfSeq * 1)()
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    call = L.rafft_pf_constrained_batch
    assert call(-1, seq, ln, 37.0, None, None, None, 0.0, 0, rec, out, None, None) == _native.ERR_PARAM
    assert call(1, None, ln, 37.0, None, None, None, 0.0, 0, rec, out, None, None) == _native.ERR_PARAM
    assert call(1, seq, None, 37.0, None, None, None, 0.0, 0, rec, out, None, None) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, 0.0, 0, None, out, None, None) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, 0.0, 0, rec, None, None, None) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, -1.0, 0, rec, out, None, None) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, float("nan"), 0, rec, out, None, None) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, float("inf"), 0, rec, out, None, None) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, 0.0, -1, rec, out, None, None) == _native.ERR_PARAM
    assert call(0, None, None, 37.0, None, None, None, 0.0, 0, None, None, None, None) == _native.OK
    for bad, where in ((20001, "soft_unpaired"), (-20001, "soft_stack")):           # before anything is launched
        soft = [0] * 9
        soft[4] = bad
        with pytest.raises(_native.RafftError) as e:
            mccaskill.pf_constrained_batch_raw(["GGGAAACCC"], **{where: [soft]})
        assert e.value.code == _native.ERR_PARAM and "RAFFT_MFE_SOFT_MAX" in str(e.value) and "position 4" in str(e.value)
    with pytest.raises(_native.RafftError) as e:
        mccaskill.pf_constrained_batch_raw(["GGGAAACCC"], ["(((...)))"], temp=25.0)
    assert e.value.code == _native.ERR_TEMP
    with pytest.raises(ValueError):
        mccaskill.pf_constrained_batch_raw(["GGGAAACCC"], ["(((...)))", "."])
    with pytest.raises(ValueError):
        mccaskill.pf_constrained_batch_raw(["GGGAAACCC"], soft_unpaired=[[0] * 8])


def test_every_host_detected_error_of_a_sequence_without_a_device():
    seqs = ["GGGAAACCC"] * len(MALFORMED)
    rows, recs, pr, un = mccaskill.pf_constrained_batch_raw(seqs, MALFORMED)
    assert [r["status"] for r in recs] == [_native.ERR_STRUCT] * len(MALFORMED) and rows == ["." * 9] * len(MALFORMED)
    assert all(r["energy"] == 0.0 and r["mfe_frequency"] == 0.0 and r["mfe_dcal"] == 0 and r["n_pairs"] == 0 for r in recs)
    assert all(not p.any() for p in pr) and all(not x.any() for x in un)
    assert _native.lib().rafft_last_error().decode().startswith("sequence 0: a constraint string of another length")
    too_long = "A" * (_native.PF_MAX_LEN + 1)
    seqs = ["GGGAAACCC", too_long, "", "GGGTAACCC", "GGGAAACCC"]
    cons = ["(((..)))).", None, "(", "(((...)))", "((.....)"]
    rows, recs, pr, un = mccaskill.pf_constrained_batch_raw(seqs, cons)
    assert [r["status"] for r in recs] == [_native.ERR_STRUCT, _native.ERR_TOO_LONG, _native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_STRUCT]
    assert rows == ["." * 9, "." * len(too_long), "", "." * 9, "." * 9] and pr[1] is None and un[1] is None
    assert _native.lib().rafft_last_error().decode().startswith("sequence 0: a constraint")
    mccaskill.pf_constrained_batch_raw(seqs[1:], cons[1:])
    assert _native.lib().rafft_last_error().decode() == "sequence 0: longer than RAFFT_MFE_MAX_LEN"
    assert rafft_amd.pf_constrained_batch(seqs, cons, raise_errors=False) == [None] * 5
    with pytest.raises(ValueError, match="malformed constraint"):
        rafft_amd.pf_constrained("GGGAAACCC", "(((...))")
    with pytest.raises(KeyError):
        rafft_amd.pf_constrained("GGGTAACCC", "(((...)))")


def test_cli_pf_takes_constraints_and_shape(tmp_path, capsys, monkeypatch):
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--pf", "-C", "--shape", "r.shape", "--shape-slope", "2.0", "--shape-intercept", "-0.5"])
    assert a.pf and a.constraint and a.shape == "r.shape" and a.shape_slope == 2.0 and a.shape_intercept == -0.5
    for argv in (["-s", "GGGAAACCC", "--pf", "--pf-span", "40", "-C"], ["-s", "GGGAAACCC", "--pf", "--pf-span", "40", "--shape", "x"]):
        with pytest.raises(SystemExit) as e:                                        # --pf-span with constraints stays an error
            cli.main(argv)
        assert "--pf-span" in str(e.value)
    for argv in (["-s", "GGGAAACCC", "-C"], ["-s", "GGGAAACCC", "--shape", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--mfe" in str(e.value) and "--pf" in str(e.value)
    with pytest.raises(SystemExit, match="no --mfe"):
        cli.main(["-s", "GGGAAACCC", "--pf", "--mfe", "--shape", "x"])
    seen = {}
    P = np.zeros((9, 9))
    P[0, 8], P[1, 7] = 0.75, 0.25

    def fake(sequences, constraints, soft_unpaired, soft_stack, temp, probs=True):
        seen.update(sequences=sequences, constraints=constraints, soft_unpaired=soft_unpaired, soft_stack=soft_stack, probs=probs)
        return [mccaskill.PfResult(-3.25, "(.......)", 0.5, -2.95, P if probs else None, PC.unpaired_of(P))] * len(sequences)
    one = tmp_path / "one.shape"
    one.write_text("1 0.0\n")
    # -s SEQ -C: the constraint is one line on stdin, for --pf as for --mfe; a stdin that gives none is an error of its own
    for mode in ("--pf", "--mfe"):
        for text in ("", "\n"):
            monkeypatch.setattr(sys, "stdin", io.StringIO(text))
            with pytest.raises(SystemExit, match="constraint line from stdin"):
                cli.main(["-s", "GGGAAACCC", mode, "-C"], pf_constrained_batch=fake, mfe_constrained_batch=fake)
    monkeypatch.setattr(sys, "stdin", io.StringIO("(.......)\n"))
    cli.main(["-s", "GGGAAACCC", "--pf", "-C"], pf_constrained_batch=fake)
    assert capsys.readouterr().out == "GGGAAACCC 9 (.......) -3.25 1 0.5\n" and seen["constraints"] == ["(.......)"] and seen["soft_stack"] is None
    monkeypatch.undo()
    cli.main(["-s", "GGGAAACCC", "--pf", "--shape", str(one)], pf_constrained_batch=fake)
    assert capsys.readouterr().out == "GGGAAACCC 9 (.......) -3.25 1 0.5\n"       # the line of --pf
    assert seen["constraints"] is None and seen["soft_unpaired"] is None and seen["soft_stack"][0].tolist() == [-60] + [0] * 8 and not seen["probs"]
    fa = tmp_path / "seqs.fa"
    fa.write_text(">a\nGGGAAACCC\n(((...)))\n>b\nGGGGAAAACCCC\n....xxxx....\n")
    bpp = tmp_path / "out.bpp"
    cli.main(["-sf", str(fa), "--batch", "--pf", "-C", "--bpp", str(bpp), "--bpp-cutoff", "0.5"], pf_constrained_batch=fake)
    assert seen["constraints"] == ["(((...)))", "....xxxx...."] and seen["probs"] and capsys.readouterr().out.count("\n") == 2
    assert bpp.read_text() == "a 1 9 0.75\nb 1 9 0.75\n"                            # dense although the results hold `unpaired`
