"""rafft_pf_constrained_batch on a real MI355X (`-m gpu`): the sums over every enumerated structure that
satisfies the constraint, with the soft terms in the weights, in one batch with null entries between the packs; the tests' mirror of
the constrained recurrences at 60-105 nt on the constructions of section 20 and at 133 and 197 nt, where every 64-candidate loop
goes past its second round; the bits of rafft_pf_batch where nothing constrains; the same bits in any order, alone and with one
sequence a chunk; the scale; other temperatures; the limits; the MEA row over the result; the command line.
Bounds: those of tests/test_gpu_pf.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, cli, mccaskill, rafft as R, zuker
from conftest import ROOT
import _lane_rounds as LR
import _mfe_con_np as MC
import _mfe_np as MF
import _par_reader as PR
import _pf_np as PF
import _pf_con_np as PC
import test_gpu_mfe_constrained as TC
from test_gpu_mfe_constrained import sets, back_to_builtin, install         # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

E_TOL, P_TOL, F_TOL = 1e-8, 1e-9, 1e-9      # kcal/mol, probability, share (relative): tests/test_gpu_pf.py


def run(cases, **kw):
    """pf_constrained_batch_raw of a list of (seq, con, u, b) cases; an array of nothing but None goes as no array at all"""
    col = lambda k: None if all(c[k] is None for c in cases) else [c[k] for c in cases]
    return mccaskill.pf_constrained_batch_raw([c[0] for c in cases], col(1), col(2), col(3), **kw)


def bits(raw, k):
    """everything the call returns for sequence k, as bytes and integers"""
    rows, recs, probs, un = raw
    r = recs[k]
    return (rows[k], r["status"], r["length"], r["mfe_dcal"], r["n_pairs"], np.float64(r["energy"]).tobytes(), np.float64(r["mfe_frequency"]).tobytes(),
            None if probs[k] is None else probs[k].tobytes(), None if un[k] is None else un[k].tobytes())


def centroid_of(P):
    row = ["."] * len(P)
    for i, j in zip(*np.nonzero(P > 0.5)):
        row[i], row[j] = "(", ")"
    return "".join(row)


def against(raw, k, Z, P, best, kt):
    """the errors of result k - energy, P, unpaired, share (relative) - against (Z, P) and the optimum `best`; the exact fields"""
    rows, recs, probs, un = raw
    r = recs[k]
    assert r["status"] == 0 and r["mfe_dcal"] == best and rows[k] == centroid_of(probs[k]) and r["n_pairs"] == rows[k].count("(")
    assert np.isfinite(probs[k]).all() and np.isfinite(un[k]).all() and not np.tril(probs[k]).any()
    f = math.exp(-best / (100.0 * kt)) / Z
    return (abs(r["energy"] + kt * math.log(Z)), float(np.abs(probs[k] - P).max()), float(np.abs(un[k] - PC.unpaired_of(P)).max()),
            abs(r["mfe_frequency"] / f - 1.0))


def report(name, errs):
    worst = [max(e[x] for e in errs) for x in range(4)]
    print(f"\n{name}: largest error of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of unpaired {worst[2]:.3g}, of the share {worst[3]:.3g} (relative)")
    assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= P_TOL and worst[3] <= F_TOL


def check_errors_are_zero(cases, raw):
    rows, recs, probs, un = raw
    for k, r in enumerate(recs):
        if r["status"]:
            assert rows[k] == "." * len(cases[k][0]) and (r["mfe_dcal"], r["n_pairs"], r["energy"], r["mfe_frequency"]) == (0, 0, 0.0, 0.0)
            assert probs[k] is None or not probs[k].any()
            assert un[k] is None or not un[k].any()


# ---- 1. every structure

def enumerated_energies(seqs, temp=37.0):
    enum = {s: MF.enumerate_structures(s) for s in seqs}
    en, st = R.eval_structures([s for s in seqs for _ in enum[s]], [r for s in seqs for r in enum[s]], temp=temp)       # one call
    assert not any(st)
    energy, at = {}, 0
    for s in seqs:
        energy[s] = en[at:at + len(enum[s])]
        at += len(enum[s])
    return enum, energy


@pytest.mark.parametrize("which", ["builtin", "tie0"])
def test_gpu_constrained_pf_equals_the_sums_over_every_structure_that_satisfies_the_constraint(sets, which):
    install(sets, which)
    cases = TC.exhaustive_batch()
    seqs = MC.short_sequences()
    assert len(cases) == 24 * 15 and sum(c[1] is None and c[2] is None for c in cases) == 24
    enum, energy = enumerated_energies(seqs)
    kt = PF.kt_of(37.0)
    raw = run(cases)                                                                # ONE batch
    rows, recs, probs, un = raw
    errs, n_inf = [], 0
    for k, (s, con, u, b) in enumerate(cases):
        Z, P, best = PC.exact_con(s, con, u, b, enum[s], energy[s], kt)
        if best is None:
            assert recs[k]["status"] == N.ERR_INFEASIBLE, k
            n_inf += 1
            continue
        errs.append(against(raw, k, Z, P, best, kt))
    report(which, errs)
    check_errors_are_zero(cases, raw)
    assert n_inf >= 20 and len(errs) >= 150
    first = [r["status"] for r in recs].index(N.ERR_INFEASIBLE)
    assert N.lib().rafft_last_error().decode() == f"sequence {first}: no structure satisfies its constraints"
    a = max(first - 2, 0)                                                           # the neighbours of an infeasible case, alone: the same bits
    for k in range(a, a + 6):
        assert bits(run(cases[k:k + 1]), 0) == bits(raw, k), k


# ---- 2. against the mirror where enumeration cannot reach

_WANT = {}


def mirror_results(key, tables, cases, temp=37.0):
    if key not in _WANT:
        m = PC.PfConMirror(tables, temp)
        _WANT[key] = [m.run(*c) for c in cases]
    return _WANT[key]


def test_gpu_constrained_pf_equals_the_mirror_at_60_to_105_nt(sets):
    which = "builtin"
    install(sets, which)
    cases, marks = TC.mirror_cases(sets, which)
    tables = PR.tables_at(sets[which], 37.0)
    want = mirror_results(which, tables, cases)
    kt = PF.kt_of(37.0)
    raw = run(cases)
    rows, recs, probs, un = raw
    best = TC.run(cases)[1]                     # (rafft_mfe_constrained_batch: tests/test_gpu_mfe_constrained.py holds it to ConMirror on these cases)
    errs = []
    for k, (Z, P, _) in enumerate(want):
        if Z == 0.0:
            assert recs[k]["status"] == N.ERR_INFEASIBLE, k
            continue
        errs.append(against(raw, k, Z, P, best[k], kt))
    report(which, errs)
    check_errors_are_zero(cases, raw)
    assert len(errs) >= 9
    for k in range(len(cases)):                                                     # x is unpaired, | < > ( ) are paired, whatever else holds
        if recs[k]["status"] == 0:
            for x, c in enumerate(cases[k][1] or ""):
                if c != ".":
                    assert abs(un[k][x] - (1.0 if c == "x" else 0.0)) <= P_TOL, (k, x, c)
                if c == "<":
                    assert not probs[k][:, x].any()
                if c == ">":
                    assert not probs[k][x, :].any()
    for k in marks["adjacent"]:                                                     # | directly inside a forced pair
        con = cases[k][1]
        assert recs[k]["status"] == 0 and abs(probs[k][con.index("("), con.index(")")] - 1.0) <= P_TOL and abs(un[k][con.index("|")]) <= P_TOL
    k = marks["crossing"]                                                           # a forced pair that crosses a helix of the free optimum
    (i, j), con = marks["helix"], cases[k][1]
    assert recs[k]["status"] == 0 and abs(probs[k][con.index("("), con.index(")")] - 1.0) <= P_TOL
    assert probs[k][i, j] == probs[k][i + 1, j - 1] == probs[k][i + 2, j - 2] == 0.0
    free = mccaskill.pf_batch_raw([cases[k][0]])
    assert free[2][0][i + 1, j - 1] > 0.1 and recs[k]["energy"] > free[1][0]["energy"]
    k = marks["hairpin3"]                                                           # a hairpin of exactly 3 around a |
    assert recs[k]["status"] == 0 and probs[k][3, 7] == 0.0 and abs(un[k][5]) <= P_TOL
    assert recs[k + 1]["status"] == N.ERR_INFEASIBLE
    assert recs[1]["status"] == 0 and abs(un[1][0] - 1.0) <= P_TOL and abs(un[1][66] - 1.0) <= P_TOL                  # x at both ends
    assert recs[2]["status"] == 0 and abs(un[2][0]) <= P_TOL and abs(un[2][74]) <= P_TOL                             # < and > at both ends


def test_gpu_constrained_pf_equals_the_mirror_past_the_second_lane_round():
    """133 and 197 nt with a drawn constraint and soft terms: the C and M splits, the exterior sums and the outside sums of these
    lengths take two and three rounds of 64 candidates (tests/_lane_rounds.py), the free / U factors of the M and M1o sums with them"""
    cases = LR.con_cases()
    assert [len(c[0]) for c in cases] == [133, 197] and all(set(c[1]) - {"."} and np.abs(c[2]).max() > 100 for c in cases)
    tables = LR.tables("builtin")
    want = mirror_results("rounds", tables, cases)
    raw = run(cases)
    kt = PF.kt_of(37.0)
    errs = [against(raw, k, Z, P, LR.con_fold(cases[k])[0][0], kt) for k, (Z, P, _) in enumerate(want)]
    report("133 / 197 nt", errs)
    for k, c in enumerate(cases):
        assert float(raw[2][k].max()) > 0.5 and any(abs(raw[3][k][x] - (c[1][x] == "x")) <= P_TOL for x in range(len(c[0])) if c[1][x] != ".")


# ---- 3. where nothing constrains: the bits of rafft_pf_batch

def test_gpu_constrained_pf_is_pf_batch_where_nothing_constrains():
    seqs = TC.neutral_sequences()
    assert len(seqs[-1]) == 200 and sum(60 <= len(s) <= 90 for s in seqs) >= 6       # (and two constructed ones of 54 and 55 nt)
    free = mccaskill.pf_batch_raw(seqs)
    assert not any(r["status"] for r in free[1])
    zero = lambda s: np.zeros(len(s), dtype=np.int32)
    forms = {"no arrays": [(s, None, None, None) for s in seqs],
             "all-'.' strings": [(s, "." * len(s), None, None) for s in seqs],
             "zero arrays": [(s, None, zero(s), zero(s)) for s in seqs],
             "all three": [(s, "." * len(s), zero(s), zero(s)) for s in seqs],
             "mixed": [(s, ("." * len(s), None)[k % 2], (zero(s), None, None)[k % 3], (None, zero(s))[k % 2]) for k, s in enumerate(seqs)]}
    for name, cases in forms.items():
        rows, recs, probs, un = run(cases)
        assert rows == free[0] and recs == free[1], name
        for k in range(len(seqs)):
            assert probs[k].tobytes() == free[2][k].tobytes(), (name, k)
            assert np.abs(un[k] - PC.unpaired_of(probs[k])).max() <= 1e-12


# ---- 4. the same bits in any order, alone, in every chunking

def test_gpu_constrained_pf_same_bits_in_any_order_alone_and_in_every_chunking():
    rng = np.random.default_rng(5)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (33, 58, 71, 20, 64, 45, 80, 9, 40, 41)]
    cases = []
    for k, s in enumerate(seqs):
        u = rng.integers(-150, 151, len(s)).astype(np.int32) if k % 3 == 0 else None
        b = rng.integers(-200, 101, len(s)).astype(np.int32) if k % 2 == 0 else None
        cases.append((s, MC.draw_constraint(rng, s) if k % 4 != 3 else None, u, b))
    cases.append((seqs[1], None, None, None))
    whole = run(cases)
    assert [r["status"] for r in whole[1]].count(0) >= 5 and N.ERR_INFEASIBLE in [r["status"] for r in whole[1]]
    check_errors_are_zero(cases, whole)
    all_bits = [bits(whole, k) for k in range(len(cases))]
    for kw in (dict(workspace_bytes=1), dict(workspace_bytes=2 * 6 * 64 * 64 * 8)):        # one sequence a chunk; two or so
        got = run(cases, **kw)
        assert [bits(got, k) for k in range(len(cases))] == all_bits, kw
    order = [int(k) for k in rng.permutation(len(cases))]
    got = run([cases[k] for k in order])
    assert [bits(got, at) for at in range(len(order))] == [all_bits[k] for k in order]
    for k in (0, 2, len(cases) - 1):                                                # alone
        assert bits(run(cases[k:k + 1]), 0) == all_bits[k]
    no_arrays = run(cases, probs=False, unpaired=False)                            # the records and rows do not depend on what is asked for
    assert no_arrays[0] == whole[0] and no_arrays[1] == whole[1] and no_arrays[2] is None and no_arrays[3] is None


# ---- 5. the scale

def test_gpu_constrained_pf_does_not_depend_on_the_scale(sets):
    cases, _ = TC.mirror_cases(sets, "builtin")
    cases = cases[:5] + LR.con_cases()[:1]
    base = run(cases, scale_factor=1.07)
    assert not any(r["status"] for r in base[1])
    assert [bits(base, k) for k in range(len(cases))] == [bits(run(cases), k) for k in range(len(cases))]                # 0 means 1.07
    worst = [0.0] * 4
    for sf in (1.0, 1.2):
        rows, recs, probs, un = run(cases, scale_factor=sf)
        assert not any(r["status"] for r in recs) and rows == base[0] and [r["mfe_dcal"] for r in recs] == [r["mfe_dcal"] for r in base[1]]
        for k in range(len(cases)):
            err = (abs(recs[k]["energy"] - base[1][k]["energy"]), float(np.abs(probs[k] - base[2][k]).max()), float(np.abs(un[k] - base[3][k]).max()),
                   abs(recs[k]["mfe_frequency"] / base[1][k]["mfe_frequency"] - 1.0))
            worst = [max(a, b) for a, b in zip(worst, err)]
    print(f"\nscale_factor 1.0 / 1.2 against 1.07: largest difference of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of unpaired {worst[2]:.3g}, "
          f"of the share {worst[3]:.3g} (relative)")
    assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= P_TOL and worst[3] <= F_TOL


# ---- 6. other temperatures

@pytest.mark.parametrize("temp", [25.0, 60.0])
def test_gpu_constrained_pf_at_another_temperature(sets, temp):
    install(sets, "synthetic")
    cases = [c for c in TC.exhaustive_batch() if len(c[0]) >= 16][::7]
    assert len(cases) >= 12
    seqs = sorted({c[0] for c in cases})
    enum, energy = enumerated_energies(seqs, temp)
    kt = PF.kt_of(temp)
    raw = run(cases, temp=temp)
    errs = []
    for k, (s, con, u, b) in enumerate(cases):
        Z, P, best = PC.exact_con(s, con, u, b, enum[s], energy[s], kt)
        if best is None:
            assert raw[1][k]["status"] == N.ERR_INFEASIBLE
            continue
        errs.append(against(raw, k, Z, P, best, kt))
    report(f"{temp} C", errs)
    assert len(errs) >= 5
    at37 = run(cases)
    assert [r["status"] for r in at37[1]] == [r["status"] for r in raw[1]] and [r["energy"] for r in at37[1]] != [r["energy"] for r in raw[1]]


# ---- 7. the limits

def test_gpu_constrained_pf_at_its_limits():
    rng = np.random.default_rng(61)
    s60 = "".join(rng.choice(list("ACGU"), 60))
    cases = [(s60, None, None, None), ("A" * (N.PF_MAX_LEN + 1), None, None, None), (s60, "x" + "." * 59, None, None)]
    raw = run(cases)
    assert [r["status"] for r in raw[1]] == [0, N.ERR_TOO_LONG, 0] and raw[2][1] is None and raw[3][1] is None
    check_errors_are_zero(cases, raw)
    soft = np.zeros(60, dtype=np.int32)
    soft[59] = N.MFE_SOFT_MAX + 1
    for where in ("soft_unpaired", "soft_stack"):
        with pytest.raises(N.RafftError) as e:
            mccaskill.pf_constrained_batch_raw([s60, s60], **{where: [None, soft]})
        assert e.value.code == N.ERR_PARAM and "sequence 1" in str(e.value)
    # soft terms far from physical values: 12 000 kcal/mol on the open chain, the only structure of poly-A
    rows, recs, probs, un = mccaskill.pf_constrained_batch_raw(["A" * 60], soft_unpaired=[np.full(60, N.MFE_SOFT_MAX, dtype=np.int32)])
    r = recs[0]
    print(f"\nu = 20000 on 60 A: status {r['status']}, energy {r['energy']!r}, share {r['mfe_frequency']!r}")
    assert r["status"] in (0, N.ERR_CAPACITY) and rows == ["." * 60]
    assert math.isfinite(r["energy"]) and math.isfinite(r["mfe_frequency"]) and np.isfinite(probs[0]).all() and np.isfinite(un[0]).all()
    if r["status"] == 0:
        assert abs(r["energy"] - 12000.0) <= 1e-6 and r["mfe_dcal"] == 60 * N.MFE_SOFT_MAX and not probs[0].any() and (un[0] == 1.0).all()
    else:
        assert r["energy"] == 0.0 and not probs[0].any() and not un[0].any()


# ---- 8. what stands on the probabilities

def test_gpu_mea_over_constrained_probabilities_holds_the_forced_pairs(sets):
    cases, marks = TC.mirror_cases(sets, "builtin")
    picked = [cases[k] for k in marks["adjacent"] + [marks["crossing"]]]
    res = rafft_amd.pf_constrained_batch([c[0] for c in picked], [c[1] for c in picked])
    mea = rafft_amd.mea_from_probs([r.probs for r in res])
    for c, r, m in zip(picked, res, mea):
        i, j = c[1].index("("), c[1].index(")")
        assert MC.pair_table(m.structure)[i] == j and MC.pair_table(r.centroid)[i] == j and r.unpaired is not None
        assert round(r.mfe_energy * 100) == zuker.mfe_constrained(c[0], c[1]).dcal


# ---- 9. the command line as a process

def test_gpu_cli_pf_shape(tmp_path):
    rng = np.random.default_rng(9)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (40, 55)]
    react = [rng.random(len(s)) * 1.5 for s in seqs]
    fa, sh, bpp = tmp_path / "seqs.fa", tmp_path / "r.shape", tmp_path / "out.bpp"
    fa.write_text("".join(f">s{k}\n{s}\n" for k, s in enumerate(seqs)))
    sh.write_text("".join(f">s{k}\n" + "".join(f"{x + 1} {float(v)!r}\n" for x, v in enumerate(r)) for k, r in enumerate(react)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-sf", str(fa), "--batch", "--pf", "--shape", str(sh), "--bpp", str(bpp)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = rafft_amd.pf_constrained_batch(seqs, None, None, [zuker.shape_deigan(x) for x in react])
    assert r.stdout.splitlines() == [cli.format_pf_line(s, w) for s, w in zip(seqs, want)]
    free = rafft_amd.pf_batch(seqs, probs=False)
    assert [w.energy for w in want] != [f.energy for f in free]
    lines = bpp.read_text().splitlines()
    assert lines and all(len(x.split()) == 4 for x in lines) and {x.split()[0] for x in lines} == {"1", "2"}        # (a FASTA file gives --bpp no names: the sequence's number)
    n_pairs = sum(int((np.triu(w.probs, 1) >= 1e-5).sum()) for w in want)
    assert len(lines) == n_pairs
