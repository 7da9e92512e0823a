"""rafft_pf_batch on a real MI355X (`-m gpu`): Z and every P(i,j) against the sums over every structure of short sequences (evaluated
by eval_kernel in one call, summed with fsum), against the tests' own mirror where enumeration cannot reach, invariance under the
scale, a sequence an unscaled fp64 sum could not hold, one whose scaled sums leave the fp64 range in either direction, other
temperatures under a parameter file with enthalpies, same input - same bits across batch position, order and chunking, and errors
that stay with their sequence.
The bounds - 1e-8 kcal/mol on the ensemble energy, 1e-9 on a probability, 1e-9 relative on the MFE's share - are what fp64 sums of
positive terms leave (a few thousand operations times 2^-53) with two orders of margin; they are not measured values."""
import ctypes
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, mccaskill, params, rafft as R, zuker
from conftest import GOLD, ROOT
import _loops as LP
import _mfe_np as MF
import _par_reader as PR
import _pf_np as PF

pytestmark = pytest.mark.gpu

TABLES = ("builtin", "multiloops_win")
KT = PF.kt_of(37.0)
E_TOL, P_TOL, F_TOL = 1e-8, 1e-9, 1e-9
MULTILOOP_SEQS = ["GAGAAACGAAACGAAACC", "GAGAAACGAAACGAAACAC", "GAAGAAACGAAACGAAACC", "GUGAAACGAAACGAAACAU", "GAGAAACGAAACGAAACCA"]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    idx.update(ml_closing=-700, ml_intern=-300)               # negative enough that multiloops hold most of Z at 16-20 nt
    out = dict(builtin=builtin, multiloops_win=idx, synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name, comment in (("multiloops_win", "index-sensitive, multiloops win"), ("synthetic", "made-up enthalpies")):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=comment)
    return out


def install(sets, which):
    if which == "builtin":
        params.reset_params()
    else:
        params.load_params(sets["paths"][which])


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()


def bits(rows, recs, probs, k):
    """everything rafft_pf_batch returns for sequence k, as bytes and integers"""
    r = recs[k]
    return (rows[k], r["status"], r["mfe_dcal"], r["n_pairs"], np.float64(r["energy"]).tobytes(), np.float64(r["mfe_frequency"]).tobytes(),
            None if probs is None else probs[k].tobytes())


def rand(rng, n, letters="ACGU", p=None):
    return "".join(rng.choice(list(letters), n, p=p))


# ---- 1. the symbol

def test_gpu_pf_symbol_and_record():
    assert N.lib().rafft_pf_batch is not None and ctypes.sizeof(N.PfSeq) == 32
    rows, recs, probs = mccaskill.pf_batch_raw(["GGGGAAAACCCC"])
    assert rows == ["((((....))))"] and recs[0]["status"] == 0 and recs[0]["length"] == 12 and recs[0]["n_pairs"] == 4
    assert recs[0]["energy"] < recs[0]["mfe_dcal"] / 100.0 < 0 and 0.5 < recs[0]["mfe_frequency"] < 1.0 and probs[0][0, 11] > 0.5      # (a centroid pair)


# ---- 2. every structure

def exhaustive_sequences():
    rng = np.random.default_rng(1971)
    seqs = ["A", "GC", "GAC", "GAAC"]                                              # lengths 1-4: the open chain alone
    seqs += [rand(rng, n) for n in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20, 20, 20)]
    seqs += [rand(rng, n, "GCU") for n in (14, 16, 17)]
    for name in LP.KINDS:                                                          # GC hairpins around the special loops
        for sp in LP.OWN_SPECIAL[name]:
            seqs.append("GG" + sp + "CC")
    seqs += ["GGGACACCCAGGACCACCC", "G" * 10 + "U" * 10, "GU" * 9, "GGGUUUGGGUUUCCC", "GCGCAAAGCGCAAAGCGC", "GGGAAACCCAGGGAAACCCA", "NGGGAAACCCN"]
    return seqs + LP.N_SEQS + MULTILOOP_SEQS


_ENUM = {}


def enumerated(seqs):
    for s in seqs:
        if s not in _ENUM:
            _ENUM[s] = MF.enumerate_structures(s)
    return [_ENUM[s] for s in seqs]


@pytest.mark.parametrize("which", TABLES)
def test_gpu_pf_equals_the_sums_over_every_structure(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    assert 44 <= len(seqs) <= 59 and max(map(len, seqs)) == 20 and sum("N" in s for s in seqs) == 5
    rows = enumerated(seqs)
    flat_s = [s for s, rr in zip(seqs, rows) for _ in rr]
    flat_r = [r for rr in rows for r in rr]
    en, st = R.eval_structures(flat_s, flat_r)                                     # one call
    assert not any(st)
    got_rows, recs, probs = mccaskill.pf_batch_raw(seqs)
    mfe = zuker.mfe_batch_raw(seqs)
    assert [r["status"] for r in recs] == [0] * len(seqs)
    assert [r["mfe_dcal"] for r in recs] == mfe[1]
    worst_e = worst_p = worst_f = 0.0
    at, n_leading = 0, 0
    for k, (s, rr) in enumerate(zip(seqs, rows)):
        e = en[at:at + len(rr)]
        at += len(rr)
        Z, P = PF.exact(rr, e, KT)
        worst_e = max(worst_e, abs(recs[k]["energy"] - (-KT * math.log(Z))))
        worst_p = max(worst_p, float(np.abs(probs[k] - P).max()))
        f = math.exp(-min(e) / (100.0 * KT)) / Z
        worst_f = max(worst_f, abs(recs[k]["mfe_frequency"] / f - 1.0))
        assert min(e) == recs[k]["mfe_dcal"]
        lead = math.fsum(math.exp(-x / (100.0 * KT)) for r, x in zip(rr, e) if PF.has_leading_unpaired_multiloop(r)) / Z
        n_leading += lead > 1e-3
    print(f"\n{which}: largest error of the energy {worst_e:.3g} kcal/mol, of P {worst_p:.3g}, of the MFE share {worst_f:.3g} (relative)")
    assert worst_e <= E_TOL and worst_p <= P_TOL and worst_f <= F_TOL
    assert got_rows[:4] == [".", "..", "...", "...."] and all(r["energy"] == 0.0 and r["mfe_frequency"] == 1.0 for r in recs[:4])
    if which == "multiloops_win":
        assert n_leading >= 3                                                      # an ambiguous M would not pass (tests/test_pf_host.py)


# ---- 3. against the mirror where enumeration cannot reach

def mirror_sequences():
    rng = np.random.default_rng(78)
    seqs = [rand(rng, n) for n in (60, 75, 90)]
    # one good helix pair separated by an A-run on one side: 30 is an allowed bulge, 31 is not
    for run in (30, 31):
        seqs.append("GGGCG" + "A" * run + "GCGCG" + "GAAA" + "CGCGC" + "CGCCC")
    return seqs


_MIRROR = {}


@pytest.mark.parametrize("which", TABLES)
def test_gpu_pf_equals_the_mirror_at_60_to_90_nt(sets, which):
    install(sets, which)
    seqs = mirror_sequences()
    if which not in _MIRROR:
        m = PF.PfMirror(PR.tables_at(sets[which], 37.0))
        _MIRROR[which] = [m.run(s) for s in seqs]
    rows, recs, probs = mccaskill.pf_batch_raw(seqs)
    assert not any(r["status"] for r in recs)
    worst_e = max(abs(recs[k]["energy"] - (-KT * math.log(z))) for k, (z, _) in enumerate(_MIRROR[which]))
    worst_p = max(float(np.abs(probs[k] - p).max()) for k, (_, p) in enumerate(_MIRROR[which]))
    print(f"\n{which}: largest error of the energy {worst_e:.3g} kcal/mol, of P {worst_p:.3g}")
    assert worst_e <= E_TOL and worst_p <= P_TOL
    if which == "builtin":
        # the cap decides these two: in the mirror the outer helix over the bulge of 30 is nearly certain, and without the bulge
        # of 31 it is nearly absent - the device follows both
        (_, p30), (_, p31) = _MIRROR[which][-2:]
        assert p30[4, len(seqs[-2]) - 5] > 0.99 and p31[4, len(seqs[-1]) - 5] < 0.01
        assert rows[-2].startswith("(((((" + "." * 30 + "(((((") and not rows[-1].startswith("(")


# ---- 4. the scale

def test_gpu_pf_does_not_depend_on_the_scale():
    rng = np.random.default_rng(4)
    seqs = [rand(rng, n) for n in (150, 220, 300)]
    base = mccaskill.pf_batch_raw(seqs, scale_factor=1.07)
    assert not any(r["status"] for r in base[1])
    assert [bits(*base, k) for k in range(3)] == [bits(*mccaskill.pf_batch_raw(seqs), k) for k in range(3)]      # 0 means 1.07
    worst_e = worst_p = 0.0
    for sf in (0.5, 1.5):
        rows, recs, probs = mccaskill.pf_batch_raw(seqs, scale_factor=sf)
        assert not any(r["status"] for r in recs) and rows == base[0]
        worst_e = max(worst_e, max(abs(a["energy"] - b["energy"]) for a, b in zip(recs, base[1])))
        worst_p = max(worst_p, max(float(np.abs(a - b).max()) for a, b in zip(probs, base[2])))
    print(f"\nscale_factor 0.5 / 1.5 against 1.07: largest difference of the energy {worst_e:.3g} kcal/mol, of P {worst_p:.3g}")
    assert worst_e <= E_TOL and worst_p <= P_TOL


# ---- 5. the range

def test_gpu_pf_holds_a_sequence_an_unscaled_sum_could_not():
    rng = np.random.default_rng(1500)
    big, small = rand(rng, 1500, "ACGU", [0.1, 0.4, 0.4, 0.1]), rand(rng, 30)
    rows, recs, probs = mccaskill.pf_batch_raw([big, small])
    r = recs[0]
    print(f"\n1500 nt: MFE {r['mfe_dcal']} dcal/mol, ensemble energy {r['energy']:.4f} kcal/mol, MFE share {r['mfe_frequency']:.3g}, {r['n_pairs']} centroid pairs")
    assert r["mfe_dcal"] < -45000                                                  # exp(450 / kT) is far above the fp64 range
    assert r["status"] == N.OK
    assert math.isfinite(r["energy"]) and r["energy"] <= r["mfe_dcal"] / 100.0
    P = probs[0]
    assert np.isfinite(P).all() and P.min() >= 0.0
    per_base = P.sum(axis=0) + P.sum(axis=1)
    print(f"largest sum of P over the partners of a position: 1 + {per_base.max() - 1.0:.3g}")
    assert per_base.max() <= 1.0 + 1e-9
    en, st = R.eval_structures([big], [rows[0]])
    assert st == [0] and r["n_pairs"] == rows[0].count("(") > 100
    alone = mccaskill.pf_batch_raw([small])
    assert bits(rows, recs, probs, 1) == bits(*alone, 0)


def test_gpu_pf_reports_a_sequence_whose_scaled_sums_leave_the_fp64_range():
    """a helix of 200 GC stacks between two ordinary sequences.  With a scale of practically 1 its sums overflow, with a scale far too
    large they underflow to 0: in both calls it - and only it - gets RAFFT_ERR_CAPACITY, an all-dot row and zeros (mfe_dcal keeps the
    MFE's energy, which the driver has before the sums are formed); with the default scale it is held"""
    rng = np.random.default_rng(404)
    big, left, right = "G" * 200 + "GAAA" + "C" * 200, rand(rng, 40), rand(rng, 25)
    seqs = [left, big, right]
    mfe = zuker.mfe_batch_raw([big])[1][0]
    print(f"\n404 nt: MFE {mfe} dcal/mol")
    assert mfe < -60000                                                            # exp(437.4 / kT) is the largest fp64 at 37 C
    for sf in (1e-9, 3.0):
        without = mccaskill.pf_batch_raw([left, right], scale_factor=sf)           # (a sequence's bits depend on the scale)
        assert not any(x["status"] for x in without[1])
        rows, recs, probs = mccaskill.pf_batch_raw(seqs, scale_factor=sf)
        r = recs[1]
        assert [x["status"] for x in recs] == [0, N.ERR_CAPACITY, 0], sf
        assert N.lib().rafft_last_error().decode().startswith("sequence 1:")
        assert rows[1] == "." * len(big) and r["energy"] == 0.0 and r["mfe_frequency"] == 0.0 and r["n_pairs"] == 0 and r["length"] == len(big)
        assert r["mfe_dcal"] == mfe
        assert probs[1].shape == (len(big), len(big)) and not probs[1].any()
        assert [bits(rows, recs, probs, 0), bits(rows, recs, probs, 2)] == [bits(*without, 0), bits(*without, 1)]
        rows2, recs2, none = mccaskill.pf_batch_raw(seqs, scale_factor=sf, probs=False)
        assert none is None and rows2 == rows and recs2 == recs
    without = mccaskill.pf_batch_raw([left, right])
    rows, recs, probs = mccaskill.pf_batch_raw(seqs)
    r, P = recs[1], probs[1]
    assert r["status"] == N.OK and r["mfe_dcal"] == mfe and math.isfinite(r["energy"]) and r["energy"] <= mfe / 100.0
    assert np.isfinite(P).all() and P.min() >= 0.0
    per_base = P.sum(axis=0) + P.sum(axis=1)
    print(f"default scale: ensemble energy {r['energy']:.4f} kcal/mol, {r['n_pairs']} centroid pairs, largest sum of P over the partners of a position: 1 + {per_base.max() - 1.0:.3g}")
    assert per_base.max() <= 1.0 + 1e-9
    assert [bits(rows, recs, probs, 0), bits(rows, recs, probs, 2)] == [bits(*without, 0), bits(*without, 1)]


# ---- 6. other temperatures

def exact_errors(seqs, recs, probs, temp):
    """largest errors of the energy, of P and of the MFE's share against the exact sums over every structure of each sequence, under
    the installed tables at `temp` (one eval_kernel call)"""
    kt = PF.kt_of(temp)
    rows = enumerated(seqs)
    en, st = R.eval_structures([s for s, rr in zip(seqs, rows) for _ in rr], [r for rr in rows for r in rr], temp=temp)
    assert not any(st)
    worst_e = worst_p = worst_f = 0.0
    at = 0
    for k, rr in enumerate(rows):
        e = en[at:at + len(rr)]
        at += len(rr)
        Z, P = PF.exact(rr, e, kt)
        assert min(e) == recs[k]["mfe_dcal"]
        worst_e = max(worst_e, abs(recs[k]["energy"] - (-kt * math.log(Z))))
        worst_p = max(worst_p, float(np.abs(probs[k] - P).max()))
        worst_f = max(worst_f, abs(recs[k]["mfe_frequency"] / (math.exp(-min(e) / (100.0 * kt)) / Z) - 1.0))
    return worst_e, worst_p, worst_f


_MIRROR_T = {}


@pytest.mark.parametrize("temp", [25.0, 60.0])
def test_gpu_pf_at_another_temperature(sets, temp):
    """a parameter file with (made-up) enthalpies: kT and the tables are those of the call's temperature - against the exact sums
    with eval_kernel's energies at that temperature and kt_of(temp), and against the mirror over tables rescaled by the tests' own
    reader at 60-90 nt; the bounds are those of 37 C (their derivation does not involve kT); 37 C comes back afterwards"""
    install(sets, "synthetic")
    short, longer = exhaustive_sequences(), mirror_sequences()
    at37 = mccaskill.pf_batch_raw(short + longer)
    rows, recs, probs = mccaskill.pf_batch_raw(short, temp=temp)
    assert not any(r["status"] for r in recs)
    worst_e, worst_p, worst_f = exact_errors(short, recs, probs, temp)
    print(f"\n{temp} C, every structure: largest error of the energy {worst_e:.3g} kcal/mol, of P {worst_p:.3g}, of the MFE share {worst_f:.3g} (relative)")
    assert worst_e <= E_TOL and worst_p <= P_TOL and worst_f <= F_TOL
    if temp not in _MIRROR_T:
        m = PF.PfMirror(PR.tables_at(sets["synthetic"], temp), temp)
        _MIRROR_T[temp] = [m.run(s) for s in longer]
    kt = PF.kt_of(temp)
    rows, recs, probs = mccaskill.pf_batch_raw(longer, temp=temp)
    assert not any(r["status"] for r in recs)
    worst_e = max(abs(recs[k]["energy"] - (-kt * math.log(z))) for k, (z, _) in enumerate(_MIRROR_T[temp]))
    worst_p = max(float(np.abs(probs[k] - p).max()) for k, (_, p) in enumerate(_MIRROR_T[temp]))
    print(f"{temp} C, mirror at 60-90 nt: largest error of the energy {worst_e:.3g} kcal/mol, of P {worst_p:.3g}")
    assert worst_e <= E_TOL and worst_p <= P_TOL
    # kT differs by 4 % and 7 % from 310.15 K's and every table is rescaled: ensemble energies of -5 to -30 kcal/mol move by far more
    # than the bound - a kT or a table left at 37 C cannot pass
    shift = [abs(recs[k]["energy"] - at37[1][len(short) + k]["energy"]) for k in range(len(longer))]
    print(f"{temp} C: the ensemble energies differ from those at 37 C by {min(shift):.3g} to {max(shift):.3g} kcal/mol")
    assert min(shift) > 1e5 * E_TOL
    again = mccaskill.pf_batch_raw(short + longer)
    assert [bits(*again, k) for k in range(len(short + longer))] == [bits(*at37, k) for k in range(len(short + longer))]


# ---- 7. same input, same bits

def test_gpu_pf_same_input_same_bits():
    rng = np.random.default_rng(6)
    seqs = [rand(rng, n) for n in (33, 58, 71, 20, 64, 45, 80, 9)]
    whole = mccaskill.pf_batch_raw(seqs)
    want = {s: bits(*whole, k) for k, s in enumerate(seqs)}
    for k in (0, 3, len(seqs) - 1):                                                # alone
        assert bits(*mccaskill.pf_batch_raw([seqs[k]]), 0) == want[seqs[k]]
    for order in (seqs[::-1], [seqs[k] for k in rng.permutation(len(seqs))], seqs[1:] + seqs[:1]):
        got = mccaskill.pf_batch_raw(order)
        assert [bits(*got, k) for k in range(len(order))] == [want[s] for s in order]
    # several chunks: room for the tables of two 64-nt sequences, then for those of one 9-nt sequence
    for budget in (2 * 6 * 64 * 64 * 8, 6 * 9 * 9 * 8):
        got = mccaskill.pf_batch_raw(seqs, workspace_bytes=budget)
        assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs]


# ---- 8. sanity at 100-200 nt

def test_gpu_pf_sanity_at_100_to_200_nt():
    rng = np.random.default_rng(7)
    seqs = [rand(rng, int(n)) for n in rng.integers(100, 201, 20)]
    rows, recs, probs = mccaskill.pf_batch_raw(seqs)
    rows2, recs2, none = mccaskill.pf_batch_raw(seqs, probs=False)
    assert none is None and rows2 == rows and recs2 == recs                        # prob_out NULL: the same row and record
    for s, row, r, P in zip(seqs, rows, recs, probs):
        L = len(s)
        assert r["status"] == 0 and r["length"] == L
        i, j = np.indices((L, L))
        can = np.array([[(a + b) in MF.PAIRS for b in s] for a in s])
        assert not P[~can | (j - i < 4)].any()
        assert 0.0 <= P.min() and P.max() <= 1.0 + 1e-12
        assert r["energy"] <= min(0.0, r["mfe_dcal"] / 100.0) and 0.0 < r["mfe_frequency"] <= 1.0
        db = ["."] * L
        for a, b in zip(*np.nonzero(P > 0.5)):
            assert db[a] == "." and db[b] == "."                                   # no base twice
            db[a], db[b] = "(", ")"
        assert "".join(db) == row and r["n_pairs"] == row.count("(")
        LP.pair_table(row)                                                         # well nested
    en, st = R.eval_structures(seqs, rows)
    assert not any(st)


# ---- 9. errors stay with their sequence

def test_gpu_pf_errors_stay_with_their_sequence():
    good = ["GGGGAAAACCCC", "GGGAAACCCAGGGAAACCC", "GCGCUUCGGCGC", "ACGUACGUACGUACGUAGC"]
    alone = mccaskill.pf_batch_raw(good)
    seqs = [good[0], "", good[1], "GGGXAAACCC", good[2], "A" * (N.PF_MAX_LEN + 1), good[3]]
    rows, recs, probs = mccaskill.pf_batch_raw(seqs)                                # returns: the call is RAFFT_OK
    assert [r["status"] for r in recs] == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, 0, N.ERR_TOO_LONG, 0]
    assert N.lib().rafft_last_error().decode().startswith("sequence 1")
    assert [rows[k] for k in (1, 3, 5)] == ["", "." * 10, "." * (N.PF_MAX_LEN + 1)]
    assert all(recs[k]["energy"] == 0.0 and recs[k]["n_pairs"] == 0 and recs[k]["mfe_frequency"] == 0.0 for k in (1, 3, 5))
    assert not probs[3].any() and probs[5] is None
    assert [bits(rows, recs, probs, k) for k in (0, 2, 4, 6)] == [bits(*alone, k) for k in range(4)]
    got = rafft_amd.pf_batch(seqs, raise_errors=False)
    assert [g is None for g in got] == [False, True, False, True, False, True, False]
    assert got[0].centroid == rows[0] and got[0].energy == recs[0]["energy"] and got[0].mfe_energy == recs[0]["mfe_dcal"] / 100.0
    assert np.array_equal(got[0].probs, probs[0]) and rafft_amd.pf(good[0], probs=False).probs is None
    with pytest.raises(KeyError):
        rafft_amd.pf_batch(seqs[2:4])
    # RAFFT_ERR_PARAM: the outputs are not touched, and the next call is exact
    L = N.lib()
    buf = ctypes.create_string_buffer(b"untouched!", 16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (N.PfSeq * 1)()
    rec[0].status, rec[0].energy = 77, 7.5
    pr = np.full((12, 12), 3.25)
    pp = (ctypes.c_void_p * 1)(pr.ctypes.data)
    seq = (ctypes.c_char_p * 1)(good[0].encode())
    ln = (ctypes.c_int * 1)(12)
    for args in ((-1, seq, ln, 37.0, 0.0, 0, rec, out, pp), (1, None, ln, 37.0, 0.0, 0, rec, out, pp), (1, seq, ln, 37.0, 0.0, 0, None, out, pp),
                 (1, seq, ln, 37.0, -0.5, 0, rec, out, pp), (1, seq, ln, 37.0, float("nan"), 0, rec, out, pp), (1, seq, ln, 37.0, float("inf"), 0, rec, out, pp),
                 (1, seq, ln, 37.0, 0.0, -1, rec, out, pp)):
        assert L.rafft_pf_batch(*args) == N.ERR_PARAM
        assert buf.value == b"untouched!" and rec[0].status == 77 and rec[0].energy == 7.5 and (pr == 3.25).all()
        assert bits(*mccaskill.pf_batch_raw(good[:1]), 0) == bits(*alone, 0)
    for batch in (good, ["", "GGGXAACCC"]):                                        # the built-in tables are 37 C only, as for the fold
        with pytest.raises(N.RafftError) as e:
            mccaskill.pf_batch_raw(batch, temp=25.0)
        assert e.value.code == N.ERR_TEMP


# ---- 10. the command line as a process, with the real scorer

def test_gpu_cli_pf_scores_table(tmp_path):
    from rafft_amd import cli, scoring
    with gzip.open(os.path.join(GOLD, "bench_inputs.tsv.gz"), "rt") as fh:
        bench = [line.rstrip("\n").split("\t") for line in fh]
    picked = sorted(bench, key=lambda f: len(f[1]))[::len(bench) // 6][:6]
    rows = [(f[1], f[8], f[0]) for f in picked]
    csvf = tmp_path / "known.csv"
    csvf.write_text("".join(f"{s},{k},{n}\n" for s, k, n in rows))
    out, lines = tmp_path / "scores.csv", tmp_path / "lines.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-sf", str(csvf), "--batch", "--pf", "--scores", str(out), "-o", str(lines)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = out.read_text().splitlines()
    assert got[0] == "seq,len_seq,struct,nrj,nbp,pvv,sens,name" and len(got) == 1 + len(rows)
    want = rafft_amd.pf_batch([x[0] for x in rows], probs=False)
    for line, (s, known, name), res in zip(got[1:], rows, want):
        ppv, sens = scoring.score(res.centroid, known)
        assert line == f"{s},{len(s)},{res.centroid},{res.energy},{res.centroid.count('(')},{round(ppv, 2)},{round(sens, 2)},{name}"
    assert lines.read_text().splitlines() == [cli.format_pf_line(x[0], res) for x, res in zip(rows, want)]
    assert any("(" in res.centroid for res in want)
