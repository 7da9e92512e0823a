"""rafft_mea_batch / rafft_mea_probs_batch on a real MI355X (`-m gpu`): the maximum over every structure of short sequences, the
numpy mirror bit for bit (tests/_mea_np.py), the bits of rafft_pf_batch, constructed matrices that tie, errors that stay with
their sequence, the command line.
Bounds.  1e-9 on an expected accuracy: a sum of at most L <= 20 terms of at most 8 each, formed in two orders (below 20 * 160 *
2^-53 < 1e-12).  1e-12 on q: a running sum of at most 20 probabilities against numpy's pairwise sum.  1e-10 relative on the
diversity: at most 20 000 non-negative terms in two orders (2e4 * 2^-53 = 2e-12).  Against the exact ensemble: every P is within
P_TOL of test_gpu_pf and d/dP of 2 P (1 - P) is at most 2 in magnitude, hence 2 * (cells with P > 0) * P_TOL."""
import ctypes
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, mccaskill, params, rafft as R
from conftest import GOLD, ROOT
import _loops as LP
import _mea_np as M
import _pf_np as PF
from test_gpu_pf import P_TOL, TABLES, enumerated, exhaustive_sequences, install, mirror_sequences, rand, sets  # noqa: F401 (sets: a fixture)

pytestmark = pytest.mark.gpu

KT = PF.kt_of(37.0)
GAMMAS = (0.5, 1.0, 4.0)
EA_TOL, Q_TOL, DIV_RTOL = 1e-9, 1e-12, 1e-10


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()


def bits(rows, recs, probs, un, k):
    """everything rafft_mea_batch returns for sequence k, as bytes and integers"""
    r = recs[k]
    return (rows[k], r["status"], r["length"], r["mfe_dcal"], r["n_pairs"], r["dcal"], np.float64(r["energy"]).tobytes(), np.float64(r["mea"]).tobytes(),
            np.float64(r["diversity"]).tobytes(), None if probs is None or probs[k] is None else probs[k].tobytes(), un[k].tobytes())


def well_nested(row):
    LP.pair_table(row)
    return row.count("(") == row.count(")")


# ---- 1. the symbols

def test_gpu_mea_symbols_and_records():
    L = N.lib()
    assert L.rafft_mea_batch is not None and L.rafft_mea_probs_batch is not None
    assert ctypes.sizeof(N.MeaSeq) == 48 and ctypes.sizeof(N.MeaProbsSeq) == 32
    rows, recs, probs, un = mccaskill.mea_batch_raw(["GGGGAAAACCCC"])
    r = recs[0]
    assert rows == ["((((....))))"] and r["status"] == 0 and r["length"] == 12 and r["n_pairs"] == 4 and r["dcal"] == R.eval_structures(["GGGGAAAACCCC"], rows)[0][0] < 0
    assert r["energy"] < r["mfe_dcal"] / 100.0 and 8.0 < r["mea"] <= 12.0 and 0.0 < r["diversity"] < 2.0 and un[0].shape == (12,)
    res = rafft_amd.mea("GGGGAAAACCCC")
    assert res.structure == rows[0] and res.mea == r["mea"] and res.energy_of_structure == r["dcal"] / 100.0 and res.probs is None


# ---- 2. every structure

_PARSED = {}


def parsed(seq):
    """(owner, i, j, n): the pairs of every structure of the enumeration, flat"""
    if seq not in _PARSED:
        rows = enumerated([seq])[0]
        owner, pi, pj = [], [], []
        for a, r in enumerate(rows):
            for i, j in PF.pairs_of(r):
                owner.append(a); pi.append(i); pj.append(j)
        _PARSED[seq] = (np.array(owner, dtype=np.int64), np.array(pi, dtype=np.int64), np.array(pj, dtype=np.int64), len(rows))
    return _PARSED[seq]


def accuracy_of_all(seq, P, q, gamma):
    """expected_accuracy of every structure of the enumeration: the pairs' weights, and q over what they leave unpaired"""
    owner, pi, pj, n = parsed(seq)
    if not len(owner):
        return np.full(n, q.sum())
    return q.sum() + np.bincount(owner, weights=2.0 * gamma * P[pi, pj] - q[pi] - q[pj], minlength=n)


def ensemble_distance(seq, w):
    """sum_a sum_b p_a p_b d_bp(a, b): directly for up to 1500 structures, and through |a| + |b| - 2 |a and b| summed pair by pair"""
    owner, pi, pj, n = parsed(seq)
    p = np.asarray(w) / math.fsum(w)
    if not len(owner):
        return 0.0
    L = len(seq)
    key, inv = np.unique(pi * L + pj, return_inverse=True)
    Pk = np.bincount(inv, weights=p[owner], minlength=len(key))
    by_pair = float((2.0 * Pk * (1.0 - Pk)).sum())
    if n <= 1500:
        X = np.zeros((n, len(key)))
        X[owner, inv] = 1.0
        size = X.sum(axis=1)
        D = size[:, None] + size[None, :] - 2.0 * (X @ X.T)
        direct = float(p @ D @ p)
        assert abs(direct - by_pair) <= 1e-12 * max(1.0, by_pair)
    return by_pair


@pytest.mark.parametrize("which", TABLES)
def test_gpu_mea_equals_the_maximum_over_every_structure(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    all_rows = enumerated(seqs)
    en, st = R.eval_structures([s for s, rr in zip(seqs, all_rows) for _ in rr], [r for rr in all_rows for r in rr])      # one call
    assert not any(st)
    worst = dict(mea=0.0, row=0.0, q=0.0, div=0.0, ens=0.0)
    for gamma in GAMMAS:
        rows, recs, probs, un = mccaskill.mea_batch_raw(seqs, gamma)
        assert [r["status"] for r in recs] == [0] * len(seqs)
        dc, st2 = R.eval_structures(seqs, rows)
        assert not any(st2) and list(dc) == [r["dcal"] for r in recs]
        at = 0
        for k, (s, rr) in enumerate(zip(seqs, all_rows)):
            e = en[at:at + len(rr)]
            at += len(rr)
            P, q, r = probs[k], un[k], recs[k]
            assert rows[k] in rr and r["n_pairs"] == rows[k].count("(")
            worst["mea"] = max(worst["mea"], abs(r["mea"] - float(accuracy_of_all(s, P, q, gamma).max())))
            worst["row"] = max(worst["row"], abs(M.expected_accuracy(rows[k], P, q, gamma) - r["mea"]))
            worst["q"] = max(worst["q"], float(np.abs(q - np.maximum(0.0, 1.0 - (P.sum(axis=0) + P.sum(axis=1)))).max()))
            ref = M.diversity(P)
            worst["div"] = max(worst["div"], abs(r["diversity"] - ref) / ref if ref else abs(r["diversity"]))
            if gamma == GAMMAS[0]:
                ens = ensemble_distance(s, [math.exp(-x / (100.0 * KT)) for x in e])
                assert abs(r["diversity"] - ens) <= 2 * np.count_nonzero(P) * P_TOL, (s, r["diversity"], ens)
                worst["ens"] = max(worst["ens"], abs(r["diversity"] - ens))
        for k in range(4):                                                         # lengths 1-4: the open chain alone
            assert rows[k] == "." * (k + 1) and recs[k]["mea"] == k + 1 and recs[k]["diversity"] == 0.0 and recs[k]["dcal"] == 0
    print(f"\n{which}: largest error of mea {worst['mea']:.3g}, of the row's accuracy {worst['row']:.3g}, of q {worst['q']:.3g}, of the diversity "
          f"{worst['div']:.3g} (relative), against the exact ensemble {worst['ens']:.3g}")
    assert worst["mea"] <= EA_TOL and worst["row"] <= EA_TOL and worst["q"] <= Q_TOL and worst["div"] <= DIV_RTOL


# ---- 3. the mirror, bit for bit

def long_sequence():
    """200 nt: a hairpin of 64, a linker, a hairpin whose last base closes it - the traceback of (0, 199) finds the partner of 199
    beyond position 64, in its second round of 64 candidates"""
    rng = np.random.default_rng(200)
    comp = {"G": "C", "C": "G"}

    def hairpin(n):
        stem = rand(rng, n, "GC")
        return stem + "GAAA" + "".join(comp[c] for c in reversed(stem))
    return hairpin(30) + rand(rng, 72, "GCU", [0.3, 0.3, 0.4]) + hairpin(30)


def test_gpu_mea_equals_the_mirror_bit_for_bit():
    seqs = mirror_sequences() + [long_sequence()]
    assert len(seqs[-1]) == 200
    for gamma in (1.0, 3.0):
        rows, recs, probs, un = mccaskill.mea_batch_raw(seqs, gamma)
        assert not any(r["status"] for r in recs)
        for k, s in enumerate(seqs):
            E, W, cands = M.table(probs[k], un[k], gamma)
            stats = {}
            row = M.traceback(E, W, cands, un[k], stats=stats)
            assert rows[k] == row and np.float64(recs[k]["mea"]).tobytes() == np.float64(E[0, len(s) - 1]).tobytes(), (k, gamma)
            assert abs(M.expected_accuracy(row, probs[k], un[k], gamma) - recs[k]["mea"]) <= 1e-9 * len(s)
            if len(s) == 200:
                n_cand = max(len(c) for c in cands)
                print(f"\n200 nt, gamma {gamma}: up to {n_cand} candidates in a column, the traceback's longest search took {stats['rounds']} rounds of 64, {row.count('(')} pairs")
                assert n_cand > 64 and stats["rounds"] >= 2
    assert sum("(" in r for r in rows) >= 4


# ---- 4. the bits of rafft_pf_batch; same input, same bits

def test_gpu_mea_has_the_bits_of_pf_and_does_not_depend_on_the_batch():
    rng = np.random.default_rng(6)
    seqs = [rand(rng, n) for n in (33, 58, 71, 20, 64, 45, 80, 9)]
    whole = mccaskill.mea_batch_raw(seqs)
    pf_rows, pf_recs, pf_probs = mccaskill.pf_batch_raw(seqs)
    for k in range(len(seqs)):
        assert whole[1][k]["status"] == 0 and whole[1][k]["mfe_dcal"] == pf_recs[k]["mfe_dcal"]
        assert np.float64(whole[1][k]["energy"]).tobytes() == np.float64(pf_recs[k]["energy"]).tobytes()
        assert whole[2][k].tobytes() == pf_probs[k].tobytes()
    want = {s: bits(*whole, k) for k, s in enumerate(seqs)}
    for k in (0, 3, len(seqs) - 1):                                                # alone
        assert bits(*mccaskill.mea_batch_raw([seqs[k]]), 0) == want[seqs[k]]
    for order in (seqs[::-1], [seqs[k] for k in rng.permutation(len(seqs))]):
        got = mccaskill.mea_batch_raw(order)
        assert [bits(*got, k) for k in range(len(order))] == [want[s] for s in order]
    for budget in (2 * 6 * 64 * 64 * 8, 6 * 9 * 9 * 8):                            # two 64-nt sequences a chunk; one sequence a chunk
        got = mccaskill.mea_batch_raw(seqs, workspace_bytes=budget)
        assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs]
    none = mccaskill.mea_batch_raw(seqs, probs=False)                              # prob_out NULL: the same rows and records
    assert none[2] is None and none[0] == whole[0] and none[1] == whole[1]
    # the matrix call on the device's own P: the same q, row, mea and diversity
    rows, recs, un = mccaskill.mea_from_probs_raw([np.minimum(P, 1.0) for P in whole[2]])      # (a P may be one rounding above 1)
    for k in range(len(seqs)):
        if whole[2][k].max() > 1.0:
            continue
        assert rows[k] == whole[0][k] and un[k].tobytes() == whole[3][k].tobytes()
        assert (recs[k]["n_pairs"], recs[k]["mea"], recs[k]["diversity"]) == (whole[1][k]["n_pairs"], whole[1][k]["mea"], whole[1][k]["diversity"])


# ---- 5. constructed matrices

def dyadic_matrix(rng, L, density, eighths):
    P = np.zeros((L, L))
    for i in range(L):
        for j in range(i + 4, L):
            if rng.random() < density:
                P[i, j] = rng.choice(eighths) / 8.0
    return P


def tie_cases():
    """matrices of few distinct values, dense enough that q is 0 nearly everywhere: E then counts weights of equal size and most
    cells are reproduced by several candidates; two sparse ones with q > 0 at the end"""
    rng = np.random.default_rng(55)
    every = tuple(range(1, 9))
    specs = ((9, 1.0, (4,), 1.0), (24, 1.0, (4, 8), 1.0), (24, 0.5, (2, 4), 0.5), (37, 0.6, (4,), 1.0), (37, 0.3, (1, 2, 4, 8), 4.0), (64, 0.5, (4, 8), 1.0),
             (65, 0.2, (8,), 0.5), (70, 0.3, every, 2.0), (129, 0.1, (4, 8), 1.0), (130, 0.1, every, 1.0), (24, 0.1, every, 0.5), (37, 0.05, every, 4.0))
    return [(dyadic_matrix(rng, L, dens, eighths), gamma) for L, dens, eighths, gamma in specs]


def test_gpu_mea_probs_breaks_ties_as_the_definition_does():
    cases = tie_cases()
    n_differs = 0
    for gamma in sorted({g for _, g in cases}):
        mats = [P for P, g in cases if g == gamma]
        rows, recs, un = mccaskill.mea_from_probs_raw(mats, gamma)
        again = mccaskill.mea_from_probs_raw(mats[::-1], gamma, workspace_bytes=1)   # one matrix a chunk, the other order
        assert again[0] == rows[::-1] and again[1] == recs[::-1]
        for k, P in enumerate(mats):
            q = M.unpaired(P)
            assert recs[k]["status"] == 0 and un[k].tobytes() == q.tobytes()        # (sums of eighths are exact)
            row, mea = M.mea(P, q, gamma)
            assert rows[k] == row and recs[k]["mea"] == mea and recs[k]["n_pairs"] == row.count("(")
            assert recs[k]["diversity"] == M.diversity(P)                           # (eighths again)
            n_differs += M.mea(P, q, gamma, last=True)[0] != row
    print(f"\n{len(cases)} matrices of eighths: the last reproducing candidate gives another row on {n_differs}")
    assert n_differs >= 3


def test_gpu_mea_probs_on_index_sensitive_and_certain_matrices():
    mats = []
    for L in (40, 130):
        i, j = np.indices((L, L))
        mats.append(np.where(j - i > 3, (i * L + j + 1.0) / float(L ** 3), 0.0))   # distinct per cell; a position's total stays below 1
    for gamma in (1.0, 2.5):
        rows, recs, un = mccaskill.mea_from_probs_raw(mats, gamma)
        for k, P in enumerate(mats):
            assert len(np.unique(P[P > 0])) == np.count_nonzero(P)
            assert float(np.abs(un[k] - M.unpaired(P)).max()) <= Q_TOL
            row, mea = M.mea(P, un[k], gamma)
            assert rows[k] == row and np.float64(recs[k]["mea"]).tobytes() == np.float64(mea).tobytes()
            assert abs(recs[k]["diversity"] / M.diversity(P) - 1.0) <= DIV_RTOL
    # certain pairs: two hairpins inside a closing helix, nothing else
    want = "((((.(((....)))..((((.....))))..))))."
    C = np.zeros((len(want), len(want)))
    for i, j in M.pairs_of(want):
        C[i, j] = 1.0
    for gamma in GAMMAS:
        (res,) = rafft_amd.mea_from_probs([C], gamma)
        assert res.structure == want and res.mea == 2 * gamma * want.count("(") + want.count(".") and res.diversity == 0.0
        assert res.unpaired.tolist() == [float(c == ".") for c in want] and res.energy is None and res.energy_of_structure is None


def test_gpu_mea_consensus_of_sampled_rows():
    seq = "GGGGAAUUAGCUCAAAUGGUAGAGCGCUCGCUUAGCAUGCGAGAGGUAGCGGGAUCGAUGCCCGCAUUCUCCACCA"
    recs, rows, dcal = mccaskill.sample_batch_raw([seq], 64, seeds=11)
    texts = [r[:-1].tobytes().decode("ascii") for r in rows[0]]
    F = rafft_amd.pair_frequencies(texts)
    assert F.max() <= 1.0 and np.count_nonzero(F) > 10 and float(F[0, :].sum()) <= 1.0
    (res,) = rafft_amd.mea_from_probs([F])
    assert len(res.structure) == len(seq) and well_nested(res.structure) and "(" in res.structure
    assert all(F[i, j] > 0 for i, j in M.pairs_of(res.structure))
    assert abs(M.expected_accuracy(res.structure, F, res.unpaired, 1.0) - res.mea) <= 1e-9 * len(seq)
    assert res.structure == M.mea(F, res.unpaired, 1.0)[0]
    by_objects = rafft_amd.pair_frequencies(rafft_amd.sample(seq, 64, 11))
    assert by_objects.tobytes() == F.tobytes()


# ---- 6. errors

def test_gpu_mea_param_errors_launch_nothing():
    L = N.lib()
    good = "GGGGAAAACCCC"
    alone = mccaskill.mea_batch_raw([good])
    buf = ctypes.create_string_buffer(b"untouched!", 16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (N.MeaSeq * 1)()
    rec[0].status, rec[0].mea = 77, 7.5
    pr, un = np.full((12, 12), 3.25), np.full(12, 2.5)
    pp, up = (ctypes.c_void_p * 1)(pr.ctypes.data), (ctypes.c_void_p * 1)(un.ctypes.data)
    seq = (ctypes.c_char_p * 1)(good.encode())
    ln = (ctypes.c_int * 1)(12)
    for args in ((1, seq, ln, 37.0, 0.0, 0, -1.0, rec, out, pp, up), (1, seq, ln, 37.0, 0.0, 0, float("nan"), rec, out, pp, up),
                 (1, seq, ln, 37.0, 0.0, 0, float("inf"), rec, out, pp, up), (-1, seq, ln, 37.0, 0.0, 0, 1.0, rec, out, pp, up),
                 (1, seq, ln, 37.0, -0.5, 0, 1.0, rec, out, pp, up), (1, seq, ln, 37.0, 0.0, -1, 1.0, rec, out, pp, up), (1, seq, ln, 37.0, 0.0, 0, 1.0, None, out, pp, up)):
        assert L.rafft_mea_batch(*args) == N.ERR_PARAM
        assert buf.value == b"untouched!" and rec[0].status == 77 and rec[0].mea == 7.5 and (pr == 3.25).all() and (un == 2.5).all()
    assert bits(*mccaskill.mea_batch_raw([good], 0.0), 0) == bits(*alone, 0)       # gamma 0 means 1.0
    with pytest.raises(N.RafftError) as e:                                         # the built-in tables are 37 C only
        mccaskill.mea_batch_raw([good], temp=25.0)
    assert e.value.code == N.ERR_TEMP
    # the matrix call: a good matrix, then one with a bad entry - nothing is written, the cell is named
    ok = np.zeros((8, 8))
    ok[0, 7] = 0.75                                                                # (at 0.5 and gamma 1 the pair ties with two unpaired ends, and unpaired is asked first)
    base = mccaskill.mea_from_probs_raw([ok])
    assert base[0] == ["(......)"]
    assert mccaskill.mea_from_probs_raw([ok], 0.0)[:2] == base[:2]                  # gamma 0 means 1.0
    prec = (N.MeaProbsSeq * 2)()
    prec[1].status = 77
    bufs = [ctypes.create_string_buffer(b"untouched!", 16) for _ in range(2)]
    outs = (ctypes.c_void_p * 2)(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_int * 2)(8, 8)
    for value, i, j in ((1.5, 2, 7), (float("nan"), 1, 6), (-0.125, 0, 4), (float("inf"), 3, 7), (0.25, 4, 7), (0.25, 0, 1)):
        bad = np.zeros((8, 8))
        bad[i, j] = value
        bad[5, 2] = 9.0                                                            # below the diagonal: never read
        ptrs = (ctypes.c_void_p * 2)(ok.ctypes.data, bad.ctypes.data)
        assert L.rafft_mea_probs_batch(2, lens, ptrs, 1.0, 0, prec, outs, None) == N.ERR_PARAM
        msg = L.rafft_last_error().decode()
        assert msg.startswith("sequence 1:") and f"({i},{j})" in msg, msg
        assert all(b.value == b"untouched!" for b in bufs) and prec[1].status == 77
    ptrs = (ctypes.c_void_p * 2)(ok.ctypes.data, ok.ctypes.data)
    for gamma in (-1.0, float("nan")):
        assert L.rafft_mea_probs_batch(2, lens, ptrs, gamma, 0, prec, outs, None) == N.ERR_PARAM and prec[1].status == 77
    assert L.rafft_mea_probs_batch(2, lens, ptrs, 1.0, -1, prec, outs, None) == N.ERR_PARAM
    # empty and too long are errors of that matrix only
    lens3 = (ctypes.c_int * 3)(0, 8, N.PF_MAX_LEN + 1)
    bufs3 = [ctypes.create_string_buffer(n) for n in (1, 9, N.PF_MAX_LEN + 2)]
    outs3 = (ctypes.c_void_p * 3)(*[ctypes.addressof(b) for b in bufs3])
    ptrs3 = (ctypes.c_void_p * 3)(None, ok.ctypes.data, None)
    prec3 = (N.MeaProbsSeq * 3)()
    assert L.rafft_mea_probs_batch(3, lens3, ptrs3, 1.0, 0, prec3, outs3, None) == 0
    assert [r.status for r in prec3] == [N.ERR_EMPTY, 0, N.ERR_TOO_LONG] and L.rafft_last_error().decode().startswith("sequence 0:")
    assert bufs3[1].value == b"(......)" and prec3[1].mea == base[1][0]["mea"] and bufs3[2].value == b"." * (N.PF_MAX_LEN + 1) and prec3[2].mea == 0.0
    with pytest.raises(ValueError):
        rafft_amd.mea_from_probs([np.zeros((0, 0))])


def test_gpu_mea_errors_stay_with_their_sequence():
    good = ["GGGGAAAACCCC", "GGGAAACCCAGGGAAACCC", "GCGCUUCGGCGC", "ACGUACGUACGUACGUAGC"]
    alone = mccaskill.mea_batch_raw(good)
    seqs = [good[0], "", good[1], "GGGXAAACCC", good[2], "A" * (N.PF_MAX_LEN + 1), good[3]]
    rows, recs, probs, un = mccaskill.mea_batch_raw(seqs)
    assert [r["status"] for r in recs] == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, 0, N.ERR_TOO_LONG, 0]
    assert N.lib().rafft_last_error().decode().startswith("sequence 1")
    assert [rows[k] for k in (1, 3, 5)] == ["", "." * 10, "." * (N.PF_MAX_LEN + 1)]
    assert all(recs[k]["energy"] == 0.0 and recs[k]["n_pairs"] == 0 and recs[k]["mea"] == 0.0 and recs[k]["diversity"] == 0.0 and recs[k]["dcal"] == 0 for k in (1, 3, 5))
    assert not probs[3].any() and probs[5] is None and not un[3].any()
    assert [bits(rows, recs, probs, un, k) for k in (0, 2, 4, 6)] == [bits(*alone, k) for k in range(4)]
    got = rafft_amd.mea_batch(seqs, raise_errors=False)
    assert [g is None for g in got] == [False, True, False, True, False, True, False] and got[0].structure == rows[0]
    with pytest.raises(KeyError):
        rafft_amd.mea_batch(seqs[2:4])


def test_gpu_mea_reports_a_sequence_whose_scaled_sums_leave_the_fp64_range():
    """the construction of test_gpu_pf: a helix of 200 GC stacks between two ordinary sequences, under a scale of practically 1
    (overflow) and one far too large (underflow): it - and only it - gets RAFFT_ERR_CAPACITY, an all-dot row and zeros"""
    rng = np.random.default_rng(404)
    big, left, right = "G" * 200 + "GAAA" + "C" * 200, rand(rng, 40), rand(rng, 25)
    seqs = [left, big, right]
    for sf in (1e-9, 3.0):
        without = mccaskill.mea_batch_raw([left, right], scale_factor=sf)
        assert not any(x["status"] for x in without[1])
        rows, recs, probs, un = mccaskill.mea_batch_raw(seqs, scale_factor=sf)
        r = recs[1]
        assert [x["status"] for x in recs] == [0, N.ERR_CAPACITY, 0], sf
        assert N.lib().rafft_last_error().decode().startswith("sequence 1:")
        assert rows[1] == "." * len(big) and r["length"] == len(big) and r["mfe_dcal"] < -60000
        assert r["energy"] == 0.0 and r["mea"] == 0.0 and r["diversity"] == 0.0 and r["n_pairs"] == 0 and r["dcal"] == 0
        assert not probs[1].any() and not un[1].any()
        assert [bits(rows, recs, probs, un, 0), bits(rows, recs, probs, un, 2)] == [bits(*without, 0), bits(*without, 1)]
    rows, recs, probs, un = mccaskill.mea_batch_raw(seqs)                          # the default scale holds it
    assert recs[1]["status"] == 0 and rows[1].count("(") >= 195 and recs[1]["dcal"] == R.eval_structures([big], [rows[1]])[0][0]


# ---- 7. the command line as a process, with the real scorer

def test_gpu_cli_mea(tmp_path):
    from rafft_amd import cli, scoring
    with gzip.open(os.path.join(GOLD, "bench_inputs.tsv.gz"), "rt") as fh:
        bench = [line.rstrip("\n").split("\t") for line in fh]
    picked = sorted(bench, key=lambda f: len(f[1]))[::len(bench) // 6][:6]
    rows = [(f[1], f[8], f[0]) for f in picked]
    csvf = tmp_path / "known.csv"
    csvf.write_text("".join(f"{s},{k},{n}\n" for s, k, n in rows))
    out, lines = tmp_path / "scores.csv", tmp_path / "lines.txt"
    exe = [sys.executable, os.path.join(ROOT, "bin", "rafft")]
    r = subprocess.run(exe + ["-sf", str(csvf), "--batch", "--mea", "2.0", "--scores", str(out), "-o", str(lines)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = out.read_text().splitlines()
    assert got[0] == "seq,len_seq,struct,nrj,nbp,pvv,sens,name" and len(got) == 1 + len(rows)
    want = rafft_amd.mea_batch([x[0] for x in rows], 2.0)
    for line, (s, known, name), res in zip(got[1:], rows, want):
        ppv, sens = scoring.score(res.structure, known)
        assert line == f"{s},{len(s)},{res.structure},{res.energy_of_structure},{res.structure.count('(')},{round(ppv, 2)},{round(sens, 2)},{name}"
    assert lines.read_text().splitlines() == [cli.format_mea_line(x[0], res) for x, res in zip(rows, want)]
    assert any("(" in res.structure for res in want)
    r = subprocess.run(exe + ["-s", rows[0][0], "--pf", "--mea"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and cli.MEA_EXCLUSIVE in r.stderr
    # --sample N --mea: the consensus of the sampled rows in place of the graph text
    s = rows[1][0]
    r = subprocess.run(exe + ["-s", s, "--sample", "64", "--seed", "11", "--mea", "2.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    (res,) = rafft_amd.mea_from_probs([rafft_amd.pair_frequencies(rafft_amd.sample(s, 64, 11))], 2.0)
    assert r.stdout == cli.format_consensus_line(s, res) + "\n" and well_nested(res.structure)
