"""The dynamic-programming kernels of the batch drivers past the second round of their 64-candidate loops, on a real MI355X
(`-m gpu`): rafft_pf_batch, rafft_mfe_batch, rafft_mfe_constrained_batch, rafft_subopt_batch, rafft_sample_batch, rafft_mea_batch,
rafft_pf_span_batch and rafft_mfe_span_batch against the tests' numpy mirrors at 133-261 nt, where a C or M split has up to 250
candidates, the exterior loop 257 and an outside sum as many (tests/_lane_rounds.py builds the inputs; tests/test_lane_rounds.py
shows that each of them tells a loop that stops after two or three rounds from the right one by a thousand bounds and more).
The bounds are those of tests/test_gpu_pf.py and tests/test_gpu_pf_span.py, imported: a few thousand operations times 2^-53 with two
orders of margin holds at 261 nt as it does at 90.  Rows, energies in dcal and bands are integers and bytes: no tolerance.
Measured on an MI355X: the file takes 23 s, 20 s of it the numpy mirrors (9 s in the first test, which fills the cache the later
ones read).  Largest errors:
    built-in, 9-261 nt     energy 2.8e-14 kcal/mol   P 3.7e-15   MFE share 4.6e-14
    multiloops_win, 197 nt energy 0                  P 1.1e-15   MFE share 0
    25 C, 197 nt           energy 3.6e-15            P 1.0e-15   MFE share 5.9e-15
    span 130 / 200         energy 7.1e-15 / 2.8e-14  P 1.6e-15 / 2.7e-15   unpaired 1.7e-15 / 2.8e-15
    5000 samples           the largest deviation of a pair count is 0.49 (197 nt) and 0.41 (261 nt) of what the check allows
Pairs with j - i >= 128 hold 0.15 (197 nt), 0.34 (261 nt) and 0.23 (FAR_BRANCH) of the pair probability; 11, 12, 31 and 8 structures
lie within 60 dcal.
"""
import math

import numpy as np
import pytest

from rafft_amd import _native as N, mccaskill, params, rafft as R, wuchty, zuker
import _lane_rounds as LR
import _par_reader as PR
import _pf_np as PF
import _sample_stats as ST
from test_gpu_mfe import check_rows
from test_gpu_mfe_constrained import check_rows as check_constrained_rows, run as run_constrained
from test_gpu_mfe_span import check_span_rows, triples
from test_gpu_pf import E_TOL, F_TOL, P_TOL
from test_gpu_pf_span import against_mirror, centroid_of
from test_gpu_sample import distinct, loops_ok, pair_counts
from test_gpu_subopt import evaluate_back, pairs_of

pytestmark = pytest.mark.gpu

KT = PF.kt_of(37.0)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    out = dict(LR.par_sets(), paths={})
    d = tmp_path_factory.mktemp("par")
    for name in ("multiloops_win", "tie0", "tie1", "synthetic"):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=name)
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


def pf_errors(seqs, got, want, kt, mfe):
    """largest errors of the energy, of P and of the MFE's share against [(energy, P)] of a mirror; the MFE is the MFE mirror's, the
    centroid the mirror's P > 0.5"""
    rows, recs, probs = got
    worst_e = worst_p = worst_f = 0.0
    for k, (e, P) in enumerate(want):
        r = recs[k]
        assert r["status"] == 0 and r["length"] == len(seqs[k]) and r["mfe_dcal"] == mfe[k]
        worst_e = max(worst_e, abs(r["energy"] - e))
        worst_p = max(worst_p, float(np.abs(probs[k] - P).max()))
        worst_f = max(worst_f, abs(r["mfe_frequency"] / math.exp((e - mfe[k] / 100.0) / kt) - 1.0))
        if not (np.abs(P - 0.5) <= P_TOL).any():
            assert rows[k] == centroid_of(P) and r["n_pairs"] == rows[k].count("(")
    return worst_e, worst_p, worst_f


def far_share(P, d):
    """the share of the pair probability that lies on pairs with j - i >= d"""
    return float(np.triu(P, d).sum() / P.sum())


# ---- 1. the partition function

@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_gpu_pf_equals_the_mirror_through_every_round(sets, which):
    """one call per table set, beside a 9-nt and a 64-nt sequence (Lmax differs from L).  Under `multiloops_win` the 197-nt sequence
    has its minimum at -535 kcal/mol: the mirror is the scaled one"""
    install(sets, which)
    seqs = LR.SHORT + (LR.SEQS if which == "builtin" else LR.SEQS[1:2])
    want = [LR.pf(which, s) if which == "builtin" else LR.scaled_pf(which, s) for s in seqs]
    mfe = [LR.fold(which, s)[0][0] for s in seqs]
    got = mccaskill.pf_batch_raw(seqs)
    worst = pf_errors(seqs, got, want, KT, mfe)
    shares = [(len(s), round(far_share(P, 128), 3), round(far_share(P, 192), 3)) for s, (_, P) in zip(seqs, want) if len(s) > 128]
    print(f"\n{which}: largest error of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of the MFE share {worst[2]:.3g} (relative); "
          f"(nt, share of P on pairs with j - i >= 128, >= 192): {shares}")
    assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= F_TOL
    assert max(x[1] for x in shares) > 0.1                                         # the far pairs carry weight
    if which == "builtin":
        assert got[2][-1][0, len(LR.FAR_BRANCH) - 1] > 0.9                         # the multiloop with the 202-nt last branch
    else:
        assert mfe[-1] < -45000                                                    # exp(450 / kT) is far above the fp64 range


def test_gpu_pf_at_25_degrees_through_every_round(sets):
    install(sets, "synthetic")
    seqs = LR.SHORT + LR.SEQS[1:2]
    kt = PF.kt_of(25.0)
    want = [LR.pf("synthetic", s, 25.0) for s in seqs]
    mfe = [LR.fold("synthetic", s, temp=25.0)[0][0] for s in seqs]
    got = mccaskill.pf_batch_raw(seqs, temp=25.0)
    worst = pf_errors(seqs, got, want, kt, mfe)
    print(f"\n25 C: largest error of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of the MFE share {worst[2]:.3g} (relative)")
    assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= F_TOL
    at37 = mccaskill.pf_batch_raw(seqs, probs=False)
    assert abs(at37[1][-1]["energy"] - got[1][-1]["energy"]) > 1e5 * E_TOL         # kT and every table moved


# ---- 2. the minimum, its rows

@pytest.mark.parametrize("which", ["builtin", "tie0", "tie1"])
def test_gpu_mfe_rows_are_the_mirrors_through_every_ballot_round(sets, which):
    """routed - 133 and 146 nt in LDS, the others in device memory - and everything in device memory.  Under the flat tables the two
    candidate orders give different rows on every sequence (tests/test_lane_rounds.py), the two candidates lying in one ballot
    round, the third or the fourth"""
    install(sets, which)
    seqs = LR.SEQS if which == "builtin" else LR.stretched_tie_sequences()
    lc = N.lib().rafft_mfe_lds_len()
    assert sum(len(s) <= lc for s in seqs) >= 1 and sum(len(s) > lc for s in seqs) >= 2 and min(map(len, seqs)) > 128
    want = [LR.fold(which, s)[0] for s in seqs]
    routed = zuker.mfe_batch_raw(seqs)
    forced = zuker.mfe_batch_raw(seqs, max_lds_len=4)
    assert routed == forced
    wrong = [(s, r, w[1]) for s, r, w in zip(seqs, routed[0], want) if r != w[1]]
    assert not wrong, (which, len(wrong), wrong[:2])
    assert routed[1] == [w[0] for w in want] and routed[2] == [w[1].count("(") for w in want]
    check_rows(seqs, routed)


def test_gpu_constrained_mfe_equals_the_mirror_through_every_round():
    cases = LR.con_cases()
    want = [LR.con_fold(c) for c in cases]
    lc = N.lib().rafft_mfe_lds_len()
    assert [len(c[0]) <= lc for c in cases] == [True, False]                        # both classes in the routed call
    raw = run_constrained(cases)
    rows, dcal, n_pairs, ps, status = raw
    assert status == [0, 0]
    for k, ((d, row), pseudo, off) in enumerate(want):
        assert (dcal[k], rows[k], ps[k]) == (d, row, pseudo) and pseudo != 0, (k, rows[k], row)
    check_constrained_rows(cases, raw)
    assert raw == run_constrained(cases, max_lds_len=4)
    assert max(max(w[2].values()) for w in want) >= 128


# ---- 3. the band

def test_gpu_subopt_band_is_the_walks_through_every_round():
    seqs, delta = LR.SEQS, 60
    want = [LR.band("builtin", s, delta) for s in seqs]
    recs, rows, dcal = wuchty.subopt_batch_raw(seqs, delta)
    assert not any(r["status"] for r in recs)
    for k, s in enumerate(seqs):
        got = pairs_of(rows, dcal, k)
        assert len(got) == len(want[k]) == recs[k]["n_structs"] and set(got) == set(want[k]), len(s)
    assert evaluate_back(seqs, rows, dcal) == sum(map(len, want))
    print(f"\nstructures within {delta} dcal:", [len(w) for w in want])


# ---- 4. samples

def test_gpu_sample_pair_counts_equal_the_mirrors_probabilities():
    """5000 draws of the 197- and the 261-nt sequence against the MIRROR's P: tests/_sample_stats.py lets a correct sampler fail one
    comparison with probability <= 1e-9; 2 x 261^2 / 2 comparisons: below 1e-4 for the test"""
    seqs, n = LR.SEQS[1:3], 5000
    recs, rows, dcal = mccaskill.sample_batch_raw(seqs, n, seeds=197)
    flat_s, flat_r, flat_d = [], [], []
    for k, s in enumerate(seqs):
        e, P = LR.pf("builtin", s)
        assert recs[k]["status"] == 0 and recs[k]["n_samples"] == n and rows[k].shape == (n, len(s) + 1)
        assert abs(recs[k]["energy"] - e) <= E_TOL and recs[k]["mfe_dcal"] == LR.fold("builtin", s)[0][0]
        texts, counts, first, inv = distinct(rows[k])
        assert all(loops_ok(s, t) for t in texts)
        assert np.array_equal(dcal[k], dcal[k][first][inv]) and dcal[k].min() >= recs[k]["mfe_dcal"]
        flat_s += [s] * len(texts); flat_r += texts; flat_d += [int(dcal[k][f]) for f in first]
        XP = pair_counts(texts, counts, len(s))
        bad = ST.misses(XP, n, P)
        assert len(bad) == 0, (len(s), [(divmod(int(b), len(s)), XP.ravel()[b], n * P.ravel()[b]) for b in bad[:5]])
        far = np.triu(XP, 128).sum() / XP.sum()
        print(f"\n{len(s)} nt: {len(texts)} distinct structures in {n} draws, {far:.3f} of the drawn pairs have j - i >= 128, "
              f"the largest deviation is {float((np.abs(XP - n * P) / ST.allowed(n, P)).max()):.3f} of what the check allows")
        assert far > 0.1
    got, st = R.eval_structures(flat_s, flat_r)                                    # every sampled energy, one call
    assert not any(st) and list(got) == flat_d


# ---- 5. MEA's input

def test_gpu_mea_has_the_bits_of_pf_through_every_round():
    seqs = LR.SEQS
    mea = mccaskill.mea_batch_raw(seqs)
    pf_rows, pf_recs, pf_probs = mccaskill.pf_batch_raw(seqs)
    for k in range(len(seqs)):
        assert mea[1][k]["status"] == 0 == pf_recs[k]["status"] and mea[1][k]["mfe_dcal"] == pf_recs[k]["mfe_dcal"]
        assert np.float64(mea[1][k]["energy"]).tobytes() == np.float64(pf_recs[k]["energy"]).tobytes()
        assert mea[2][k].tobytes() == pf_probs[k].tobytes()


# ---- 6. under a span wider than two rounds

@pytest.mark.parametrize("k, span", [(1, 130), (2, 200)])
def test_gpu_span_drivers_equal_their_mirrors_on_bands_wider_than_two_rounds(k, span):
    """197 nt at span 130: the band has anti-diagonals beyond 128, its sums up to 126 candidates - two rounds filled to the last
    lanes.  261 nt at span 200: splits of up to 189 candidates, exterior windows of 196 that start above 0 - a third and a fourth
    round"""
    seqs = [LR.SHORT[0], LR.SEQS[k]]
    mir = [LR.span_pf("builtin", s, span) for s in seqs]
    got = mccaskill.pf_span_batch_raw(seqs, span)
    worst = against_mirror(seqs, got, mir, KT)
    print(f"\n{len(seqs[1])} nt, span {span}: largest error of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of unpaired {worst[2]:.3g}")
    assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= P_TOL
    assert got[2][1].shape == (len(seqs[1]), span)
    want = [LR.span_fold("builtin", s, span) for s in seqs]
    raw = zuker.mfe_span_batch_raw(seqs, span)
    assert triples(raw) == [(w[1], w[0], w[1].count("(")) for w in want]
    check_span_rows(seqs, raw, span)
    assert [r["mfe_dcal"] for r in got[1]] == raw[1]
    # the span binds: structures are lost, and pairs the free ensemble holds are beyond it
    assert raw[1][1] > LR.fold("builtin", seqs[1])[0][0]
    assert float(np.triu(LR.pf("builtin", seqs[1])[1], span).max()) > P_TOL
    assert float(np.triu(mir[1][1], 128).max()) > 1e3 * P_TOL                      # and pairs with j - i >= 128 carry weight under it
    if span == 200:
        assert max(j - i + 1 for i, j in PF.pairs_of(want[1][1])) > 128 and float(np.triu(mir[1][1], 128).max()) > 0.9
