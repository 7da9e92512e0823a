"""The inputs of tests/test_gpu_lane_rounds.py tell a 64-candidate loop that stops after its second or third round from the right
one (tests/_lane_rounds.py; mirrors only, no GPU):
* each of the seven sums of the partition function, cut after two and after three rounds, moves the ensemble energy or a pair
  probability of a sequence of `SEQS` by a thousand times the bound the GPU tests hold the device to, or more;
* the stretched tie sequences have two co-optimal rows that the candidate order separates, and their folds in the documented
  order take an exterior stem and a multiloop split in the third and in the fourth ballot round;
* the energy band of the subopt test is neither one structure nor thousands, and the drawn constraints leave a structure.
Measured (kcal/mol and probabilities; the bounds are 1e-5 and 1e-6):
    C split        2 rounds: 197 nt dE 0.079         3 rounds: 261 nt dE 0.080
    M split        2 rounds: 197 nt dE 0.0096        3 rounds: 261 nt dE 0.077
    exterior F     2 rounds: 197 nt dE 0.10          3 rounds: 261 nt dE 1.3
    Mo over Co     2 rounds: 197 nt dP 0.10          3 rounds: 261 nt dP 3.4e-8 - not enough; FAR_BRANCH dP 0.999
    Mo over Mo     2 rounds: 197 nt dP 3.8e-3        3 rounds: 261 nt dP 3.0e-6
    M1o over Mo    2 rounds: 197 nt dP 1.4e-3        3 rounds: 261 nt dP 7.5e-4
    M1o over Co    2 rounds: 197 nt dP 3.2e-4        3 rounds: 261 nt dP 2.1e-3
"""
import math

import numpy as np
import pytest

import oracle
from rafft_amd import params
import _lane_rounds as LR
import _pf_np as PF
from test_gpu_pf import E_TOL, P_TOL

KT = PF.kt_of(37.0)


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def test_the_sequences_are_what_the_rounds_need():
    assert [len(s) for s in LR.SEQS] == [133, 197, 261, 228] and [len(s) for s in LR.SHORT] == [9, 64]
    assert [len(s) for s in LR.stretched_tie_sequences()] == [146, 210, 170, 234]
    # a C split of (i,j) has j - i - 10 candidates: 133 nt stay within two rounds, 197 within three, 228 and 261 take a fourth
    assert 133 - 11 <= 128 < 197 - 11 <= 192 < 228 - 11 < 261 - 11 <= 256


def test_scaled_mirror_is_the_mirror():
    """at scale 1 the same bits; under the scale of the minimum the same sums in another rounding - a thousandth of the bounds the
    device is held to"""
    s = LR.SEQS[0]
    m, (Z, P) = LR.base_mirror("builtin", s)
    lnz, P1 = LR.ScaledPfMirror(LR.tables("builtin")).run(s)
    assert lnz == math.log(Z) and P1.tobytes() == P.tobytes()
    e, P2 = LR.scaled_pf("builtin", s)
    d_e, d_p = abs(e - m.energy(Z)), float(np.abs(P2 - P).max())
    print(f"\n133 nt, scaled against unscaled: energy {d_e:.3g} kcal/mol, P {d_p:.3g}")
    assert d_e <= 1e-3 * E_TOL and d_p <= 1e-3 * P_TOL
    for x in LR.SHORT:                                        # 9 and 64 nt under the tables the scaled form is there for
        (e0, P0), (e1, P1) = LR.pf("multiloops_win", x), LR.scaled_pf("multiloops_win", x)
        assert abs(e1 - e0) <= 1e-3 * E_TOL and float(np.abs(P1 - P0).max()) <= 1e-3 * P_TOL and e0 < 0.0
    # and the cut is a cut: one round of the C split kept at 133 nt
    cut = LR.RoundsMirror(LR.tables("builtin"), "C split", 1)
    assert abs(KT * (cut.run(s, m)[0] - math.log(Z))) > 1e3 * E_TOL and cut.n_cut > 0


@pytest.mark.parametrize("rounds_kept", [2, 3])
@pytest.mark.parametrize("which", LR.LOOPS)
def test_a_sum_that_stops_early_moves_the_result(which, rounds_kept):
    """the sequences in turn, shortest first, until one discriminates: the energy for an inside sum (Z moves), a probability for an
    outside sum (Z does not)"""
    seen = []
    for s in LR.SEQS[1:] if rounds_kept == 2 else LR.SEQS[2:]:
        m, (Z, P) = LR.base_mirror("builtin", s)
        cut = LR.RoundsMirror(LR.tables("builtin"), which, rounds_kept)
        if which in LR.INSIDE_LOOPS:
            d_e, d_p = abs(KT * math.log(cut.inside(s, m, cut.n_kept if which != "exterior F" else len(s)) / Z)), 0.0
        else:
            lnz, P2 = cut.run(s, m)
            assert lnz == math.log(Z)
            d_e, d_p = 0.0, float(np.abs(P2 - P).max())
        assert cut.n_cut > 0
        seen.append((len(s), d_e, d_p))
        if d_e >= 1e3 * E_TOL or d_p >= 1e3 * P_TOL:
            break
    print(f"\n{which}, {rounds_kept} rounds kept: (nt, dE, dP) {seen}")
    assert seen[-1][1] >= 1e3 * E_TOL or seen[-1][2] >= 1e3 * P_TOL, seen


@pytest.mark.parametrize("which", ["tie0", "tie1"])
def test_stretched_tie_sequences_reach_the_third_and_fourth_ballot_round(which):
    oracle.set_tables(LR.tables(which))
    far_f, far_split = [], []
    for s in LR.stretched_tie_sequences():
        (d, first), off = LR.fold(which, s)
        (d2, last), off2 = LR.fold(which, s, "last")
        assert oracle.eval_structure(s, first) == d == d2 == oracle.eval_structure(s, last), (which, s)
        assert first != last, (which, s)                      # two rows of the minimum: the order decides
        print(f"\n{which} {len(s)} nt: offsets in the documented order {off}, in the reversed order {off2}")
        far_f.append(off["F"])
        far_split.append(max(off["M"], off["C"]))
    far_f.sort()
    far_split.sort()
    assert far_f[-2] >= 128 and far_f[-1] >= 192, far_f       # an exterior stem in the third round, another in the fourth
    assert far_split[-2] >= 128 and far_split[-1] >= 192, far_split


def test_the_band_and_the_constraints_leave_something_to_compare():
    sizes = [len(LR.band("builtin", s, 60)) for s in LR.SEQS]
    print("\nstructures within 60 dcal:", sizes)
    assert all(2 <= n <= 500 for n in sizes)
    far = []
    for case in LR.con_cases():
        (d, row), pseudo, off = LR.con_fold(case)
        assert d is not None and pseudo != 0 and set(case[1]) - set(".")
        far.append(max(off.values()))
    assert max(far) >= 128                                    # a candidate of the third round decides a constrained cell
