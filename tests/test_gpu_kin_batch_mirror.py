"""kin_batch_integrate_kernel against an extended-precision mirror of its own scheme (tests/_kin_mirror.py), on real folding graphs
of both size classes (M^-1 in LDS up to 128 states, in device memory above), at the exact sizes where the code changes its path,
on the scheme's closed form and on schedules the wrappers never produce.

tests/test_gpu_kin_batch.py compares the populations with the differential equation and so has to tolerate the scheme's truncation
error (5e-6 .. 2e-2).  Here the mirror integrates the device's OWN matrix (rates=True; that matrix is held to
_kin_graphs.reference_rate_matrix in the same test) on the same schedule, so only rounding is left.  On real graphs at late times
I - c h A has a condition number near 1e10 and rounding alone is 1e-8 .. 1e-7 for any fp64 implementation; the bound per output time
is therefore FACTOR times the distance of a plain fp64 LU run of the scheme from the extended one (_kin_mirror.bound), never a
constant and never anything taken from the device's output.

FACTOR: measured against delta, which comes from the mirrors alone.  The first MI355X run had FACTOR = 100 (the habit of
tests/test_gpu_landscape.py) and printed the device/delta ratios below; FACTOR is ten times the largest of them, rounded up to a power
of ten: 10 * 15.09 -> 1000.  No ratio came near 100, the mark above which the kernel would be doing something its numpy restatement
(_kin_mirror.restated_f64) does not: the restatement's ratios on the same inputs are given beside the device's.

Measured on an MI355X, |device - mirror_ext| (largest over the graph's populations):
  graph, schedule                      states   delta     first 60 % of times   all times   device/delta   restated/delta
  traj3, 30/12/4                          104   3.4e-09   1.3e-13               1.5e-08      4.54            4.88
  traj11                                  203   6.9e-11   4.0e-14               7.7e-11      1.63            1.70
  traj34                                  262   1.6e-08   3.6e-14               1.9e-08      2.02            2.08
  long4                                   130   1.3e-14   5.8e-15               1.7e-14      0.40            0.45
  long5                                   136   3.9e-15   4.2e-15               7.0e-15      0.43            0.43
  ties13                                  392   6.0e-09   6.6e-14               8.5e-09      3.99            5.04
  example_rafft_20.out                     68   1.4e-08   8.4e-14               6.9e-08      5.01            4.26
  ties14, 30/6/2                          815   1.5e-10   1.2e-15               1.2e-10      5.24            4.21
  traj34[:S], S = 1 .. 130, 30/8/2     1..130   <= 7e-15  <= 2.6e-15            <= 9.3e-15   <= 1.12         <= 1.12
  traj34[:257], 30/8/2                    257   4.6e-09   2.5e-15               4.8e-09      1.43            1.42
  two-state, solver_times, 4                2   7.3e-16   3.1e-16               4.0e-16      0.07            0.07
  star, solver_times, 4                   257   2.3e-15   2.6e-14               2.6e-14      5.99            5.93
  traj3, one step of 1e9                  104   1.0e-07   1.5e-06               1.5e-06     15.09           10.13
  traj3, 200 times with m = 1             104   2.7e-09   3.3e-13               8.8e-09     11.68           15.04
  traj3, m = 1, 7, 1, 7 ..                104   6.7e-09   1.5e-13               6.2e-09      2.23            2.34
Column 0 against the scheme's closed form: 4.0e-16 (two-state), 2.6e-14 (star).  restated/delta is restated_f64 in
the device's place on _kin_graphs.reference_rate_matrix of the same graph and schedule, a host run.  The ratios above 10 are a property of the
unpivoted Gauss-Jordan inverse followed by products with it, which the restatement shows as well; the pivoted LU is the yardstick."""
import numpy as np
import pytest

import _kin_graphs as K
import _kin_mirror as KM
from rafft_amd import _native as N
from rafft_amd import rafft_kin

pytestmark = pytest.mark.gpu

FACTOR = 1000

SCHED = rafft_kin.kinetics_schedule(30, 12, 4)              # 378 sub-steps, times out to e^23.5 where the stage matrix is stiff
REAL = ["traj3", "traj11", "traj34", "long4", "long5", "ties13", "example_rafft_20.out"]
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 130, 257)
_cache = {}


def graph_of(name):
    return KM.example_graph(name) if name.endswith(".out") else KM.golden_graphs()[name]


def call(graphs, schedule, **kw):
    times, ms, hs = schedule
    return rafft_kin.kin_batch_call([rafft_kin._batch_graph(g)[:5] for g in graphs], times, K.KT, rates=True, schedule=(times, list(ms), list(hs)), **kw)


def real_batch():
    if "real" not in _cache:
        _cache["real"] = call([graph_of(n) for n in REAL], SCHED)
    return _cache["real"]


def yardstick(key, rate, schedule):
    """(mirror_ext, delta per output time) of the device's matrix on the schedule, once per key"""
    if key not in _cache:
        _, ms, hs = schedule
        ext, res = KM.mirror_ext(rate.T, ms, hs)
        assert res < KM.residual_limit(len(rate)), (key, res)
        ext.setflags(write=False)
        _cache[key] = (ext, KM.row_error(KM.mirror_f64(rate.T, ms, hs), ext))
    return _cache[key]


def check_rate(key, graph, got):
    if ("rate", key) not in _cache:
        _cache["rate", key] = K.reference_rate_matrix(graph, K.KT)
    want = _cache["rate", key]
    assert got.shape == want.shape and np.array_equal(got != 0, want != 0), key
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=str(key))


def check(key, graph, res, k, schedule, column0=None):
    """graph k of `res`: its matrix against the reference, every population within the bound of the mirror (and column 0 within
    the bound of `column0`, a closed form); prints the figures first, returns the largest device/delta ratio"""
    assert res["status"][k] == N.OK, res["error"]
    rate, P = res["rate"][k], res["pop"][k]
    check_rate(key[0], graph, rate)
    ext, delta = yardstick(key, rate, schedule)
    ms = schedule[1]
    err = KM.row_error(P, ext)
    unit = KM.bound(delta, ms, 1)
    early = max(1, int(0.6 * len(ms)))
    worst = float((err / unit).max())
    print(f"{key[0]}: {len(rate)} states, delta {float(delta.max()):.3e}, device - mirror {float(err[:early].max()):.3e} over the first 60 % "
          f"of the times, {float(err.max()):.3e} over all, device/delta at most {worst:.2f}")
    assert P.shape == ext.shape and np.isfinite(P).all()
    assert (err <= FACTOR * unit).all(), key
    if column0 is not None:
        e0 = np.abs(P[:, 0] - column0)
        print(f"{key[0]}: column 0 against the scheme's closed form {float(e0.max()):.3e}, over delta at most {float((e0 / unit).max()):.2f}")
        assert (e0 <= FACTOR * unit).all(), key
    return worst


# ---------------------------------------------------------------- 1. real graphs, both classes, one batch

def test_gpu_real_graphs_of_both_classes_in_one_batch():
    res = real_batch()
    sizes = res["n_unique"]
    assert sizes == [len(K.unique_rows(graph_of(n))[0]) for n in REAL]
    assert sum(s > 128 for s in sizes) >= 3 and sum(65 <= s <= 128 for s in sizes) >= 2
    for k, name in enumerate(REAL):
        check((name, "sched"), graph_of(name), res, k, SCHED)


# ---------------------------------------------------------------- 2. the large graph and the one over the cap

def test_gpu_815_states_alone_and_beside_a_graph_over_the_cap():
    sched = rafft_kin.kinetics_schedule(30, 6, 2)
    big, over = KM.golden_graphs()["ties14"], KM.golden_graphs()["ms50_0"]
    alone = call([big], sched)
    assert alone["n_unique"] == [815]
    check(("ties14", "30/6/2"), big, alone, 0, sched)
    both = call([over, big], sched)
    assert both["status"] == [N.ERR_CAPACITY, N.OK] and both["n_unique"] == [1056, 815]
    assert "graph 0" in both["error"] and both["pop"][0] is None
    assert np.array_equal(both["pop"][1], alone["pop"][0]) and np.array_equal(both["rate"][1], alone["rate"][0])
    assert np.array_equal(both["uid"][1], alone["uid"][0])


# ---------------------------------------------------------------- 3. exact sizes

def test_gpu_exact_sizes_around_the_lane_rounds_and_the_lds_switch():
    """prefixes of ONE parent with exactly S unique structures: one and two lane rounds of a row (64 / 65), the last size with
    M^-1 in LDS and the first without (128 / 129: one state apart), 1 and 2"""
    sched = rafft_kin.kinetics_schedule(30, 8, 2)
    parent = KM.golden_graphs()["traj34"]
    graphs = [KM.truncated(parent, S) for S in SIZES]
    res = call(graphs, sched)
    assert res["n_unique"] == list(SIZES)
    for k, S in enumerate(SIZES):
        check((f"traj34[:{S}]", "30/8/2"), graphs[k], res, k, sched)
    assert np.array_equal(res["pop"][0], np.ones((len(sched[0]), 1)))
    a, b = (res["uid"][SIZES.index(S)] for S in (128, 129))                          # one row, one state and the class apart
    assert len(b) == len(a) + 1 and np.array_equal(b[:-1], a) and b[-1] == 128


# ---------------------------------------------------------------- 4. the closed form of the scheme

def test_gpu_two_state_and_star_against_the_closed_form_of_the_scheme():
    sched = rafft_kin.kinetics_schedule(sample_times=K.solver_times(-9.0), substeps=4)
    graphs = [K.two_state_graph(-1.0), K.star_graph(K.SOLVER_STAR_LEAVES + 1, K.SOLVER_STAR_ENERGY)]
    res = call(graphs, sched)
    assert res["status"] == [N.OK] * 2 and res["n_unique"] == [2, K.SOLVER_STAR_LEAVES + 1]
    for k, (name, mode) in enumerate((("two_state", KM.two_state_mode), ("star257", KM.star_mode))):
        lam, p_eq0 = mode(res["rate"][k])
        check((name, "solver_times"), graphs[k], res, k, sched, column0=KM.scheme_closed_form(lam, p_eq0, sched[1], sched[2]))


# ---------------------------------------------------------------- 5. schedules the wrappers never produce

def edge_schedules():
    t12 = SCHED[0]
    t200 = np.exp(np.linspace(-4.0, 23.5, 200))
    alt = [1 if k % 2 == 0 else 7 for k in range(len(t12))]
    return {"one_step_of_1e9": (np.array([1e9]), [1], [1e9]),
            "200_times_m_1": (t200, [1] * 200, np.diff(t200, prepend=0.0).tolist()),
            "m_alternating_1_7": (t12, alt, (np.diff(t12, prepend=0.0) / np.array(alt)).tolist())}


@pytest.mark.parametrize("which", list(edge_schedules()))
def test_gpu_schedule_edges(which):
    """one enormous L-stable step; 200 intervals of one sub-step, M^-1 rebuilt 200 times; sub-step counts 1, 7, 1, 7 .. with unequal
    steps - each against the mirror run on that same schedule"""
    sched = edge_schedules()[which]
    graph = KM.golden_graphs()["traj3"]
    check(("traj3", which), graph, call([graph], sched), 0, sched)


# ---------------------------------------------------------------- 6. chunking

def test_gpu_real_graphs_chunked_one_by_one_give_the_same_bits():
    whole = real_batch()
    chunked = call([graph_of(n) for n in REAL], SCHED, workspace_bytes=1)
    assert chunked["status"] == whole["status"] == [N.OK] * len(REAL)
    for k, name in enumerate(REAL):
        assert np.array_equal(chunked["pop"][k], whole["pop"][k]), name
        assert np.array_equal(chunked["rate"][k], whole["rate"][k]) and chunked["n_edges"][k] == whole["n_edges"][k], name
        assert np.array_equal(chunked["uid"][k], whole["uid"][k]) and np.array_equal(chunked["first_row"][k], whole["first_row"][k]), name
