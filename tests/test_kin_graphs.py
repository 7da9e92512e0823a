"""The kinetics host mirror (rafft_kin.get_transition_mat) and the master-equation solvers on the constructed graphs of
tests/_kin_graphs.py, on the CPU: the mirror against the independent restatement of the reference, the solvers against
closed forms."""
import os

import numpy as np
import pytest

import _kin_graphs as K
from rafft_amd import rafft_kin
from conftest import GOLD

CASES = K.well_formed_cases()
SOLVER = K.solver_cases()


def host_rate(graph, kt):
    sl, index = rafft_kin.unique_structures(graph)
    sm = {st.str_struct: (index[st.str_struct], st.energy) for st in sl}
    with np.errstate(over="ignore"):              # exp overflows to inf before min(1, .), as in the reference
        mat = rafft_kin.get_transition_mat(graph, len(sl), sm, kt)
    return np.asarray(mat, dtype=np.float64), sl


def check_mirror(graph, kt):
    want = K.reference_rate_matrix(graph, kt)
    got, sl = host_rate(graph, kt)
    assert [s.str_struct for s in sl] == [s.str_struct for s in K.unique_rows(graph)[0]]
    assert np.array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    return want


def test_builders_are_deterministic_and_complete():
    again = K.well_formed_cases()
    assert [(n, kt, [[(r.str_struct, r.energy) for r in st] for st in g]) for n, g, kt in CASES] == \
           [(n, kt, [[(r.str_struct, r.energy) for r in st] for st in g]) for n, g, kt in again]
    assert [[(r.str_struct, r.energy) for st in g for r in st] for _, g in K.malformed_graphs()] == \
           [[(r.str_struct, r.energy) for st in g for r in st] for _, g in K.malformed_graphs()]
    names = [n for n, _, _ in CASES]
    assert len(set(names)) == len(names)
    for fam in K.FAMILIES:
        assert any(n.startswith(fam + "/") for n in names), fam
    assert [n for n in names if n.startswith("length_edges/")] == [f"length_edges/L{L}" for L in K.LENGTH_EDGES]
    assert [n for n in names if n.startswith("stars/")] == [f"stars/S{S}" for S in K.STAR_SIZES]
    assert len(K.malformed_graphs()) == 12
    by = {n: g for n, g, _ in CASES}
    for L in K.LENGTH_EDGES:
        g = by[f"length_edges/L{L}"]
        assert all(len(r.str_struct) == L for st in g for r in st)
        if L >= 63:
            assert [len(st) for st in g][:2] == [1, 5]
            m = K.reference_rate_matrix(g)
            S = m.shape[0]
            # step 2 holds rows with a parent and rows without one
            kids = [np.count_nonzero(m[k, 1:6]) for k in range(6, S)]
            assert 0 in kids and max(kids) >= 1, (L, kids)
    assert sum(len(st) for st in by["length_edges/L32767"]) == 12
    for S in K.STAR_SIZES:
        assert K.reference_rate_matrix(by[f"stars/S{S}"]).shape == (S, S)
    assert [len(st) for st in by["step_shapes/facing"]] == list(K.FACING_SIZES)
    assert [len(st) for st in by["step_shapes/empty_steps"]] == [1, 1, 0, 1, 0]


def test_reference_on_hand_checked_graphs():
    """the restatement itself, on matrices small enough to write down"""
    L = 6
    a, ab = K.db_of(L, [(0, 5)]), K.db_of(L, [(0, 5), (1, 4)])
    m = K.reference_rate_matrix([[K.Row(a, -1.0), K.Row(ab, -2.0)]], 0.5)         # one step: compared with itself
    x = float(np.exp(np.longdouble(-2.0)))
    np.testing.assert_allclose(m, [[-1.0, 1.0], [x, -x]], rtol=2e-16)
    g = K.energy_chain()
    m = K.reference_rate_matrix(g, 0.61)
    e = [r.energy for st in g for r in st]
    assert e[:4] == [0.0, 0.0, 0.1, 0.0]
    assert m[0, 1] == 1.0 and m[1, 0] == 1.0                                        # dE = 0: both rates exactly 1
    k440 = e.index(440.0)
    assert 0 < m[k440 - 1, k440] < 2.3e-308 and m[k440, k440 - 1] == 1.0           # exp(-721.3): a subnormal; exp(+721.3) = inf -> 1
    k460 = e.index(460.0)
    assert m[k460 - 1, k460] == 0.0 and m[k460, k460 - 1] == 1.0                   # exp(-754.1) = 0: a one-way edge
    assert m[k460, k460 + 1] == 1.0 and m[k460 + 1, k460] == 0.0
    assert K.metropolis(-745.2) == 0.0 and K.metropolis(-744.0) == 1e-323 and K.metropolis(710.0) == 1.0
    assert K.metropolis(-1.0) == float(np.exp(np.longdouble(-1.0)))
    # the last step holds a subset of a step-0 row: the negative index connects them
    m = K.reference_rate_matrix([[K.Row(ab, -2.0)], [K.Row("......", 0.0)], [K.Row(a, -1.0)]], 0.61)
    assert m[0, 2] != 0 and m[2, 0] == 1.0 and m[1, 2] == 1.0 and m[0, 1] == 0.0


@pytest.mark.parametrize("name", [n for n, _, _ in CASES])
def test_host_mirror_equals_reference(name):
    _, graph, kt = next(c for c in CASES if c[0] == name)
    check_mirror(graph, kt)


@pytest.mark.parametrize("name", ["example_rafft_20.out", "example_rafft.out"])
def test_host_mirror_equals_reference_on_examples(name):
    graph = K.parse_graph_text(os.path.join(GOLD, name))
    want = check_mirror(graph, K.KT)
    assert want.shape[0] > 10 and np.count_nonzero(want) > 2 * want.shape[0]


def test_graph_arrays_refuses_rows_of_different_lengths():
    g = K.two_state_graph()
    rafft_kin.graph_arrays(g)
    g[1].append(K.Row("(...)", -0.5))
    with pytest.raises(ValueError, match="one length"):
        rafft_kin.graph_arrays(g)
    with pytest.raises(ValueError, match="one length"):
        rafft_kin.graph_arrays([[K.Row("...", 0.0)], [K.Row("(..)", -1.0)]])


# ---------------------------------------------------------------- the solvers against closed forms

def cpu_solver(name):
    import torch
    graph, kt, times, exact, spectral_ok = SOLVER[name]
    rate, sl = host_rate(graph, kt)
    energy = np.array([s.energy for s in sl])
    p0 = torch.zeros(len(sl), dtype=torch.float64)
    p0[0] = 1.0

    def solve(method, substeps=32, kt_solver=kt):
        return rafft_kin.solve_master_equation(torch.as_tensor(rate), energy, p0, times, method, substeps, kt=kt_solver)
    return solve, energy, kt, exact


def check_second_order(solve, exact, method, m=4):
    """TR-BDF2 is a second-order scheme: twice the steps, a quarter of the error (asserted as between 1/5 and 1/3).  At
    m = 4 the steps are 1/5 of each time interval of e^0.356, i.e. h = 0.06 t: the error is ~1e-5, ten orders above the
    rounding of a well-conditioned 2 x 2 or star solve."""
    a, b = solve(method, m), solve(method, 2 * m)
    for P in (a, b):
        assert P.min() > -1e-9 and np.allclose(P.sum(axis=1), 1.0)
    ea, eb = np.abs(a - exact).max(), np.abs(b - exact).max()
    print(f"{method}: error {ea:.3e} at substeps {m}, {eb:.3e} at {2 * m}, ratio {eb / ea:.4f}")
    assert ea > 1e-8 and eb > 1e-8
    assert 1 / 5 < eb / ea < 1 / 3


@pytest.mark.parametrize("name", ["two_state", "two_state_kt0.2", "two_state_kt5", "star"])
def test_spectral_solver_against_closed_form(name):
    solve, energy, kt, exact = cpu_solver(name)
    P = solve("spectral")
    err = np.abs(P - exact).max()
    print(f"{name}: spectral error {err:.3e}, bound {K.spectral_bound(energy, kt):.3e}")
    assert err < K.spectral_bound(energy, kt)
    assert np.array_equal(solve("auto"), P)                  # a span below 30 kT: auto is the spectral formula


def test_spectral_solver_needs_the_kt_of_the_rate_matrix():
    """kt reaches the symmetrisation: with the rate matrix of kt 0.2 and the module's 0.61 in the solver the populations are off"""
    solve, energy, kt, exact = cpu_solver("two_state_kt0.2")
    assert np.abs(solve("spectral", kt_solver=0.61) - exact).max() > 1e-3
    assert np.abs(solve("spectral") - exact).max() < K.spectral_bound(energy, kt)


@pytest.mark.parametrize("name", ["two_state", "star", "underflow"])
def test_implicit_solver_is_second_order(name):
    solve, energy, kt, exact = cpu_solver(name)
    check_second_order(solve, exact, "implicit")             # two rows: dense LU; the star: sparse LU when SciPy is there
    check_second_order(solve, exact, "implicit-dense")


def test_auto_takes_the_integrator_on_an_absorbing_state():
    solve, energy, kt, exact = cpu_solver("underflow")
    assert (energy.max() - energy.min()) / kt > rafft_kin.SPECTRAL_MAX_SPAN_KT
    P = solve("auto")
    assert np.isfinite(P).all() and P.min() >= -1e-9 and np.allclose(P.sum(axis=1), 1.0)
    assert np.array_equal(P, solve("implicit"))
    assert np.abs(P - exact).max() < 1e-3 and P[-1, 1] > 1 - 1e-9      # 1 - exp(-t): everything ends in the folded row
