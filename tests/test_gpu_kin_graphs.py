"""The kinetics kernels (kin_pair_table_kernel, kin_rates_kernel, kin_diag_kernel behind rafft_kin_rate_matrix) on the
constructed graphs of tests/_kin_graphs.py against the independent restatement of the reference, the entry point's error
returns, and the device solvers against closed forms."""
import ctypes as C

import numpy as np
import pytest

import _kin_graphs as K
from rafft_amd import _native as N
from rafft_amd import rafft_kin

pytestmark = pytest.mark.gpu

CASES = {name: (graph, kt) for name, graph, kt in K.well_formed_cases()}
MALFORMED = dict(K.malformed_graphs())
SOLVER = K.solver_cases()
_reference = {}


def reference(name):
    """(restatement of the reference, host mirror, structures) of a case, computed once"""
    if name not in _reference:
        graph, kt = CASES[name]
        sl, index = rafft_kin.unique_structures(graph)
        sm = {st.str_struct: (index[st.str_struct], st.energy) for st in sl}
        with np.errstate(over="ignore"):
            mirror = np.asarray(rafft_kin.get_transition_mat(graph, len(sl), sm, kt), dtype=np.float64)
        want = K.reference_rate_matrix(graph, kt)
        want.setflags(write=False)
        mirror.setflags(write=False)
        _reference[name] = (want, mirror, [s.str_struct for s in K.unique_rows(graph)[0]])
    return _reference[name]


def check_exact(name):
    graph, kt = CASES[name]
    want, mirror, structs = reference(name)
    got, sl, en = rafft_kin.rate_matrix_gpu(graph, kt)
    got = got.cpu().numpy()
    assert [s.str_struct for s in sl] == structs
    for ref in (want, mirror):
        assert np.array_equal(got != 0, ref != 0)
        np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_rate_matrix_equals_reference(name):
    check_exact(name)


@pytest.mark.parametrize("name", list(MALFORMED))
def test_gpu_malformed_row_is_refused_and_the_next_call_is_exact(name):
    with pytest.raises(N.RafftError) as err:
        rafft_kin.rate_matrix_gpu(MALFORMED[name])
    assert err.value.code == N.ERR_STRUCT
    check_exact("length_edges/L66")


def raw_call(graph, kt=K.KT, n_steps=None, L=None, n_unique=None, sizes=None, uid=None):
    """rafft_kin_rate_matrix through the ctypes binding with some arguments replaced -> (status, matrix)"""
    import torch
    g_sizes, rows, g_uid, energy, sl = rafft_kin.graph_arrays(graph)
    S = len(sl)
    sizes = g_sizes if sizes is None else np.asarray(sizes, dtype=np.int32)
    uid = g_uid if uid is None else np.asarray(uid, dtype=np.int32)
    assert len(sizes) == len(g_sizes) and len(uid) == len(g_uid)
    rate = torch.full((S, S), 7.0, dtype=torch.float64, device="cuda")
    rc = N.lib().rafft_kin_rate_matrix(len(sizes) if n_steps is None else n_steps, sizes.ctypes.data_as(C.POINTER(C.c_int)),
                                       len(sl[0].str_struct) if L is None else L, rows, uid.ctypes.data_as(C.POINTER(C.c_int)),
                                       S if n_unique is None else n_unique, energy.ctypes.data_as(C.POINTER(C.c_double)),
                                       float(kt), C.c_void_p(rate.data_ptr()))
    return rc, rate.cpu().numpy()


def bad_arguments():
    graph = CASES["length_edges/L66"][0]
    sizes, rows, uid, energy, sl = rafft_kin.graph_arrays(graph)
    neg = sizes.copy()
    neg[1] = -1
    high, low = uid.copy(), uid.copy()
    high[-1] = len(sl)
    low[3] = -1
    return {"L_0": dict(L=0), "L_32768": dict(L=32768), "n_unique_0": dict(n_unique=0), "n_steps_0": dict(n_steps=0),
            "kt_0": dict(kt=0.0), "kt_nan": dict(kt=float("nan")), "negative_step_size": dict(sizes=neg),
            "uid_n_unique": dict(uid=high), "uid_minus_1": dict(uid=low), "all_step_sizes_0": dict(sizes=np.zeros_like(sizes))}


@pytest.mark.parametrize("what", list(bad_arguments()))
def test_gpu_bad_argument_is_refused_and_the_next_call_is_exact(what):
    graph = CASES["length_edges/L66"][0]
    rc, rate = raw_call(graph, **bad_arguments()[what])
    assert rc == N.ERR_PARAM
    assert (rate == 7.0).all()                               # refused before anything was written
    rc, rate = raw_call(graph)
    want = reference("length_edges/L66")[0]
    assert rc == N.OK and np.array_equal(rate != 0, want != 0)
    np.testing.assert_allclose(rate, want, rtol=1e-13, atol=0)


# ---------------------------------------------------------------- the device solvers

def cpu_rate(graph, kt):
    sl, index = rafft_kin.unique_structures(graph)
    sm = {st.str_struct: (index[st.str_struct], st.energy) for st in sl}
    with np.errstate(over="ignore"):
        return np.asarray(rafft_kin.get_transition_mat(graph, len(sl), sm, kt), dtype=np.float64), np.array([s.energy for s in sl])


@pytest.mark.parametrize("method", ["spectral", "implicit", "implicit-dense"])
@pytest.mark.parametrize("name", ["two_state", "star", "underflow"])
def test_gpu_kinetics_equals_the_cpu_solve(name, method):
    import torch
    graph, kt, _, _, _ = SOLVER[name]
    max_time, n_steps, substeps = 10.0, 12, 8
    traj, times, sl, eq = rafft_kin.kinetics_gpu(graph, max_time, n_steps, method=method, substeps=substeps, kt=kt)
    rate, energy = cpu_rate(graph, kt)
    p0 = torch.zeros(len(energy), dtype=torch.float64)
    p0[0] = 1.0
    sample_times = np.exp(np.arange(n_steps) * (max_time / n_steps) - 4)
    want = rafft_kin.solve_master_equation(torch.as_tensor(rate), energy, p0, sample_times, method, substeps, kt=kt)
    got = np.array(traj)[1:]
    print(f"{name} {method}: device against CPU {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() < 1e-7


def device_solver(name):
    import torch
    graph, kt, times, exact, _ = SOLVER[name]
    rate, sl, energy = rafft_kin.rate_matrix_gpu(graph, kt)
    p0 = torch.zeros(len(sl), dtype=torch.float64, device=rate.device)
    p0[0] = 1.0
    return (lambda method, substeps=32: rafft_kin.solve_master_equation(rate, energy, p0, times, method, substeps, kt=kt)), energy, kt, exact


@pytest.mark.parametrize("name", ["two_state", "two_state_kt0.2", "two_state_kt5", "star"])
def test_gpu_spectral_solver_against_closed_form(name):
    solve, energy, kt, exact = device_solver(name)
    err = np.abs(solve("spectral") - exact).max()
    print(f"{name}: spectral error {err:.3e}, bound {K.spectral_bound(energy, kt):.3e}")
    assert err < K.spectral_bound(energy, kt)


@pytest.mark.parametrize("method", ["implicit", "implicit-dense"])
@pytest.mark.parametrize("name", ["two_state", "star", "underflow"])
def test_gpu_implicit_solver_is_second_order(name, method, m=4):
    """as tests/test_kin_graphs.py check_second_order: twice the steps, between 1/5 and 1/3 of the error"""
    solve, energy, kt, exact = device_solver(name)
    a, b = solve(method, m), solve(method, 2 * m)
    for P in (a, b):
        assert P.min() > -1e-9 and np.allclose(P.sum(axis=1), 1.0)
    ea, eb = np.abs(a - exact).max(), np.abs(b - exact).max()
    print(f"{name} {method}: error {ea:.3e} at substeps {m}, {eb:.3e} at {2 * m}, ratio {eb / ea:.4f}")
    assert ea > 1e-8 and eb > 1e-8
    assert 1 / 5 < eb / ea < 1 / 3


def test_gpu_auto_takes_the_integrator_on_an_absorbing_state():
    solve, energy, kt, exact = device_solver("underflow")
    P = solve("auto")
    assert np.isfinite(P).all() and P.min() >= -1e-9 and np.allclose(P.sum(axis=1), 1.0)
    assert np.array_equal(P, solve("implicit"))
