"""tests/_kin_mirror.py on the host: the extended-precision mirror of the batch kinetics scheme is right (closed form of the scheme,
second order against the 60-digit truth), its bound lets the kernel's arithmetic restated in numpy pass and fails two mutants of it
by three orders, and the mirror runs the scheme of the shipped host solver.  No GPU."""
import numpy as np
import pytest

import _kin_graphs as K
import _kin_mirror as KM
from rafft_amd import rafft_kin
from conftest import load_json_gz

_cache = {}


def host_rate(name):
    """rate matrix (fp64) of a golden graph or of an example, from the host mirror of get_transition_mat"""
    if name not in _cache:
        graph = KM.example_graph(name) if name.endswith(".out") else KM.golden_graphs()[name]
        ordered, index = K.unique_rows(graph)
        struct_map = {st.str_struct: (index[st.str_struct], st.energy) for st in ordered}
        _cache[name] = np.array(rafft_kin.get_transition_mat(graph, len(ordered), struct_map), dtype=np.float64)
        _cache[name].setflags(write=False)
    return _cache[name]


def schedule_of(name):
    return rafft_kin.kinetics_schedule(30, 20, 8) if name.endswith(".out") else rafft_kin.kinetics_schedule(30, 12, 4)


def mirrors(name):
    """(ext, f64, ms) on the graph's schedule, computed once"""
    key = ("mirrors", name)
    if key not in _cache:
        A = host_rate(name).T
        _, ms, hs = schedule_of(name)
        ext, res = KM.mirror_ext(A, ms, hs)
        assert res < KM.residual_limit(len(A)), (name, res)
        _cache[key] = (ext, KM.mirror_f64(A, ms, hs), ms, hs)
    return _cache[key]


def test_golden_graphs_and_their_prefixes():
    graphs = KM.golden_graphs()
    assert {n: len(K.unique_rows(g)[0]) for n, g in graphs.items()} == {n: s for n, (_, _, s) in KM.GOLDEN.items()}
    parent = graphs["traj34"]
    flat = [st.str_struct for step in parent for st in step]
    for S in (1, 2, 63, 64, 65, 127, 128, 129, 130, 257, 262):
        g = KM.truncated(parent, S)
        rows = [st.str_struct for step in g for st in step]
        assert len(K.unique_rows(g)[0]) == S and rows == flat[:len(rows)]
        assert all(len(a) == len(b) for a, b in zip(g[:-1], parent))                  # whole leading steps
        assert len({*rows[:-1]}) == S - 1                                                 # it stops at the row that makes S
    with pytest.raises(ValueError):
        KM.truncated(parent, 263)


@pytest.mark.parametrize("which", ["two_state", "star"])
def test_mirror_ext_equals_the_closed_form_of_the_scheme(which):
    """measured here: 0 on the two-state graph, 1.4e-20 on the 257-state star"""
    graph = K.two_state_graph(-1.0) if which == "two_state" else K.star_graph(K.SOLVER_STAR_LEAVES + 1, K.SOLVER_STAR_ENERGY)
    rate = K.reference_rate_matrix(graph, K.KT)
    times, ms, hs = rafft_kin.kinetics_schedule(sample_times=K.solver_times(-9.0), substeps=4)
    lam, p_eq0 = KM.two_state_mode(rate) if which == "two_state" else KM.star_mode(rate)
    want = KM.scheme_closed_form(lam, p_eq0, ms, hs)
    got, res = KM.mirror_ext(rate.T, ms, hs)
    assert res < KM.residual_limit(len(rate))
    err = np.abs(got[:, 0] - want).max()
    print(f"{which}: mirror_ext against the scheme's closed form {err:.3e}, residual {res:.3e}")
    assert got.dtype == want.dtype == np.longdouble and err <= 1e-17
    # the scheme is not the differential equation: the closed form of the ODE is further away than any rounding
    exact = K.two_state_populations(-1.0, K.KT, times) if which == "two_state" else \
        K.star_populations(K.SOLVER_STAR_LEAVES, K.SOLVER_STAR_ENERGY, K.KT, times)
    assert np.abs(got - exact).max() > 1e-8


@pytest.mark.parametrize("name", ["example_rafft_20.out", "example_rafft.out"])
def test_mirror_ext_is_second_order_against_the_60_digit_truth(name):
    tr = load_json_gz("kinetics_truth.json.gz")[name]
    A = host_rate(name).T
    ks, want = tr["sample_index"], np.array(tr["populations"])
    early = [i for i, s in enumerate(ks) if s <= 0.6 * tr["n_steps"]]
    errs = []
    for m in (8, 16):
        _, ms, hs = rafft_kin.kinetics_schedule(tr["max_time"], tr["n_steps"], m)
        P, res = KM.mirror_ext(A, ms, hs)
        assert res < KM.residual_limit(len(A))
        errs.append(np.abs(P[ks][early] - want[early]).max())
    print(f"{name}: mirror_ext against the truth over the first 60 %: {errs[0]:.3e} at substeps 8, {errs[1]:.3e} at 16, ratio {errs[1] / errs[0]:.4f}")
    assert 1 / 5 < errs[1] / errs[0] < 1 / 3


@pytest.mark.parametrize("name", ["traj3", "traj34", "example_rafft_20.out"])
def test_bound_passes_the_restated_kernel_and_fails_the_mutants(name):
    A = host_rate(name).T
    ext, f64, ms, hs = mirrors(name)
    lim = KM.bound(KM.row_error(f64, ext), ms, 10)
    ratio = KM.row_error(KM.restated_f64(A, ms, hs), ext) / (lim / 10)
    print(f"{name}: {len(A)} states, delta {KM.row_error(f64, ext).max():.3e}, restated / bound-without-factor per time: "
          + " ".join(f"{r:.2f}" for r in ratio))
    assert (ratio < 10).all()
    for mutant in (KM.mutant_stale_inverse, KM.mutant_no_reset):
        with np.errstate(all="ignore"):
            over = KM.row_error(mutant(A, ms, hs), ext) / lim
        over = over[np.isfinite(over)]                      # (the mutants end in overflow; the finite rows before that decide)
        print(f"{name}: {mutant.__name__} exceeds the bound by up to {float(over.max()):.3e} at a time of finite populations")
        assert over.max() >= 1000


@pytest.mark.parametrize("name", ["traj3", "example_rafft_20.out"])
def test_mirror_f64_runs_the_scheme_of_the_host_solver(name):
    import torch
    rate = host_rate(name)
    ext, f64, ms, hs = mirrors(name)
    times, substeps = schedule_of(name)[0], 8 if name.endswith(".out") else 4
    assert rafft_kin.kinetics_schedule(sample_times=times, substeps=substeps)[1:] == (ms, hs)
    p0 = torch.zeros(len(rate), dtype=torch.float64)
    p0[0] = 1.0
    got = rafft_kin.solve_master_equation(torch.as_tensor(np.array(rate)), np.zeros(len(rate)), p0, times, "implicit-dense", substeps)
    ratio = KM.row_error(got, f64) / KM.bound(KM.row_error(f64, ext), ms, 1)
    print(f"{name}: solve_master_equation(implicit-dense) against mirror_f64, over the bound without factor: {ratio.max():.2f}")
    assert (ratio < 10).all()
