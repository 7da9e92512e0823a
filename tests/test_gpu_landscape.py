"""Folding landscape on the GPU (rafft_amd/landscape.py, rafft_landscape.hip) against the recorded scikit-learn / scipy results
of tools/make_golden_landscape.py and the numpy restatements of _landscape_np.py.

Bounds.  delta_x / delta_stress / delta_z of the fixture are what re-ordering the fp64 sums does between two CPU implementations
(scikit-learn's BLAS path against a numpy restatement).  The GPU's tree reductions re-order more deeply and a few hundred
iterations carry the difference along; a factor of 1000 was allowed for that.  Measured on an MI355X: max |X_gpu - X_sklearn| =
2.7e-12 (1.04 x delta_x), relative stress difference 6.8e-15 (1.1 x delta_stress), |z_gpu - z_scipy| 2.3e-11 (0.8 x delta_z) - within
10 x delta, so the factor is 100."""
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import rafft_amd
import _landscape_np as NP
from rafft_amd import _native, landscape as LS, utils
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

EXAMPLES = ["example_rafft.out", "example_rafft_20.out"]
FACTOR = 100


@pytest.fixture(scope="module")
def fx():
    return NP.fixture()


@pytest.fixture(scope="module")
def graphs():
    """the 400-nt sequence of test_gpu_cfg5_graph_rate_matrix_and_kinetics (same generator seed) at ms=300 and ms=1000, and a
    sequence longer than 4096 nt at ms=3 -> name: (structures, energies)"""
    rng = np.random.default_rng(400)
    s = "".join(rng.choice(list("ACGU"), 400))
    out = {}
    for ms in (300, 1000):
        out[f"ms{ms}"] = LS.unique_structures(rafft_amd.fold(s, 100, ms, 1000, traj=True)[1])
    rng = np.random.default_rng(4321)
    s = "".join(rng.choice(list("ACGU"), 4331))                     # 67 chunks of 64 positions + 43
    out["long"] = LS.unique_structures(rafft_amd.fold(s, 100, 3, 1000, traj=True)[1])
    return out


@pytest.fixture(scope="module")
def dist(graphs):
    return {k: LS.distance_matrix_gpu(v[0]) for k, v in graphs.items()}


def x_bound(fx, X):
    return max(FACTOR * fx["delta_x"], 1e-12 * float(np.abs(X).max()))


# 1
@pytest.mark.parametrize("name", EXAMPLES)
def test_distances_small_equal_the_fixture(fx, name):
    ex = fx["examples"][name]
    D = LS.distance_matrix_gpu(ex["structs"]).cpu().numpy()
    assert D.dtype == np.uint16 and np.array_equal(D.astype(np.int64), np.array(ex["D"]))


# 2
@pytest.mark.parametrize("name", ["ms300", "ms1000", "long"])
def test_distances_large(graphs, dist, name):
    structs = graphs[name][0]
    S = len(structs)
    assert S > (1000 if name != "long" else 20)
    D = dist[name].cpu().numpy().astype(np.int64)
    assert D.shape == (S, S) and np.array_equal(D, D.T) and not D.diagonal().any()
    t, npairs = NP.pair_tables(structs)
    rng = np.random.default_rng(2)
    rows = rng.choice(S, size=min(300, S), replace=False)
    assert np.array_equal(D[rows], NP.distance_rows(t, npairs, rows))             # npairs[i] + npairs[j] - 2 common, exactly
    for i in rows[:5]:
        for j in rows[-5:]:
            assert D[i, j] == NP.bp_distance(structs[i], structs[j])
    a, b, c = rng.integers(0, S, size=(3, 100000))
    assert (D[a, c] <= D[a, b] + D[b, c]).all()                                   # bp distance is a metric
    off = D[~np.eye(S, dtype=bool)]
    assert off.min() >= 1 and off.max() <= len(structs[0])


# 3
def test_smacof_reproduces_every_scikit_learn_case(fx):
    worst_x = worst_s = 0.0
    for name in EXAMPLES:
        ex = fx["examples"][name]
        D = LS.distance_matrix_gpu(ex["structs"])
        for c in ex["cases"]:
            X, stress, n_iter, _ = LS.mds_gpu(D, max_iter=c["max_iter"], eps=c["eps"], init=np.array(c["x0"]))
            want = np.array(c["x"])
            dx, ds = float(np.abs(X - want).max()), abs(stress - c["stress"]) / c["stress"]
            print(f"{name} seed {c['seed']} ({c['max_iter']}, {c['eps']}): n_iter {n_iter} / {c['n_iter']}, |dX| {dx:.3e}, rel dstress {ds:.3e}")
            worst_x, worst_s = max(worst_x, dx), max(worst_s, ds)
            assert n_iter == c["n_iter"]
            assert ds <= FACTOR * fx["delta_stress"]
            assert dx <= x_bound(fx, want)
    print(f"GPU vs scikit-learn: max |dX| {worst_x:.3e} (delta_x {fx['delta_x']:.3e}), max rel dstress {worst_s:.3e} (delta_stress {fx['delta_stress']:.3e})")


# 4
def test_whole_pipeline_is_the_reference_call(fx):
    ex = fx["examples"]["example_rafft_20.out"]
    p = ex["pipeline"]
    fp, _ = utils.parse_rafft_output(os.path.join(GOLD, "example_rafft_20.out"))
    structs, energies = LS.unique_structures(fp)
    D = LS.distance_matrix_gpu(structs)
    pos, stress, n_iter, (Xs, stresses, n_iters) = LS.mds_gpu(D, n_init=4, random_state=3)
    assert p["n_init"] == 4 and int(np.argmin(stresses)) == p["winner"] and n_iter == p["n_iter"]
    assert list(n_iters) == [s["n_iter"] for s in p["starts"]]
    np.testing.assert_allclose(stresses, [s["stress"] for s in p["starts"]], rtol=FACTOR * fx["delta_stress"], atol=0)
    want = np.array(p["pos"])
    print(f"pipeline: |dX| {np.abs(pos - want).max():.3e}, stress {stress!r} / {p['stress']!r}")
    assert np.abs(pos - want).max() <= x_bound(fx, want)
    ls = rafft_amd.folding_landscape(fp, grid=32)
    assert np.array_equal(ls.pos, pos) and ls.n_iter == n_iter and ls.i_start == 0 and ls.i_min == int(np.argmin(energies)) and ls.winner == p["winner"]
    assert ls.z.shape == (32, 32) and np.isfinite(ls.z).all() and np.array_equal(ls.D, np.array(ex["D"]))


# 5
@pytest.mark.parametrize("name", ["ms300", "ms1000"])
def test_smacof_large_against_the_restatement(graphs, dist, name):
    """30 iterations, 2 starts, eps = 0.  ms=300: the numpy restatement in longdouble is the truth and delta = max |X_float64 -
    X_longdouble| of that same restatement the yardstick (what fp64 rounding alone does to this problem).  ms=1000 (S = 6001):
    longdouble takes minutes there, so the comparison is against the float64 restatement (torch CPU threads) and delta is the
    difference between that restatement on the points in their order and in reversed order - again fp64 re-ordering alone."""
    D = dist[name]
    Dh = D.cpu().numpy().astype(np.float64)
    S = len(Dh)
    X0 = LS.draw_starts(S, 2, 7)
    t0 = time.time()
    got = [LS.mds_gpu(D, max_iter=k, eps=0.0, init=X0)[3] for k in range(1, 31)]          # (Xs, stresses, n_iters) after k iterations
    t_gpu = time.time() - t0
    for k in range(2):
        t0 = time.time()
        if name == "ms300":
            Xt, _, _, st_t, _ = NP.smacof(Dh, X0[k], 30, 0.0, dtype=np.longdouble)
            Xd, _, _, st_d, _ = NP.smacof(Dh, X0[k], 30, 0.0)
        else:
            Xt, _, _, st_t, _ = NP.smacof_torch(Dh, X0[k], 30, 0.0)
            Xr, _, _, st_d, _ = NP.smacof_torch(Dh[::-1, ::-1].copy(), X0[k][::-1].copy(), 30, 0.0)
            Xd = Xr[::-1]
        delta = float(np.abs(np.asarray(Xd, dtype=np.float64) - np.asarray(Xt, dtype=np.float64)).max())
        d_st = np.abs(np.array(st_d, dtype=np.float64) - np.array(st_t, dtype=np.float64))
        Xg = got[-1][0][k]
        st_g = np.array([g[1][k] for g in got])
        err = float(np.abs(Xg - np.asarray(Xt, dtype=np.float64)).max())
        e_st = np.abs(st_g - np.array(st_t, dtype=np.float64))
        print(f"{name} start {k}: S {S}, |X_gpu - X_ref| {err:.3e}, delta {delta:.3e}, stress err max {e_st.max():.3e} (delta max {d_st.max():.3e}), "
              f"restatement {time.time() - t0:.1f} s, 30 GPU calls {t_gpu:.2f} s")
        assert [int(g[2][k]) for g in got] == list(range(1, 31))
        assert (np.diff(st_g) <= 0).all()
        assert err <= 100 * delta
        # (their own delta, but never below the spacing of the numbers: a restatement pair can agree to the last bit in one iteration)
        assert (e_st <= 100 * np.maximum(d_st, np.spacing(np.array(st_t, dtype=np.float64)))).all()


# 6
def test_device_side_stop(graphs, dist):
    D = dist["ms300"]
    Dh = D.cpu().numpy()
    X0 = LS.draw_starts(len(Dh), 1, 11)
    c0 = LS.mds_counters()
    t0 = time.time()
    X, stress, n_iter, _ = LS.mds_gpu(D, max_iter=5000, eps=1e-9, init=X0)
    t_gpu = time.time() - t0
    c1 = LS.mds_counters()
    Xr, sr, nr, _, crit = NP.smacof_torch(Dh, X0[0], 5000, 1e-9)
    margin_ok = all(abs(c - 1e-9) >= 1e-6 * 1e-9 for c in crit[-2:])
    print(f"device-side stop: n_iter {n_iter} (restatement {nr}, criterion {crit[-2:]}, margin rule holds: {margin_ok}), {t_gpu:.2f} s, "
          f"passes {c1[3]}, read-backs {c1[2] - c0[2]}, |dX| {np.abs(X - Xr).max():.3e}, stress {stress!r} / {sr!r}")
    assert n_iter < 5000
    if margin_ok:
        assert n_iter == nr
    else:                                   # the criterion sits within 1e-6 eps of eps: the last bit decides
        assert abs(n_iter - nr) <= 1
    # no host read-back per iteration: the `done` words are read once per chunk of 64 passes
    assert c1[0] - c0[0] == 1
    assert n_iter < c1[3] <= n_iter + 64
    assert c1[2] - c0[2] == math.ceil(c1[3] / 64)


# 7
def test_bit_reproducibility(graphs):
    structs, energies = graphs["ms300"]
    X0 = LS.draw_starts(len(structs), 2, 5)
    runs = []
    for _ in range(2):
        D = LS.distance_matrix_gpu(structs)
        pos, stress, n_iter, (Xs, stresses, n_iters) = LS.mds_gpu(D, max_iter=40, eps=0.0, init=X0)
        ti, z = LS.surface_gpu(pos, energies, grid=64)
        runs.append((D.cpu().numpy().tobytes(), Xs.tobytes(), stresses.tobytes(), ti.tobytes(), z.tobytes()))
    assert runs[0] == runs[1]


# 8
@pytest.mark.parametrize("name", EXAMPLES)
def test_surface_against_scipy(fx, name):
    import torch
    ex = fx["examples"][name]
    pos, energies = np.array(ex["pipeline"]["pos"]), np.array(ex["energies"])
    ti, z = LS.surface_gpu(pos, energies, grid=64)
    bound = FACTOR * fx["delta_z"][name]
    assert np.array_equal(ti, np.array(ex["rbf"]["ti"]))
    dz = float(np.abs(z - np.array(ex["rbf"]["z"])).max())
    phi, X = LS.tps_matrix_gpu(pos)
    np.testing.assert_allclose(phi.cpu().numpy(), NP.tps_matrix(pos), rtol=1e-13, atol=1e-13)
    w = torch.linalg.solve(phi, torch.as_tensor(energies, device="cuda"))
    res = float(np.abs(phi.cpu().numpy() @ w.cpu().numpy() - energies).max())      # at the nodes the surface returns the energies
    print(f"{name}: |z - z_scipy| {dz:.3e} (delta_z {fx['delta_z'][name]:.3e}), node residual {res:.3e}")
    assert dz <= bound and res <= bound


def test_surface_large(graphs, dist):
    import torch
    structs, energies = graphs["ms300"]
    pos = LS.mds_gpu(dist["ms300"], n_init=1, max_iter=300, eps=1e-9, random_state=3)[0]
    ti, z = LS.surface_gpu(pos, energies, grid=100)
    assert z.shape == (100, 100) and np.isfinite(z).all()
    phi, X = LS.tps_matrix_gpu(pos)
    Ph = phi.cpu().numpy()
    w = torch.linalg.solve(phi, torch.as_tensor(energies, device="cuda")).cpu().numpy()
    res = float(np.abs(Ph @ w - energies).max())
    res_np = float(np.abs(Ph @ np.linalg.solve(Ph, energies) - energies).max())
    print(f"ms300 surface: S {len(structs)}, residual {res:.3e} (numpy.linalg.solve {res_np:.3e}), |w| max {np.abs(w).max():.3e}")
    assert res <= 100 * res_np


# 9
def test_edges():
    import ctypes as C
    # a sequence that does not fold: the graph's only structure is the unfolded one
    fp = [[utils.Structure("." * 12, 0)]]
    structs, energies = LS.unique_structures(fp)
    D = LS.distance_matrix_gpu(structs)
    assert D.cpu().numpy().tolist() == [[0]]
    pos, stress, n_iter, _ = LS.mds_gpu(D, max_iter=100)
    assert pos.tolist() == [[0.0, 0.0]] and stress == 0.0
    D = LS.distance_matrix_gpu(["((....))....", "............"])
    assert D.cpu().numpy().tolist() == [[0, 2], [2, 0]]
    X0 = LS.draw_starts(2, 1, 3)
    pos, stress, n_iter, _ = LS.mds_gpu(D, max_iter=300, eps=1e-9, init=X0)
    Xr, sr, nr, _, _ = NP.smacof(np.array([[0, 2], [2, 0]]), X0[0], 300, 1e-9)
    assert n_iter == nr and np.abs(pos - Xr).max() < 1e-12 and abs(np.linalg.norm(pos[0] - pos[1]) - 2) < 1e-6
    for bad in ([")......(....", "............"], ["((....))....", "(((.....)).."], ["((....))....", "....x......."]):
        with pytest.raises(_native.RafftError) as e:
            LS.distance_matrix_gpu(bad)
        assert e.value.code == _native.ERR_STRUCT
    with pytest.raises(ValueError):
        LS.surface_gpu(np.array([[0.0, 0.0], [1.0, 0.0]]), np.array([0.0, -1.0]))
    with pytest.raises(ValueError):
        LS.surface_gpu(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0]]), np.array([0.0, -1.0, -2.0]))      # two structures on one point
    lib = _native.lib()
    buf = LS.distance_matrix_gpu(["...."])
    x0 = (C.c_double * 2)()
    st, ni = (C.c_double * 1)(), (C.c_int * 1)()
    assert lib.rafft_landscape_distances(0, 4, b"....", buf.data_ptr()) == _native.ERR_PARAM
    assert lib.rafft_landscape_distances(1, 32768, b"." * 32768, buf.data_ptr()) == _native.ERR_PARAM
    assert lib.rafft_landscape_mds(1, buf.data_ptr(), 0, x0, 10, 1e-9, buf.data_ptr(), st, ni) == _native.ERR_PARAM
    assert lib.rafft_landscape_mds(0, buf.data_ptr(), 1, x0, 10, 1e-9, buf.data_ptr(), st, ni) == _native.ERR_PARAM
    with pytest.raises(ValueError):
        LS.mds_gpu(buf, init=np.zeros((1, 1, 3)))                                   # two components only


# 10
def test_cli_as_a_process():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft_landscape"), os.path.join(GOLD, "example_rafft_20.out"), "--grid", "64"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 69 and all(len(l.split()) == 4 for l in lines[:68])
    f = lines[-1].split()
    assert f[0] == "#" and f[2] == "24698.83" and f[4] == "149"
