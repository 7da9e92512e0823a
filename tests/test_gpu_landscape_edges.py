"""The landscape kernels (rafft_landscape.hip) where folded graphs never take them, on the constructed inputs of
_landscape_cases.py: distances entry by entry at the tile edges and at the longest length, SMACOF at the edges of the host's
pass chunks, with more starts than compute units and on both sides of the switch from X in LDS to X through the caches, and the
thin-plate surface with every node on a grid point, called without the solve.

Bounds are those of test_gpu_landscape.py: FACTOR * max(delta, spacing), where delta is what fp64 rounding alone does to the
same problem (float64 against longdouble restatement; at S = 8192 / 8193 the float64 restatement on the points in their order
against the reversed order), and spacing is the spacing of the numbers compared.

Measured on an MI355X (printed by the tests):
  chunk edges (S = 40, max_iter 63 .. 129)   |X_gpu - X_longdouble| 2.8e-14 = one spacing of |X| ~ 200, 0.99 to 2.26 x delta_x (1.3e-14 to
                                             2.9e-14); stress error 2.1e-14 to 1.9e-13 at a stress of 58.6, at most 5.7 x max(delta, spacing)
  S = 8192 (X in 128 KiB of LDS)             |X_gpu - X_ref| 5.7e-14 = 2.0 x delta_x (2.8e-14); the three stresses (1.3e11, spacing 1.5e-5) off
                                             by 1, 1 and 0 spacings, the restatement pair by 2, 1 and 1
  S = 8193 (X through the caches)            |X_gpu - X_ref| 5.7e-14 = 1.0 x delta_x (5.7e-14); the three stresses off by 1 spacing each, the
                                             restatement pair by 0, 1 and 3
  surface, S = 255 .. 513 on the 34 x 34     |z_gpu - z_longdouble| 8.7e-11 to 1.0e-10 at |z| up to 1.1e5, 0.93 to 1.00 x delta_z (8.9e-11 to
  lattice grid                               1.0e-10)
  surface, S = 257, G = 1, 2, 3, 17          4.4e-11 to 8.7e-11, 0.91 to 1.03 x delta_z
- all within 6 x delta, so FACTOR = 100 holds as it does in test_gpu_landscape.py.  The whole file takes 16 s, 13 s of them the four
float64 restatement runs at S = 8192 and 8193 on the CPU."""
import math

import numpy as np
import pytest

import _landscape_cases as LC
import _landscape_np as NP
from rafft_amd import _native, landscape as LS

pytestmark = pytest.mark.gpu

FACTOR = 100
PLANE_SEED = 40              # of the 40-point distance matrix and of its starts (test_landscape_cases.py checks what they promise)


def bp_matrix(structs):
    """bp_distance of every pair (the pair sets taken once per structure)"""
    sets = [NP.pair_set(s) for s in structs]
    return np.array([[len(a ^ b) for b in sets] for a in sets], dtype=np.int64)


def within(got, truth, delta):
    """-> (largest error, its ratio to delta, everything within FACTOR * max(delta, spacing of the truth))"""
    truth = np.asarray(truth, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - truth)
    ok = bool((err <= FACTOR * np.maximum(delta, np.spacing(np.abs(truth)))).all())
    return float(err.max()), float(err.max() / delta) if delta > 0 else math.inf, ok


# ------------------------------------------------------------------------------------------------------------------ distances

@pytest.mark.parametrize("k", range(len(LC.DISTANCE_SHAPES)), ids=[f"n{n}_L{L}" for n, L in LC.DISTANCE_SHAPES])
def test_distances_whole_matrix_at_tile_edges(k):
    name, structs = LC.distance_sets()[k]
    D = LS.distance_matrix_gpu(structs).cpu().numpy()
    assert D.dtype == np.uint16 and D.shape == (len(structs), len(structs))
    assert np.array_equal(D.astype(np.int64), bp_matrix(structs))


def test_distances_at_the_longest_length():
    structs = LC.long_set()
    D = LS.distance_matrix_gpu(structs).cpu().numpy()
    want = bp_matrix(structs)
    assert want.max() == 32766
    assert D.dtype == np.uint16 and np.array_equal(D.astype(np.int64), want)


# --------------------------------------------------------------------------------------------------------------------- SMACOF

@pytest.fixture(scope="module")
def plane40():
    import torch
    Dh = LC.rounded_plane_distances(40, PLANE_SEED)
    return Dh, torch.as_tensor(Dh, device="cuda")


@pytest.mark.parametrize("max_iter", [63, 64, 65, 128, 129])
def test_smacof_ends_at_a_chunk_edge(plane40, max_iter):
    """the host enqueues max_iter + 1 passes in chunks of 64 and reads the `done` words after each chunk; the last pass (stress only)
    is the last of a chunk at 63, alone in a chunk of its own at 64 and 128"""
    Dh, D = plane40
    X0 = LS.draw_starts(40, 1, PLANE_SEED)
    c0 = LS.mds_counters()
    X, stress, n_iter, _ = LS.mds_gpu(D, max_iter=max_iter, eps=-1.0, init=X0)
    c1 = LS.mds_counters()
    assert n_iter == max_iter
    assert c1[0] - c0[0] == 1 and c1[3] == max_iter + 1 == c1[1] - c0[1]
    assert c1[2] - c0[2] == math.ceil((max_iter + 1) / 64)
    Xt, st_t, nt, _, _ = NP.smacof(Dh, X0[0], max_iter, -1.0, dtype=np.longdouble)
    Xd, st_d, nd, _, _ = NP.smacof(Dh, X0[0], max_iter, -1.0)
    assert nt == nd == max_iter
    delta_x = float(np.abs(Xd - Xt).max())
    delta_s = float(abs(st_d - st_t))
    ex, rx, ok_x = within(X, Xt, delta_x)
    es, rs, ok_s = within(stress, st_t, delta_s)
    print(f"max_iter {max_iter}: |X_gpu - X_longdouble| {ex:.3e} ({rx:.2f} x delta {delta_x:.3e}), stress {stress!r}: err {es:.3e} (delta {delta_s:.3e}, "
          f"spacing {np.spacing(float(st_t)):.3e})")
    assert ok_x, (ex, delta_x)
    assert ok_s, (es, delta_s)


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_smacof_start_does_not_depend_on_its_neighbours(plane40):
    """300 starts are more than the compute units: one workgroup per start walks all rows by the grid stride, where a start alone has
    one workgroup per 16 rows.  Row sums are per wavefront and the order of the finalize sum depends on S only, so a start's bits
    are the same in both."""
    Dh, D = plane40
    X0 = LS.draw_starts(40, 300, PLANE_SEED + 1)
    Xs, stresses, n_iters = LS.mds_gpu(D, max_iter=20, eps=-1.0, init=X0)[3]
    assert Xs.shape == (300, 40, 2) and (n_iters == 20).all() and np.isfinite(Xs).all()
    assert len({x.tobytes() for x in Xs}) == 300                                 # every start got its own X_0
    for k in (0, 149, 299):
        one = LS.mds_gpu(D, max_iter=20, eps=-1.0, init=X0[k])[3]
        assert same_bytes((Xs[k], stresses[k], n_iters[k]), (one[0][0], one[1][0], one[2][0])), k
    Xt, st_t, _, _, _ = NP.smacof(Dh, X0[299], 20, -1.0, dtype=np.longdouble)    # and it is that start's iteration
    Xd, st_d, _, _, _ = NP.smacof(Dh, X0[299], 20, -1.0)
    assert within(Xs[299], Xt, float(np.abs(Xd - Xt).max()))[2] and within(stresses[299], st_t, float(abs(st_d - st_t)))[2]


def test_smacof_starts_that_stop_at_different_passes(plane40):
    """a start that has stopped is skipped by the later passes of the call; the others go on as if alone"""
    Dh, D = plane40
    X0 = LS.draw_starts(40, 5, PLANE_SEED)
    Xs, stresses, n_iters = LS.mds_gpu(D, max_iter=300, eps=1e-3, init=X0)[3]
    print("n_iter of the five starts:", list(n_iters))
    assert len(set(int(n) for n in n_iters)) > 1 and n_iters.max() < 300
    assert list(n_iters) == [NP.smacof(Dh, x0, 300, 1e-3)[2] for x0 in X0]
    for k in range(5):
        one = LS.mds_gpu(D, max_iter=300, eps=1e-3, init=X0[k])[3]
        assert same_bytes((Xs[k], stresses[k], n_iters[k]), (one[0][0], one[1][0], one[2][0])), k


@pytest.mark.parametrize("S", [8192, 8193])
def test_smacof_both_sides_of_the_lds_switch(S):
    """S = 8192 holds X in all 128 KiB of dynamic LDS; from S = 8193 the kernel reads X through the caches.  3 iterations, one start."""
    import torch
    Dh = LC.rounded_plane_distances(S, S)
    D = torch.as_tensor(Dh, device="cuda")
    X0 = LS.draw_starts(S, 1, S)
    got = [LS.mds_gpu(D, max_iter=k, eps=-1.0, init=X0) for k in (1, 2, 3)]
    assert [g[2] for g in got] == [1, 2, 3]
    Xt, _, nt, st_t, _ = NP.smacof(Dh, X0[0], 3, -1.0)
    Xr, _, nr, st_d, _ = NP.smacof(Dh[::-1, ::-1], X0[0][::-1], 3, -1.0)
    assert nt == nr == 3
    delta_x = float(np.abs(Xr[::-1] - Xt).max())
    d_st = np.abs(np.array(st_d) - np.array(st_t))
    ex, rx, ok_x = within(got[-1][0], Xt, delta_x)
    st_g = np.array([g[1] for g in got])
    e_st = np.abs(st_g - np.array(st_t))
    sp = np.spacing(np.array(st_t))
    print(f"S {S}: |X_gpu - X_ref| {ex:.3e} ({rx:.2f} x delta {delta_x:.3e}), stress err {e_st.tolist()} (delta {d_st.tolist()}, spacing {sp.tolist()})")
    assert (np.diff(st_g) <= 0).all()
    assert ok_x, (ex, delta_x)
    assert (e_st <= FACTOR * np.maximum(d_st, sp)).all()


# --------------------------------------------------------------------------------------------------------- thin-plate surface

def surface_direct(pos, w, G, lo, hi):
    """landscape_tps_kernel with given weights: no system matrix and no solve"""
    import torch
    X = torch.as_tensor(np.ascontiguousarray(pos, dtype=np.float64), device="cuda")
    W = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64), device="cuda")
    z = torch.full((G, G), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _native.check(_native.lib().rafft_landscape_surface(len(pos), X.data_ptr(), W.data_ptr(), int(G), lo, hi, z.data_ptr(), None))
    return z.cpu().numpy()


def check_surface(pos, w, G, lo, hi, what):
    ti = np.linspace(lo, hi, G)
    z = surface_direct(pos, w, G, lo, hi)
    zt = LC.tps_sum(pos, w, ti, np.longdouble)
    delta = float(np.abs(LC.tps_sum(pos, w, ti, np.float64) - zt).max())
    assert z.shape == (G, G) and np.isfinite(z).all()
    err, ratio, ok = within(z, zt, delta)
    print(f"{what}: |z_gpu - z_longdouble| {err:.3e} ({ratio:.2f} x delta_z {delta:.3e}), |z| max {float(np.abs(zt).max()):.3e}")
    assert ok, (err, delta)


@pytest.mark.parametrize("S", LC.LATTICE_SIZES)
def test_surface_with_every_node_on_a_grid_point(S):
    pos, w = LC.lattice_nodes(S, LC.LATTICE_SEED)
    lo, hi, G = LC.lattice_grid(pos)
    assert G * G % 256 != 0
    check_surface(pos, w, G, lo, hi, f"S {S}, G {G}")


@pytest.mark.parametrize("S", LC.LATTICE_SIZES)
def test_system_matrix_on_the_lattice(S):
    pos, _ = LC.lattice_nodes(S, LC.LATTICE_SEED)
    phi = LS.tps_matrix_gpu(pos)[0].cpu().numpy()
    np.testing.assert_allclose(phi, NP.tps_matrix(pos), rtol=1e-13, atol=1e-13)
    d = pos[:, None, :] - pos[None, :, :]
    r2 = (d ** 2).sum(axis=2)
    assert (r2 == 1).sum() >= 2
    assert not phi.diagonal().any()
    assert not phi[r2 == 1].any()                                                # log 1 = 0
    assert phi.tobytes() == np.ascontiguousarray(phi.T).tobytes()


@pytest.mark.parametrize("G", [1, 2, 3, 17])
def test_surface_small_grids(G):
    pos, w = LC.lattice_nodes(257, LC.LATTICE_SEED)
    lo, hi, _ = LC.lattice_grid(pos)
    check_surface(pos, w, G, lo, hi, f"S 257, G {G}")
