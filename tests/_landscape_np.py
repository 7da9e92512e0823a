"""numpy restatements of the folding-landscape arithmetic, shared by test_landscape.py and test_gpu_landscape.py.  They are the
specification the kernels are tested against; the product itself has no CPU path."""
import numpy as np

from conftest import load_json_gz


def fixture():
    return load_json_gz("landscape.json.gz")


def pair_set(db):
    stack, pairs = [], set()
    for x, c in enumerate(db):
        if c == "(":
            stack.append(x)
        elif c == ")":
            pairs.add((stack.pop(), x))
    return pairs


def bp_distance(a, b):
    """the number of base pairs in exactly one of the two structures"""
    return len(pair_set(a) ^ pair_set(b))


def pair_tables(structs):
    """(S, L) int32: 0-based partner of an opening position, else -1; and the number of pairs per structure"""
    L = len(structs[0])
    t = np.full((len(structs), L), -1, dtype=np.int32)
    for r, s in enumerate(structs):
        for i, j in pair_set(s):
            t[r, i] = j
    return t, (t >= 0).sum(axis=1)


def distance_rows(t, npairs, rows):
    """rows of the distance matrix from the opening tables: npairs[i] + npairs[j] - 2 common"""
    out = np.empty((len(rows), len(t)), dtype=np.int64)
    for k, i in enumerate(rows):
        common = ((t == t[i][None, :]) & (t >= 0)).sum(axis=1)
        out[k] = npairs[i] + npairs - 2 * common
    return out


def smacof(D, X0, max_iter, eps, dtype=np.float64, block=512):
    """sklearn.manifold._mds._smacof_single, metric case, unnormalised stress:
        dis_ij = ||X_i - X_j||, ratio_ij = D_ij / dis_ij (dis_ij == 0 -> 1e-5 in the ratio only),
        X'_i = (1/S) sum_j ratio_ij (X_i - X_j), stress = 1/2 sum_ij (||X'_i - X'_j|| - D_ij)^2 of the NEW configuration,
        stop after this iteration if (old_stress - stress) / (1/2 sum_ij ||X'_i - X'_j||^2) < eps (not in the first iteration).
    -> X, stress, n_iter, [stress of every iteration], [criterion of every iteration from the second]"""
    D = np.asarray(D).astype(dtype)
    X = np.asarray(X0).astype(dtype)
    n = len(D)

    def sweep(X, guttman):
        new, st, sq = np.zeros_like(X), dtype(0), dtype(0)
        for a in range(0, n, block):
            dx = X[a:a + block, 0, None] - X[None, :, 0]
            dy = X[a:a + block, 1, None] - X[None, :, 1]
            dis = np.sqrt(dx * dx + dy * dy)
            st += ((dis - D[a:a + block]) ** 2).sum(axis=1).sum()
            sq += (dis * dis).sum(axis=1).sum()
            if guttman:
                ratio = D[a:a + block] / np.where(dis == 0, dtype(1e-5), dis)
                new[a:a + block, 0] = (ratio * dx).sum(axis=1) / dtype(n)
                new[a:a + block, 1] = (ratio * dy).sum(axis=1) / dtype(n)
        return new, st / 2, sq / 2

    old, stresses, crit = None, [], []
    nxt, _, _ = sweep(X, True)
    for it in range(max_iter):
        X = nxt
        nxt, stress, half_sq = sweep(X, it + 1 < max_iter)       # one sweep: the stress of X and the next transform
        stresses.append(stress)
        if old is not None:
            crit.append((old - stress) / half_sq)
            if crit[-1] < eps:
                break
        old = stress
    return X, stress, it + 1, stresses, crit


def smacof_torch(D, X0, max_iter, eps):
    """the same iteration in float64 on torch's CPU threads, for the graphs with thousands of structures
    -> X, stress, n_iter, [stresses], [criteria] (numpy / floats)"""
    import torch
    D = torch.as_tensor(np.asarray(D, dtype=np.float64))
    X = torch.as_tensor(np.asarray(X0, dtype=np.float64))
    n = len(D)

    def sweep(X, guttman):
        dx = X[:, 0, None] - X[None, :, 0]
        dy = X[:, 1, None] - X[None, :, 1]
        dis = torch.sqrt(dx * dx + dy * dy)
        st = float(((dis - D) ** 2).sum(dim=1).sum()) / 2
        sq = float((dis * dis).sum(dim=1).sum()) / 2
        new = None
        if guttman:
            ratio = D / torch.where(dis == 0, torch.full_like(dis, 1e-5), dis)
            new = torch.stack([(ratio * dx).sum(dim=1), (ratio * dy).sum(dim=1)], dim=1) / n
        return new, st, sq

    old, stresses, crit = None, [], []
    nxt, _, _ = sweep(X, True)
    for it in range(max_iter):
        X = nxt
        nxt, stress, half_sq = sweep(X, it + 1 < max_iter)
        stresses.append(stress)
        if old is not None:
            crit.append((old - stress) / half_sq)
            if crit[-1] < eps:
                break
        old = stress
    return X.numpy(), stress, it + 1, stresses, crit


def tps_phi(r):
    return np.where(r == 0, 0.0, r * r * np.log(np.where(r == 0, 1.0, r)))


def tps_matrix(pos):
    d = pos[:, None, :] - pos[None, :, :]
    return tps_phi(np.sqrt((d ** 2).sum(axis=2)))


def tps_numpy_compute(structs, energies, n_init=4, max_iter=5000, eps=1e-9, random_state=3, grid=300):
    """a CPU stand-in for rafft_amd.landscape.landscape_of, for the CLI tests"""
    from rafft_amd import landscape as LS
    energies = np.asarray(energies, dtype=np.float64)
    D = np.array([[bp_distance(a, b) for b in structs] for a in structs])
    runs = [smacof(D, x0, max_iter, eps)[:3] for x0 in LS.draw_starts(len(structs), n_init, random_state)]
    best = int(np.argmin([r[1] for r in runs]))
    pos, stress, n_iter = runs[best]
    ti = np.linspace(pos.min() - 1, pos.max() + 1, grid)
    w = np.linalg.solve(tps_matrix(pos), energies)
    gx, gy = np.meshgrid(ti, ti)
    z = np.zeros_like(gx)
    for k in range(len(pos)):
        z += w[k] * tps_phi(np.sqrt((gx - pos[k, 0]) ** 2 + (gy - pos[k, 1]) ** 2))
    return LS.Landscape(list(structs), energies, D, pos, float(stress), n_iter, ti, z, 0, int(np.argmin(energies)), best)
