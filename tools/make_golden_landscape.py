"""Golden vectors of the folding landscape (tests/golden/landscape.json.gz), in the manner of make_golden.py.

usage: make_golden_landscape.py REFERENCE_DIR      (CPU only; needs the reference checkout, scikit-learn, scipy, matplotlib)

The reference's utility/surface.py is imported with a stand-in `RNA` module (ViennaRNA is not installed: ordinary
ModuleNotFoundError) whose `bp_distance` is the definition - the number of base pairs in exactly one of the two structures.  Its
own parse_rafft_output and get_distance_matrix produce D for example/rafft.out and example/rafft_20.out.  Then, recorded results
only (arrays and numbers, no program text):

  cases     seeds 3, 4, 5 x (max_iter, eps) = (50, 0), (5000, 1e-9): X0 = RandomState(seed).uniform(size=2 S).reshape(S, 2) and
            sklearn.manifold.smacof(D, metric=True, init=X0, n_init=1, max_iter, eps, return_n_iter=True,
            normalized_stress=False) -> X, stress, n_iter; the value of the stopping criterion at the last two iterations (a case
            is kept only if both are at least 1e-6 * eps away from eps: "same n_iter" is then a property of the algorithm, not
            of the last bit)
  pipeline  the reference's whole call, MDS(n_components=2, max_iter=5000, eps=1e-9, random_state=RandomState(3),
            dissimilarity="precomputed", n_jobs=20) of surface.py:98-101: positions, stress_, n_iter_, the n_init in effect, and
            every start on its own (stress, n_iter)
  rbf       Rbf(x, y, energies, function="thin_plate") on meshgrid(ti, ti), ti = linspace(min - 1, max + 1, 64)
  delta_*   the CPU-against-CPU yardstick: the same cases through a numpy restatement that sums in another order than
            scikit-learn's BLAS path (direct differences, row sums): delta_x = max |X_numpy - X_sklearn|, delta_stress
            (relative), delta_z = max |z_numpy - z_scipy|.  The tests scale their bounds from these.
"""
import gzip
import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")


def pair_set(db):
    stack, pairs = [], set()
    for x, c in enumerate(db):
        if c == "(":
            stack.append(x)
        elif c == ")":
            pairs.add((stack.pop(), x))
    return pairs


def bp_distance(a, b):
    return len(pair_set(a) ^ pair_set(b))


def smacof_numpy(D, X0, max_iter, eps, dtype=np.float64):
    """the iteration of sklearn.manifold._mds._smacof_single (metric, unnormalised stress) with direct differences
    -> X, stress, n_iter, [criterion values]"""
    D = D.astype(dtype)
    X = X0.astype(dtype)
    n = len(D)
    old, crit = None, []
    for it in range(max_iter):
        diff = X[:, None, :] - X[None, :, :]
        dis = np.sqrt((diff ** 2).sum(axis=2))
        ratio = D / np.where(dis == 0, dtype(1e-5), dis)
        X = (ratio[:, :, None] * diff).sum(axis=1) / dtype(n)
        diff = X[:, None, :] - X[None, :, :]
        dis = np.sqrt((diff ** 2).sum(axis=2))
        stress = ((dis - D) ** 2).sum(axis=1).sum() / 2
        if old is not None:
            crit.append(float((old - stress) / ((dis ** 2).sum(axis=1).sum() / 2)))
            if crit[-1] < eps:
                break
        old = stress
    return X, stress, it + 1, crit


def tps_numpy(pos, energies, ti):
    phi = lambda r: np.where(r == 0, 0.0, r * r * np.log(np.where(r == 0, 1.0, r)))
    d = pos[:, None, :] - pos[None, :, :]
    w = np.linalg.solve(phi(np.sqrt((d ** 2).sum(axis=2))), energies)
    gx, gy = np.meshgrid(ti, ti)
    r = np.sqrt((gx[:, :, None] - pos[None, None, :, 0]) ** 2 + (gy[:, :, None] - pos[None, None, :, 1]) ** 2)
    z = np.zeros_like(gx)
    for k in range(len(pos)):               # node order, as the kernel sums
        z += w[k] * phi(r[:, :, k])
    return z


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RAFFT_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    RNA = types.ModuleType("RNA")
    RNA.bp_distance = bp_distance
    sys.modules["RNA"] = RNA
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(ref, "utility"))
    import surface as SF
    from numpy.random import RandomState
    from scipy import interpolate
    from sklearn import manifold
    import sklearn
    import scipy

    out = {"versions": {"scikit-learn": sklearn.__version__, "scipy": scipy.__version__, "numpy": np.__version__}, "examples": {}}
    worst = {"delta_x": 0.0, "delta_stress": 0.0}
    for name, src in (("example_rafft.out", "rafft.out"), ("example_rafft_20.out", "rafft_20.out")):
        structures, seq = SF.parse_rafft_output(os.path.join(ref, "example", src))
        D = SF.get_distance_matrix(structures)
        S = len(structures)
        energies = np.array([e for _, e in structures])
        ex = {"structs": [s for s, _ in structures], "energies": energies.tolist(), "D": D.astype(int).tolist(), "cases": []}
        for seed in (3, 4, 5):
            for max_iter, eps in ((50, 0.0), (5000, 1e-9)):
                X0 = RandomState(seed).uniform(size=2 * S).reshape(S, 2)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    X, stress, n_iter = manifold.smacof(D, metric=True, init=X0.copy(), n_init=1, max_iter=max_iter, eps=eps,
                                                        return_n_iter=True, normalized_stress=False)
                Xn, sn, nn, crit = smacof_numpy(D, X0, max_iter, eps)
                last2 = crit[-2:]
                if not all(abs(c - eps) >= 1e-6 * eps for c in last2):
                    print(f"{name} seed {seed} ({max_iter}, {eps}): criterion {last2} too close to eps, case dropped")
                    continue
                assert nn == n_iter, (name, seed, max_iter, nn, n_iter)
                dx = float(np.abs(Xn - X).max())
                ds = float(abs(sn - stress) / stress)
                worst["delta_x"] = max(worst["delta_x"], dx)
                worst["delta_stress"] = max(worst["delta_stress"], ds)
                ex["cases"].append({"seed": seed, "max_iter": max_iter, "eps": eps, "x0": X0.tolist(), "x": X.tolist(), "stress": float(stress),
                                    "n_iter": int(n_iter), "criterion_last2": last2, "delta_x": dx, "delta_stress": ds})
                print(f"{name} seed {seed} ({max_iter}, {eps}): n_iter {n_iter} stress {stress:.6f} delta_x {dx:.2e} delta_stress {ds:.2e}")
        # the reference's whole call (surface.py:98-101)
        mds = manifold.MDS(n_components=2, max_iter=5000, eps=1e-9, random_state=RandomState(seed=3), dissimilarity="precomputed", n_jobs=20)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pos = mds.fit_transform(D)
            n_init = mds.n_init if isinstance(mds.n_init, int) else 4
            seeds = RandomState(3).randint(np.iinfo(np.int32).max, size=n_init)
            starts = []
            for sd in seeds:
                X0 = RandomState(int(sd)).uniform(size=2 * S).reshape(S, 2)
                X, stress, n_iter = manifold.smacof(D, metric=True, init=X0, n_init=1, max_iter=5000, eps=1e-9, return_n_iter=True,
                                                    normalized_stress=False)
                starts.append({"stress": float(stress), "n_iter": int(n_iter)})
        winner = int(np.argmin([s["stress"] for s in starts]))
        assert starts[winner]["stress"] == float(mds.stress_) and starts[winner]["n_iter"] == int(mds.n_iter_)
        ex["pipeline"] = {"pos": pos.tolist(), "stress": float(mds.stress_), "n_iter": int(mds.n_iter_), "n_init": int(n_init), "winner": winner,
                          "starts": starts}
        print(f"{name}: MDS stress {mds.stress_:.4f}, {mds.n_iter_} iterations, start {winner} of {n_init}")
        ti = np.linspace(np.min(pos) - 1, np.max(pos) + 1, 64)
        p1, p2 = np.meshgrid(ti, ti)
        z = interpolate.Rbf(pos[:, 0], pos[:, 1], energies, function="thin_plate")(p1, p2)
        dz = float(np.abs(tps_numpy(pos, energies, ti) - z).max())
        ex["rbf"] = {"ti": ti.tolist(), "z": z.tolist(), "delta_z": dz}
        print(f"{name}: delta_z {dz:.2e} at |z| <= {np.abs(z).max():.1f}")
        out["examples"][name] = ex
    out.update(worst)
    out["delta_z"] = {k: v["rbf"]["delta_z"] for k, v in out["examples"].items()}
    path = os.path.join(GOLD, "landscape.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(json.dumps(out).encode())
    print(path, os.path.getsize(path), "bytes;", worst)


if __name__ == "__main__":
    main()
