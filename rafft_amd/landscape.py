"""Folding landscape of a fast-folding graph (the third analysis of the reference's README: utility/surface.py,
example/landscape.png) on the MI355X.

utility/surface.py does three pieces of arithmetic, each quadratic or worse in the number S of unique structures, and draws the
result; here the arithmetic is HIP (rafft_amd/csrc/rafft_landscape.hip, C-ABI rafft_landscape_*) and the drawing stays optional:

  distance_matrix_gpu   surface.py:19-26     base-pair distance between every two structures (ViennaRNA's bp_distance: the
                                             number of pairs in exactly one of the two)
  mds_gpu               surface.py:98-101    metric MDS onto a plane, scikit-learn's SMACOF iteration and stopping rule, all starts
                                             at once, the stopping decision on the device
  surface_gpu           surface.py:107-111   thin-plate interpolation of the energies over the plane (scipy's Rbf, smooth = 0):
                                             system matrix and grid evaluation as kernels, the dense solve through rocSOLVER
                                             (torch.linalg.solve)
  landscape             surface.py:81-111    the whole of main() minus the drawing

No CPU fallback and no scikit-learn / scipy import: the starts are drawn with numpy exactly as scikit-learn draws them on the
path the reference takes (n_jobs=20), so positions are comparable with the reference's picture."""
import sys
from collections import namedtuple

import numpy as np

from . import rafft_kin
from .utils import Structure

Landscape = namedtuple("Landscape", "structs energies D pos stress n_iter ti z i_start i_min winner")      # winner: index of the best start

N_COMPONENTS = 2        # the only value the reference uses; the kernels keep a point in one 16-byte LDS word


def unique_structures(fast_paths):
    """Structures in order of first appearance over all steps (surface.py:29-40) -> (structures, energies)."""
    ordered, _ = rafft_kin.unique_structures(fast_paths)
    return [s.str_struct for s in ordered], np.array([float(s.energy) for s in ordered], dtype=np.float64)


def parse_barrier_output(infile):
    """surface.py:43-51: `<index> <structure> <energy> ...` lines after the sequence -> (fast_paths with one step, sequence)."""
    step = []
    with open(infile) as fh:
        seq = fh.readline().strip()
        for line in fh:
            val = line.strip().split()
            if len(val) >= 3:
                step.append(Structure(val[1], energy=float(val[2])))
    return [step], seq


def parse_subopt_output(infile, prob=1.0, seed=None):
    """surface.py:54-63: `<structure> <energy>` lines after the sequence, each kept with probability `prob` (the reference draws
    from the unseeded global generator; here a seed makes the sample repeatable)."""
    import random
    rng = random.Random(seed)
    step = []
    with open(infile) as fh:
        seq = fh.readline().strip()
        for line in fh:
            val = line.strip().split()
            if len(val) >= 2 and rng.uniform(0, 1) <= prob:
                step.append(Structure(val[0], energy=float(val[1])))
    return [step], seq


def distance_matrix_gpu(structs):
    """get_distance_matrix (surface.py:19-26) -> S x S torch.uint16 CUDA tensor, exact, zero diagonal."""
    import torch
    from . import _native as N
    structs = list(structs)
    S = len(structs)
    L = len(structs[0]) if S else 0
    if any(len(s) != L for s in structs):
        raise ValueError("structures of different lengths")
    if S < 1 or L < 1:
        raise ValueError("no structure")
    lib = N.lib()
    D = torch.empty((S, S), dtype=torch.uint16, device="cuda")
    torch.cuda.synchronize()
    N.check(lib.rafft_landscape_distances(S, L, "".join(structs).encode("ascii"), D.data_ptr()))
    return D


def draw_starts(S, n_init, random_state):
    """The initial configurations scikit-learn draws when `smacof` runs its starts as parallel jobs (the reference's n_jobs=20):
    seeds = RandomState(random_state).randint(iinfo(int32).max, size=n_init), start k = RandomState(seeds[k]).uniform(size=2 S)."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    seeds = rs.randint(np.iinfo(np.int32).max, size=n_init)
    return np.stack([np.random.RandomState(int(sd)).uniform(size=S * N_COMPONENTS).reshape(S, N_COMPONENTS) for sd in seeds])


def mds_gpu(D, n_init=4, max_iter=5000, eps=1e-9, random_state=3, init=None):
    """manifold.MDS(n_components=2, max_iter, eps, random_state, dissimilarity="precomputed").fit_transform(D) (surface.py:98-101).
    D: S x S torch.uint16 CUDA tensor (distance_matrix_gpu).  init: (n_init, S, 2) or (S, 2) initial configurations; without it
    they are drawn as scikit-learn draws them (draw_starts).  Returns (pos, stress, n_iter, all_starts): the start of smallest
    stress (the first on ties), and all_starts = (positions (n_init, S, 2), stresses, n_iters) as numpy arrays."""
    import ctypes as C
    import torch
    from . import _native as N
    if D.dtype != torch.uint16 or D.dim() != 2 or D.shape[0] != D.shape[1] or not D.is_cuda:
        raise ValueError("D must be a square torch.uint16 CUDA tensor (distance_matrix_gpu)")
    D = D.contiguous()
    S = D.shape[0]
    if init is None:
        x0 = draw_starts(S, n_init, random_state)
    else:
        x0 = np.array(init, dtype=np.float64)
        if x0.ndim == 2:
            x0 = x0[None]
        if x0.ndim != 3 or x0.shape[1] != S or x0.shape[2] != N_COMPONENTS:
            raise ValueError(f"init must have shape (n_init, {S}, {N_COMPONENTS}): two components only")
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    n_init = x0.shape[0]
    X = torch.empty((n_init, S, N_COMPONENTS), dtype=torch.float64, device="cuda")
    stress = np.zeros(n_init, dtype=np.float64)
    n_iter = np.zeros(n_init, dtype=np.int32)
    torch.cuda.synchronize()
    N.check(N.lib().rafft_landscape_mds(S, D.data_ptr(), n_init, x0.ctypes.data_as(C.POINTER(C.c_double)), int(max_iter), float(eps),
                                        X.data_ptr(), stress.ctypes.data_as(C.POINTER(C.c_double)), n_iter.ctypes.data_as(C.POINTER(C.c_int))))
    Xh = X.cpu().numpy()
    best = int(np.argmin(stress))
    return Xh[best], float(stress[best]), int(n_iter[best]), (Xh, stress, n_iter)


def mds_counters():
    """(MDS calls, SMACOF passes enqueued, host read-backs of the per-start `done` words, passes of the last call)"""
    import ctypes as C
    from . import _native as N
    out = (C.c_longlong * 4)()
    N.check(N.lib().rafft_landscape_counters(C.byref(out)))
    return tuple(out)


def tps_matrix_gpu(pos):
    """The S x S thin-plate system matrix phi(||X_i - X_j||), phi(r) = r^2 log r -> (torch float64 CUDA tensor, positions tensor)."""
    import torch
    from . import _native as N
    X = torch.as_tensor(np.ascontiguousarray(pos, dtype=np.float64), device="cuda")
    S = X.shape[0]
    if X.dim() != 2 or X.shape[1] != N_COMPONENTS:
        raise ValueError("positions must have shape (S, 2)")
    phi = torch.empty((S, S), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib().rafft_landscape_surface(S, X.data_ptr(), None, 0, 0.0, 0.0, None, phi.data_ptr()))
    return phi, X


def surface_gpu(pos, energies, grid=300, margin=1.0):
    """Rbf(pos[:, 0], pos[:, 1], energies, function="thin_plate") on meshgrid(ti, ti), ti = linspace(pos.min() - margin,
    pos.max() + margin, grid) (surface.py:107-111) -> (ti, z), z[i, j] = surface at (x = ti[j], y = ti[i]), numpy float64."""
    import torch
    from . import _native as N
    pos = np.asarray(pos, dtype=np.float64)
    energies = np.asarray(energies, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[0] < 3:
        raise ValueError("a thin-plate surface needs at least 3 structures")
    if energies.shape != (pos.shape[0],):
        raise ValueError("one energy per structure")
    phi, X = tps_matrix_gpu(pos)
    e = torch.as_tensor(energies, device="cuda")
    try:
        w = torch.linalg.solve(phi, e)
    except RuntimeError as exc:
        raise ValueError("singular thin-plate system: two structures share a position") from exc
    if not bool(torch.isfinite(w).all()):
        raise ValueError("singular thin-plate system: two structures share a position")
    lo, hi = float(pos.min() - margin), float(pos.max() + margin)
    ti = np.linspace(lo, hi, grid)
    z = torch.empty((grid, grid), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib().rafft_landscape_surface(X.shape[0], X.data_ptr(), w.data_ptr(), int(grid), lo, hi, z.data_ptr(), None))
    return ti, z.cpu().numpy()


def landscape_of(structs, energies, n_init=4, max_iter=5000, eps=1e-9, random_state=3, grid=300, margin=1.0):
    """surface.py:89-111 from the unique structures and their energies -> Landscape (D as a numpy array)."""
    energies = np.asarray(energies, dtype=np.float64)
    D = distance_matrix_gpu(structs)
    pos, stress, n_iter, (_, stresses, _) = mds_gpu(D, n_init, max_iter, eps, random_state)
    ti, z = surface_gpu(pos, energies, grid, margin)
    return Landscape(list(structs), energies, D.cpu().numpy(), pos, stress, n_iter, ti, z, 0, int(np.argmin(energies)), int(np.argmin(stresses)))


def landscape(fast_paths, **kw):
    """The whole of surface.py:main minus the drawing.  fast_paths: the graph (fold(..., traj=True)[1], parse_rafft_output) or the
    path of a `--traj` text file.  i_start = 0, i_min = the first structure of minimum energy (surface.py:103-104)."""
    if isinstance(fast_paths, str):
        from .utils import parse_rafft_output
        fast_paths, _ = parse_rafft_output(fast_paths)
    structs, energies = unique_structures(fast_paths)
    return landscape_of(structs, energies, **kw)


def draw(ls, out):
    """What surface.py:113-126 draws.  Returns False (one line on stderr) without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from matplotlib import cm
    except ImportError:
        print("rafft_landscape: matplotlib is not installed, no picture written", file=sys.stderr)
        return False
    plt.rcParams["font.family"] = "serif"
    plt.rcParams["font.size"] = 13
    fig, ax = plt.subplots()
    p1, p2 = np.meshgrid(ls.ti, ls.ti)
    ax.contour(p1, p2, ls.z, colors="k", linewidths=0.5, levels=7)
    ax.contourf(p1, p2, ls.z, cmap=cm.coolwarm, alpha=0.3, levels=7)
    ax.scatter(ls.pos[:, 0], ls.pos[:, 1], c=ls.energies, s=30, lw=0, label="MDS", cmap=cm.coolwarm, alpha=1.0)
    mark = [ls.i_start, ls.i_min]
    ax.scatter(ls.pos[mark, 0], ls.pos[mark, 1], c="black", s=80, lw=0, alpha=1.0)
    ax.scatter(ls.pos[mark, 0], ls.pos[mark, 1], c=np.asarray(ls.energies)[mark], s=30, lw=0, label="MDS", cmap=cm.coolwarm, alpha=1.0,
               vmin=float(np.min(ls.energies)), vmax=float(np.max(ls.energies)))
    fig.savefig(out, dpi=300, transparent=True)
    plt.close(fig)
    return True


def format_table(ls):
    """one line per structure `<structure> <energy> <x> <y>`, then `# stress S iterations N start K structures S`"""
    lines = ["{} {:.1f} {:.6f} {:.6f}".format(s, e, x, y) for s, e, (x, y) in zip(ls.structs, ls.energies, ls.pos)]
    lines.append("# stress {:.2f} iterations {:d} start {:d} structures {:d}".format(ls.stress, ls.n_iter, ls.winner, len(ls.structs)))
    return "\n".join(lines) + "\n"


def parse_arguments(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Folding landscape of a fast-folding graph (utility/surface.py): table of MDS positions, "
                                                 "optional picture and energy grid.")
    parser.add_argument("rafft_out", help="rafft --traj output (or a barriers / subopt file, or the binary side-car)")
    parser.add_argument("--out", "-o", help="picture file (needs matplotlib)")
    parser.add_argument("--bar", action="store_true", help="read barriers output")
    parser.add_argument("--sub", action="store_true", help="read subopt output")
    parser.add_argument("--samp_prob", "-sp", type=float, default=1.0, help="with --sub: keep each structure with this probability")
    parser.add_argument("--sidecar", action="store_true", help="rafft_out is the binary side-car written by `rafft --traj --sidecar`")
    parser.add_argument("--n_init", type=int, default=4, help="random starts of the MDS (scikit-learn's default: 4)")
    parser.add_argument("--max_iter", type=int, default=5000)
    parser.add_argument("--eps", type=float, default=1e-9)
    parser.add_argument("--seed", type=int, default=3, help="seed of the starts (and of the --sub sample)")
    parser.add_argument("--grid", type=int, default=300, help="points per side of the surface grid")
    parser.add_argument("--table", help="write the table to this file instead of stdout")
    parser.add_argument("--grid-out", dest="grid_out", help="write the surface to FILE.npy: row 0 = ti, rows 1.. = z")
    return parser.parse_args(argv)


def main(argv=None, compute=None):
    """bin/rafft_landscape.  `compute(structs, energies, n_init=, max_iter=, eps=, random_state=, grid=) -> Landscape` defaults to the
    GPU pipeline (landscape_of)."""
    args = parse_arguments(argv)
    if args.bar:
        fast_paths, seq = parse_barrier_output(args.rafft_out)
    elif args.sub:
        fast_paths, seq = parse_subopt_output(args.rafft_out, args.samp_prob, args.seed)
    elif args.sidecar:
        from .utils import read_sidecar
        fast_paths, seq = read_sidecar(args.rafft_out, text_energies=True)
    else:
        from .utils import parse_rafft_output
        fast_paths, seq = parse_rafft_output(args.rafft_out)
    if args.bar or args.sub:            # these readers keep every line (surface.py:43-63: no de-duplication)
        structs = [s.str_struct for s in fast_paths[0]]
        energies = np.array([float(s.energy) for s in fast_paths[0]], dtype=np.float64)
    else:
        structs, energies = unique_structures(fast_paths)
    if compute is None:
        compute = landscape_of
    ls = compute(structs, energies, n_init=args.n_init, max_iter=args.max_iter, eps=args.eps, random_state=args.seed, grid=args.grid)
    text = format_table(ls)
    if args.table:
        with open(args.table, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    if args.grid_out:
        np.save(args.grid_out, np.vstack([ls.ti[None, :], ls.z]))
    if args.out:
        draw(ls, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
