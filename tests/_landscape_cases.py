"""Constructed inputs for the landscape kernels (test_landscape_cases.py, test_gpu_landscape_edges.py): structure sets with
closed-form base-pair distances at the tile edges and at the longest length, distance matrices that need no structures, and
thin-plate nodes on an integer lattice, where grid points fall on nodes.  numpy only: no GPU and no torch."""
import numpy as np

L_MAX = 32767                                                    # the longest length rafft_landscape_distances accepts
DISTANCE_SHAPES = [(63, 1), (64, 2), (65, 63), (64, 64), (65, 65), (129, 127), (129, 129), (193, 200)]      # (structures, length)
LATTICE = 32                                                     # nodes of the thin-plate cases: cells of a LATTICE x LATTICE lattice
LATTICE_SIZES = [255, 256, 257, 513]                             # either side of the surface kernel's node tile of 256, and three tiles
LATTICE_SEED = 257
LONG_SEED = 3


def random_structure(L, rng, p_open, p_close):
    """a seeded random well-nested structure (the generator of test_gpu_scoring.py, round brackets only)"""
    out = ["."] * L
    stack = []
    for x in range(L):
        u = rng.random()
        if u < p_open:
            stack.append(x)
        elif u < p_open + p_close and stack:
            out[stack.pop()], out[x] = "(", ")"
    return "".join(out)


def deep(L, k):
    """k pairs nested around the middle: (i, L - 1 - i) for i < k"""
    return "(" * k + "." * (L - 2 * k) + ")" * k


def single(L, i, j):
    """the structure whose only pair is (i, j)"""
    s = ["."] * L
    s[i], s[j] = "(", ")"
    return "".join(s)


def closed_forms(L):
    """rows of length L whose distances are known without counting:
         deep    [(k, row)]        d(deep k, deep m) = |k - m|, d(deep k, unfolded) = k
         pairs   [((i, j), row)]   single pairs: (0, j) for several j, which share the opening position and differ in the partner, and
                                   (k, L - 1 - k); two different ones are at distance 2, and a single pair (k, L - 1 - k) is at
                                   distance m - 1 from deep m > k and m + 1 from deep m <= k
         open    the unfolded row"""
    ks = sorted({k for k in (1, 2, 3, L // 4, L // 2 - 1, L // 2) if 1 <= k and 2 * k <= L})
    js = sorted({j for j in (1, 2, 3, L // 2, L - 2, L - 1) if 1 <= j <= L - 1})
    ms = sorted({k for k in (0, 1, L // 4, (L - 2) // 2) if 0 <= k < L - 1 - k})
    pairs = {}
    for j in js:
        pairs[(0, j)] = single(L, 0, j)
    for k in ms:
        pairs[(k, L - 1 - k)] = single(L, k, L - 1 - k)
    return {"deep": [(k, deep(L, k)) for k in ks], "pairs": sorted(pairs.items()), "open": "." * L}


def distance_sets():
    """-> [(name, structures)]: n structures of length L for every (n, L) of DISTANCE_SHAPES: the closed forms of that length, one
    of them twice, then dense random structures that share nothing by construction (duplicates are allowed: distance_matrix_gpu
    does not de-duplicate)"""
    out = []
    for n, L in DISTANCE_SHAPES:
        cf = closed_forms(L)
        rows = [r for _, r in cf["deep"]] + [r for _, r in cf["pairs"]] + [cf["open"]]
        rows.append(rows[0])
        assert len(rows) < n
        rng = np.random.default_rng([n, L])
        rows += [random_structure(L, rng, 0.45, 0.45) for _ in range(n - len(rows))]
        out.append((f"n{n}_L{L}", rows))
    return out


def long_set():
    """7 rows at the longest length: the opening table then holds the partner 0x7fff, and rows 0 and 1 share no pair, which is the
    largest distance there is (2 * 16383 = 32766)"""
    L = L_MAX
    rng = np.random.default_rng(LONG_SEED)
    return [deep(L, 16383), "." + "(" * 16383 + ")" * 16383, "." * L, single(L, 0, L - 1), single(L, L - 2, L - 1),
            random_structure(L, rng, 0.45, 0.45), random_structure(L, rng, 0.45, 0.45)]


def rounded_plane_distances(S, seed, block=1024):
    """S integer points of [0, 200)^2, D = rint(euclidean distance) as uint16: symmetric, zero diagonal, zeros off the diagonal
    where two points coincide.  An MDS input of any size without structures."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 200, size=(S, 2)).astype(np.float64)
    D = np.empty((S, S), dtype=np.uint16)
    for a in range(0, S, block):
        dx = p[a:a + block, 0, None] - p[None, :, 0]
        dy = p[a:a + block, 1, None] - p[None, :, 1]
        D[a:a + block] = np.rint(np.sqrt(dx * dx + dy * dy)).astype(np.uint16)
    return D


def lattice_nodes(S, seed):
    """S distinct cells of the LATTICE x LATTICE integer lattice -> (positions (S, 2) float64, standard-normal weights (S,))"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(LATTICE * LATTICE, size=S, replace=False)
    pos = np.stack([cells % LATTICE, cells // LATTICE], axis=1).astype(np.float64)
    return pos, rng.standard_normal(S)


def lattice_grid(pos):
    """(lo, hi, G) of the grid linspace(min - 1, max + 1, G) with unit step: every node of a lattice set lies on one of its points"""
    lo, hi = float(pos.min() - 1), float(pos.max() + 1)
    return lo, hi, int(round(hi - lo)) + 1


def tps_sum(pos, w, ti, dtype):
    """z[i, j] = sum_k w_k phi(||(ti[j], ti[i]) - pos_k||), phi(r) = r^2 log r, phi(0) = 0, summed in node order in `dtype`"""
    pos, w, ti = np.asarray(pos).astype(dtype), np.asarray(w).astype(dtype), np.asarray(ti).astype(dtype)
    gx, gy = ti[None, :], ti[:, None]
    z = np.zeros((len(ti), len(ti)), dtype=dtype)
    for k in range(len(pos)):
        dx, dy = gx - pos[k, 0], gy - pos[k, 1]
        r = np.sqrt(dx * dx + dy * dy)
        z += w[k] * np.where(r == 0, dtype(0), (r * r) * np.log(np.where(r == 0, dtype(1), r)))
    return z
