"""The barrier tree of rafft_barriers_batch, restated for its tests (test infrastructure; pure Python: no GPU, no product code).
Deliberately the OTHER algorithm: the sequential flooding of `barriers`, where the library reduces the landscape to a graph of
minima and runs Kruskal over it.

* `neighbour_ranks(rows)`: per row the ranks of its neighbours, from a dict of pair-frozensets and a scan over position pairs that
  knows nothing of loops: every (i, j) is toggled in the row's pair set and the result looked up.  Whatever the dict holds is a
  row that was handed over, so a hit IS a row that differs by exactly one pair; the scan is cut to the position pairs that occur
  in any row at all, since toggling any other pair cannot give a row of the list.
* `flood(rows)`: rows in rank order; a union-find that keeps the lowest rank as root; a row without a lower neighbour is a new
  minimum; at a multi-way merge every root that does not survive gets the survivor as father and the row as saddle.  Gradient
  basins separately, by chasing the lowest-ranked neighbour; edges from a plain double loop.
* `literal_tree(rows)`: the definition of include/rafft_hip.h taken literally (a breadth-first search per minimum and level).
"""
import numpy as np

import _descend_np as DS


def neighbour_ranks(rows):
    sets = [frozenset(DS.pairs_of(r)) for r in rows]
    index = {}
    for k, s in enumerate(sets):
        assert s not in index, ("duplicate row", index[s], k)
        index[s] = k
    all_pairs = sorted({p for s in sets for p in s})
    out = []
    for s in sets:
        nb = []
        for p in all_pairs:
            o = index.get(s ^ {p})
            if o is not None:
                nb.append(o)
        out.append(sorted(nb))
    return out


def flood(rows, dcal=None, nbs=None):
    """dict(rank, father, saddle_rank, saddle_dcal, dcal, basin_size: one entry per minimum, numbered by ascending rank; basin: per
    row its minimum index; edges: sorted [(a, b, saddle_rank)]; down: per row)"""
    n = len(rows)
    nbs = neighbour_ranks(rows) if nbs is None else nbs
    up = list(range(n))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    minima, father_rank, saddle = [], {}, {}
    for x in range(n):
        lower = [r for r in nbs[x] if r < x]
        if not lower:
            minima.append(x)
            continue
        roots = sorted({find(r) for r in lower})
        up[x] = roots[0]
        for r in roots[1:]:
            up[r] = roots[0]
            father_rank[r], saddle[r] = roots[0], x
    idx = {m: k for k, m in enumerate(minima)}
    down = [min(nbs[x]) if nbs[x] and min(nbs[x]) < x else x for x in range(n)]
    basin = []
    for x in range(n):
        while down[x] != x:
            x = down[x]
        basin.append(idx[x])
    edges = {}
    for x in range(n):
        for r in nbs[x]:
            if r < x and basin[r] != basin[x]:
                key = (min(basin[r], basin[x]), max(basin[r], basin[x]))
                edges[key] = min(edges.get(key, x), x)
    d = [0] * n if dcal is None else [int(v) for v in dcal]
    sr = [saddle.get(m, -1) for m in minima]
    return dict(rank=minima, father=[idx[father_rank[m]] if m in father_rank else -1 for m in minima], saddle_rank=sr,
                saddle_dcal=[d[t] if t >= 0 else 0 for t in sr], dcal=[d[m] for m in minima],
                basin_size=np.bincount(np.array(basin, dtype=np.int64), minlength=len(minima)).tolist(), basin=basin,
                edges=sorted((t, a, b) for (a, b), t in edges.items()), down=down)


def literal_tree(rows, nbs=None):
    """(rank, father, saddle_rank) per minimum from the definition alone: a minimum is a row without a lower-ranked neighbour; for
    a minimum m the smallest t such that the component of m among the rows of rank <= t holds a row of rank below m (found by
    bisection over t - components only grow with t - each probe a breadth-first search); father: the minimum index of the
    lowest-ranked row of that component"""
    n = len(rows)
    nbs = neighbour_ranks(rows) if nbs is None else nbs
    minima = [x for x in range(n) if not any(r < x for r in nbs[x])]
    idx = {m: k for k, m in enumerate(minima)}

    def lowest_of_component(m, t):
        seen, todo, low = {m}, [m], m
        while todo:
            x = todo.pop()
            for r in nbs[x]:
                if r <= t and r not in seen:
                    seen.add(r)
                    todo.append(r)
                    low = min(low, r)
        return low

    father, saddle = [], []
    for m in minima:
        if lowest_of_component(m, n - 1) == m:
            father.append(-1); saddle.append(-1)
            continue
        lo, hi = m, n - 1                 # at lo the component holds nothing below m (m is a minimum); at hi it does
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if lowest_of_component(m, mid) < m:
                hi = mid
            else:
                lo = mid
        father.append(idx[lowest_of_component(m, hi)]); saddle.append(hi)
    return minima, father, saddle


def matches(rec, want):
    """the first difference between a record of barriers_batch_raw and the mirror's dict, or None"""
    for key in ("rank", "father", "saddle_rank", "saddle_dcal", "dcal", "basin_size", "basin"):
        got = np.asarray(rec[key]).tolist()
        if got != list(want[key]):
            return key
    if [(int(t), int(a), int(b)) for a, b, t in rec["edges"]] != want["edges"]:
        return "edges"
    return None


def reverse_equal_runs(rows, dcal):
    """the same rows with every run of equal energies reversed"""
    out, k, n = [], 0, len(rows)
    while k < n:
        e = k
        while e < n and dcal[e] == dcal[k]:
            e += 1
        out.extend(range(e - 1, k - 1, -1))
        k = e
    return [rows[x] for x in out], [dcal[x] for x in out]


def tie_share(nbs, dcal):
    """the share of rows that have a neighbour of their own energy"""
    return sum(any(dcal[r] == dcal[x] for r in nbs[x]) for x in range(len(nbs))) / max(len(nbs), 1)
