"""The direct-path search of rafft_findpath_batch, twice, for its tests (test infrastructure; pure Python: no GPU, no product code).

* `search(seq, a, b, width, energy)`: a restatement of the search DESIGN.md section 13 defines - moves numbered removals first, an
  addition legal once its conflicting removals are applied, candidates sorted by (saddle, energy, parent rank, move number), the
  first `width` with distinct sets of applied moves kept - over WHOLE-STRUCTURE energies (`energy(seq, row)`, oracle.eval_structure by
  default): deliberately not incremental, so an error in the device's loop bookkeeping cannot hide in it.
* `exact_saddle(seq, a, b, energy)`: dynamic programming over all subsets of applied moves - the lowest saddle of ANY legal direct
  path (d <= ~16).
* `host_problems()`: the fixed list of short problems both test files use.
"""
import numpy as np

import oracle
import _mfe_np as MF


def pairs_of(row):
    stack, out = [], set()
    for x, c in enumerate(row):
        if c == "(":
            stack.append(x)
        elif c == ")":
            out.add((stack.pop(), x))
    assert not stack
    return out


def move_list(a, b):
    """(moves, n_rem): the pairs of a not in b ascending, then the pairs of b not in a ascending"""
    A, B = pairs_of(a), pairs_of(b)
    rem, add = sorted(A - B), sorted(B - A)
    return rem + add, len(rem)


def conflict_masks(moves, n_rem):
    """per move the bit mask of the removals that must be applied before it (0 for a removal)"""
    out = [0] * len(moves)
    for m in range(n_rem, len(moves)):
        i, j = moves[m]
        for r in range(n_rem):
            p, q = moves[r]
            if len({p, q, i, j}) < 4 or p < i < q < j or i < p < j < q:
                out[m] |= 1 << r
    return out


def row_of(a, moves, n_rem, mask):
    row = list(a)
    for m, (i, j) in enumerate(moves):
        if mask >> m & 1:
            row[i], row[j] = (".", ".") if m < n_rem else ("(", ")")
    return "".join(row)


def _energy_of(seq, a, moves, n_rem, energy):
    cache = {}

    def en(mask):
        if mask not in cache:
            cache[mask] = energy(seq, row_of(a, moves, n_rem, mask))
        return cache[mask]
    return en


def search(seq, a, b, width, energy=oracle.eval_structure):
    """dict(dist, start_dcal, end_dcal, saddle_dcal, saddle_step, moves, dcal): moves as the library reports them - (i, j) for an added
    pair, (-i-1, -j-1) for a removed one - and the dist + 1 energies"""
    moves, n_rem = move_list(a, b)
    d = len(moves)
    conf = conflict_masks(moves, n_rem)
    en = _energy_of(seq, a, moves, n_rem, energy)
    e0 = en(0)
    beam = [(e0, e0, 0, ())]                    # (saddle, energy, mask, moves so far), in rank order
    for _ in range(d):
        cand = []
        for rank, (sad, _e, mask, path) in enumerate(beam):
            for m in range(d):
                if mask >> m & 1 or conf[m] & ~mask:
                    continue
                e = en(mask | 1 << m)
                cand.append((max(sad, e), e, rank, m))
        cand.sort()
        nxt, seen = [], set()
        for sad, e, rank, m in cand:
            mask = beam[rank][2] | 1 << m
            if mask in seen:
                continue
            seen.add(mask)
            nxt.append((sad, e, mask, beam[rank][3] + (m,)))
            if len(nxt) == width:
                break
        beam = nxt
    path = beam[0][3]
    dcal, mask = [e0], 0
    for m in path:
        mask |= 1 << m
        dcal.append(en(mask))
    out_moves = [((-moves[m][0] - 1, -moves[m][1] - 1) if m < n_rem else moves[m]) for m in path]
    assert mask == (1 << d) - 1 and max(dcal) == beam[0][0]
    return dict(dist=d, start_dcal=e0, end_dcal=dcal[-1], saddle_dcal=max(dcal), saddle_step=dcal.index(max(dcal)), moves=out_moves, dcal=dcal)


def exact_saddle(seq, a, b, energy=oracle.eval_structure):
    moves, n_rem = move_list(a, b)
    d = len(moves)
    assert d <= 16
    conf = conflict_masks(moves, n_rem)
    en = _energy_of(seq, a, moves, n_rem, energy)
    INF = 10 ** 9
    best = [INF] * (1 << d)
    best[0] = en(0)
    for mask in range(1, 1 << d):
        lo = INF
        for m in range(d):
            prev = mask & ~(1 << m)
            if mask >> m & 1 and not conf[m] & ~prev and best[prev] < lo:
                lo = best[prev]
        if lo < INF:
            best[mask] = max(lo, en(mask))
    return best[-1]


SEED = 20261020


def host_problems(n=144, seed=SEED):
    """(seq, a, b) with 1 <= d <= 10: random 16-22-nt sequences over ACGU, a and b two different structures of the sequence's
    enumeration (canonical pairs, hairpins of at least 3), drawn with a fixed seed"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        seq = "".join(rng.choice(list("ACGU"), int(rng.integers(16, 23))))
        rows = MF.enumerate_structures(seq)
        if len(rows) < 8:
            continue
        for _ in range(4):
            a, b = (rows[int(x)] for x in rng.choice(len(rows), 2, replace=False))
            if 1 <= len(pairs_of(a) ^ pairs_of(b)) <= 10:
                out.append((seq, a, b))
    return out[:n]
