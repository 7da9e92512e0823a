"""The direct-path search of rafft_findpath_batch, three times, for its tests (test infrastructure; pure Python: no GPU, no product code).

* `search(seq, a, b, width, energy)`: a restatement of the search DESIGN.md section 13 defines - moves numbered removals first, an
  addition legal once its conflicting removals are applied, candidates sorted by (saddle, energy, parent rank, move number), the
  first `width` with distinct sets of applied moves kept - over WHOLE-STRUCTURE energies (`energy(seq, row)`, oracle.eval_structure by
  default): deliberately not incremental, so an error in the device's loop bookkeeping cannot hide in it.
* `exact_saddle(seq, a, b, energy)`: dynamic programming over all subsets of applied moves - the lowest saddle of ANY legal direct
  path (d <= ~16).
* `search_marked(...)`: the search once more, in the kernels' scheme - duplicates marked by comparing masks with the lower ranks, all
  unmarked candidates sorted, the first `width` kept - with the errors a kernel could make past 64 moves or 64 beam states as
  `defect`, and counts of how far a problem takes those loops (tests/_findpath_cases.py).
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
    """mask -> energy(seq, row of the mask), each mask once; an `energy` that carries a dict `masks` (of this seq, a, b alone) shares
    it among the searches it is passed to"""
    cache = getattr(energy, "masks", {})

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


STAT_KEYS = ("max_first_rank", "marks_ge64", "marks_ge128", "refused_high", "max_live", "max_k")
WORD = (1 << 64) - 1


def search_marked(seq, a, b, width, energy=oracle.eval_structure, defect=None, stats=None):
    """The same search the way the kernels carry it out (header of rafft_findpath.hip): no set of seen masks - state s marks move m
    when a state s' of lower rank has mask(s') \\ mask(s) = {m}; every unapplied, unmarked, legal (state, move) gets a key; the keys are
    sorted and the first `width` kept.  The dict of `search`, or None when a level has no candidate.

    `defect` states what a kernel with one error would compute (never compared with the device):
      "conf_word0"        only the removals numbered below 64 are looked at before an addition
      "dup_bit_word0"     the differing bit of a duplicate is taken modulo 64
      "dedup_rounds:r"    only the ranks below 64 r are examined for duplicates
      "moves_rounds:r"    only the moves numbered below 64 r are offered
    A defective search that has to evaluate a row that is no structure - an addition beside a pair that crosses it or shares a base
    with it, which no dot-bracket row states, or a row the oracle refuses - returns "invalid".
    `stats` (a dict) receives STAT_KEYS: the highest rank that was the FIRST to form a mark (-1: none), the marks at moves >= 64 and
    >= 128, the additions that only removals numbered >= 64 kept back, the largest beam, the largest K = min(candidates, width)."""
    kind, _, arg = (defect or "").partition(":")
    assert kind in ("", "conf_word0", "dup_bit_word0", "dedup_rounds", "moves_rounds"), defect
    moves, n_rem = move_list(a, b)
    d = len(moves)
    rank_cap = 64 * int(arg) if kind == "dedup_rounds" else width
    d_offer = min(d, 64 * int(arg)) if kind == "moves_rounds" else d
    conf = conflict_masks(moves, n_rem)
    en = _energy_of(seq, a, moves, n_rem, energy)
    st = {} if stats is None else stats
    st.update(dict.fromkeys(STAT_KEYS, 0), max_first_rank=-1)
    e0 = en(0)
    beam = [(e0, e0, 0, ())]                    # (saddle, energy, mask, moves so far), in rank order
    for _ in range(d):
        st["max_live"] = max(st["max_live"], len(beam))
        cand = []
        for rank, (sad, _e, mask, path) in enumerate(beam):
            marked = 0
            for r2 in range(min(rank, rank_cap)):
                x = beam[r2][2] & ~mask
                if x and not x & (x - 1):
                    m = (x.bit_length() - 1) & (63 if kind == "dup_bit_word0" else -1)
                    if not marked >> m & 1:
                        marked |= 1 << m
                        st["max_first_rank"] = max(st["max_first_rank"], r2)
                        st["marks_ge64"] += m >= 64
                        st["marks_ge128"] += m >= 128
            for m in range(d_offer):
                if (mask | marked) >> m & 1:
                    continue
                need = conf[m] & ~mask
                st["refused_high"] += need != 0 and not need & WORD
                if need and (kind != "conf_word0" or need & WORD):
                    continue
                if need:
                    return "invalid"
                try:
                    e = en(mask | 1 << m)
                except ValueError:
                    assert defect
                    return "invalid"
                cand.append((max(sad, e), e, rank, m))
        if not cand:
            return None
        cand.sort()
        st["max_k"] = max(st["max_k"], min(len(cand), width))
        beam = [(sad, e, beam[rank][2] | 1 << m, beam[rank][3] + (m,)) for sad, e, rank, m in cand[:width]]
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
