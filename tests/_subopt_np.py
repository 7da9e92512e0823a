"""Every structure within an energy band, for the tests of rafft_subopt_batch (test infrastructure; pure Python / numpy: no GPU, no
product code).

`band(mirror, seq, delta)` walks the decision tree of DESIGN.md section 12 over the tables of `_mfe_np.Mirror.fill` and the Mirror's
loop functions.  A state is (pairs so far, e_fixed, e_pending, LIFO stack of pending segments); a step pops the top segment, forms its
candidates in the documented order and keeps those with e_fixed + e_cand + e_pending' <= mfe + delta:
    F(0..j):  j unpaired -> F(0..j-1); stems (i,j), i ascending -> F(0..i-1), C(i,j)
    C(i,j):   hairpin; interior loops (p ascending, then q descending) -> C(p,q); multiloop splits, k ascending -> M(i+1,k-1), M1(k,j-1)
    M1(i,j):  j unpaired -> M1(i,j-1); the stem -> C(i,j)
    M(i,j):   k ascending from i: "unpaired alone before k" -> M1(k,j); then M(i,k-1), M1(k,j)
Of one candidate the segment named last above is pushed last, so it is expanded first.  An exterior segment shorter than five
positions holds nothing to choose and is not pushed.  The walk is depth first, so the leaves come out in the left-to-right order of
the tree - the order a level-synchronous expansion that keeps finished states in place arrives at; the rows are then ordered by a
stable sort on the energy.  The size of that expansion's frontier at level l is (states at depth l) + (leaves above l); the walk
counts both and reports the largest.
"""
from collections import defaultdict

import numpy as np

import _mfe_np as MF

BIG = MF.BIG


def band(mirror, seq, delta, with_stats=False):
    """[(row, dcal)] ordered by dcal ascending, equal energies in enumeration order; with_stats=True: (rows, dict(frontier=...,
    levels=...))"""
    L = len(seq)
    if seq not in mirror._filled:
        mirror._filled[seq] = mirror.fill(seq)
    S, Cn, M, M1, F = mirror._filled[seq]
    C, M, M1 = Cn.tolist(), M.tolist(), M1.tolist()         # (plain lists: the walk reads single cells)
    tabs = {"C": C, "M": M, "M1": M1}
    c_cands = {}                                            # the candidates of a C cell, formed once
    sc = mirror.sc
    mlb = sc["ml_base"]
    nb = lambda x: int(S[x]) if 0 <= x < L else -1
    limit = F[L] + delta
    cap = L // 5 + 2

    def tmin(seg):
        i, j, kind = seg
        return F[j + 1] if kind == "F" else tabs[kind][i][j]

    def candidates(seg):
        if seg[2] != "C":
            return candidates_of(seg)
        if seg not in c_cands:
            c_cands[seg] = list(candidates_of(seg))
        return c_cands[seg]

    def candidates_of(seg):
        """(loop terms fixed by the candidate, segments to push in push order), in the documented order"""
        i, j, kind = seg
        if kind == "F":
            yield 0, ([(0, j - 1, "F")] if j - 1 >= 4 else [])
            for a in range(0, j - 3):
                if C[a][j] < BIG:
                    e = mirror.stem(int(MF.PT[S[a], S[j]]), nb(a - 1), nb(j + 1), True)
                    yield e, ([(0, a - 1, "F")] if a - 1 >= 4 else []) + [(a, j, "C")]
        elif kind == "C":
            t = int(MF.PT[S[i], S[j]])
            assert t
            yield mirror.hairpin(seq, S, i, j), []
            il = mirror.interior_candidates(S, Cn, np.array([i]), np.array([j]))[0]
            for x in np.nonzero(il < BIG)[0]:
                p, q = i + 1 + int(MF._N1[x]), j - 1 - int(MF._N2[x])
                yield int(il[x]) - C[p][q], [(p, q, "C")]
            close = sc["ml_closing"] + mirror.stem(int(MF.RT[t]), int(S[j - 1]), int(S[i + 1]), False)
            for k in range(i + 6, j - 4):
                if M[i + 1][k - 1] < BIG and M1[k][j - 1] < BIG:
                    yield close, [(i + 1, k - 1, "M"), (k, j - 1, "M1")]
        elif kind == "M1":
            if j > i and M1[i][j - 1] < BIG:
                yield mlb, [(i, j - 1, "M1")]
            if C[i][j] < BIG:
                yield mirror.stem(int(MF.PT[S[i], S[j]]), nb(i - 1), nb(j + 1), False), [(i, j, "C")]
        else:
            for k in range(i, j - 3):
                if M1[k][j] >= BIG:
                    continue
                yield (k - i) * mlb, [(k, j, "M1")]
                if k - 1 - i >= 4 and M[i][k - 1] < BIG:
                    yield 0, [(i, k - 1, "M"), (k, j, "M1")]

    first = ((0, L - 1, "F"),) if L >= 5 else ()
    work = [(0, F[L] if L >= 5 else 0, first, None, 0)]
    leaves_e, leaves_p = [], []
    at_depth, leaves_at = defaultdict(int), defaultdict(int)
    while work:
        ef, ep, segs, pairs, depth = work.pop()
        at_depth[depth] += 1
        if not segs:
            leaves_at[depth] += 1
            leaves_e.append(ef)
            leaves_p.append(pairs)
            continue
        seg, rest = segs[-1], segs[:-1]
        base_p = ep - tmin(seg)
        if seg[2] == "C":
            pairs = (seg[0], seg[1], pairs)
        kept = []
        for e, push in candidates(seg):
            ep2 = base_p + sum(tmin(x) for x in push)
            if ef + e + ep2 <= limit:
                assert len(rest) + len(push) <= cap, "more pending segments than L / 5 + 2"
                kept.append((ef + e, ep2, rest + tuple(push), pairs, depth + 1))
        assert kept, "a kept state has no kept candidate"
        work.extend(reversed(kept))
    rows = []
    for pairs in leaves_p:
        db = ["."] * L
        while pairs is not None:
            db[pairs[0]], db[pairs[1]] = "(", ")"
            pairs = pairs[2]
        rows.append("".join(db))
    order = sorted(range(len(rows)), key=lambda k: leaves_e[k])          # (stable)
    out = [(rows[k], leaves_e[k]) for k in order]
    if not with_stats:
        return out
    frontier, above = 0, 0
    for d in range(max(at_depth) + 1):
        frontier = max(frontier, at_depth[d] + above)
        above += leaves_at[d]
    return out, dict(frontier=frontier, levels=max(at_depth))
