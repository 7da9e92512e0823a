"""Two-strand dimers, twice, for the tests of rafft_cofold_batch (test infrastructure; pure Python / numpy: no GPU, no product code).
A dimer is the concatenation seq = A B with cut c = len(A): position c is the first base of B, the nick is the missing bond
between c-1 and c.  DESIGN.md section 22 states the model.

* `enumerate_dimer(seq, c)`: every structure of the dimer as a dot-bracket string without a separator - canonical non-crossing
  pairs, a pair on one strand encloses at least 3 positions, a pair (i,j) with i < c <= j any number.
* `dimer_energy(mirror, seq, c, row, duplex_init)`: the definition, loop by loop, from `_mfe_np.Mirror`'s loop functions.  The nick
  lies in the exterior loop, or in the loop closed by the innermost pair that spans it.  That loop and the exterior loop are
  exterior loops - 0 for unpaired positions, stem(.., ext=True) for every stem, the closing pair of the nick loop read from inside,
  a neighbour across a strand end absent - every other loop is what it is for a single strand, and duplex_init is added once iff a
  pair spans the nick.
* `CutMirror(tables, duplex_init)`: the recurrences of section 22 and their traceback in the documented candidate order ("first")
  or with the last reproducing candidate of every cell ("last").  `defect` gives a mirror with a defect, there to show what the
  enumeration check catches: "split_k" - the splits of M and of the multiloop term forget that the bond before k must exist,
  which changes nothing, because M1[c][j] holds no structure anyway (its stem needs i != c): the test of the splits is implied;
  "branch_start" - the splits and M1's stem all forget it, so a multiloop takes a branch that begins at c across the nick;
  "fa_two_rounds" / "fb_two_rounds" - FA keeps the stems (i,j) with j < i + 4 + 128 only, FB the stems (i,j) with i < c + 128:
  what a 64-lane loop over the candidates of a strand end computes when it stops after two rounds (values only: `mfe_cut`).
  After `fold_cut`, `ties` counts per kind of decision - F, FA, FB, M, M1, C_intra, C_cross - the decision points of that
  traceback with more than one reproducing candidate, and for the cross cells how many of them set the nick loop against an
  interior loop (C_cross_nick_interior) and against a split (C_cross_nick_split).
"""
from functools import lru_cache

import numpy as np

from _mfe_np import BIG, CODE, INF, MIN_HP, PAIRS, PT, RT, Mirror, _N1, _N2


def enumerate_dimer(seq, c):
    L = len(seq)
    ok = [[(seq[i] + seq[j]) in PAIRS and (i < c <= j or j - i - 1 >= MIN_HP) for j in range(L)] for i in range(L)]

    @lru_cache(maxsize=None)
    def rec(i, j):
        """pair sets on positions i..j"""
        if j <= i:
            return ((),)
        out = list(rec(i + 1, j))
        for k in range(i + 1, j + 1):
            if ok[i][k]:
                inner, rest = rec(i + 1, k - 1), rec(k + 1, j)
                out += [((i, k),) + a + b for a in inner for b in rest]
        return tuple(out)

    rows = []
    for pairs in rec(0, L - 1):
        db = ["."] * L
        for i, j in pairs:
            db[i], db[j] = "(", ")"
        rows.append("".join(db))
    return rows


def pair_table(row):
    pt, stack = [-1] * len(row), []
    for x, ch in enumerate(row):
        if ch == "(":
            stack.append(x)
        elif ch == ")":
            y = stack.pop()
            pt[x], pt[y] = y, x
    assert not stack
    return pt


def branches(pt, a, b):
    """the pairs (p, q) directly inside a..b"""
    out, p = [], a
    while p <= b:
        if pt[p] > p:
            out.append((p, pt[p]))
            p = pt[p] + 1
        else:
            p += 1
    return out


def dimer_energy(mirror, seq, c, row, duplex_init):
    L = len(seq)
    S = np.array([CODE[ch] for ch in seq], dtype=np.int64)
    pt = pair_table(row)
    sc = mirror.sc
    x = lambda i, j: i < c <= j
    n5 = lambda p: int(S[p - 1]) if p > 0 and p != c else -1        # a neighbour across a strand end does not exist
    n3 = lambda q: int(S[q + 1]) if q < L - 1 and q + 1 != c else -1
    ext_stems = lambda br: sum(mirror.stem(int(PT[S[p], S[q]]), n5(p), n3(q), True) for p, q in br)
    e = ext_stems(branches(pt, 0, L - 1))
    if any(x(i, j) for i, j in enumerate(pt) if j > i):
        e += duplex_init
    for i, j in enumerate(pt):
        if j < i:
            continue
        t, br = int(PT[S[i], S[j]]), branches(pt, i + 1, j - 1)
        assert t
        if x(i, j) and not any(x(p, q) for p, q in br):             # the loop that holds the nick
            e += mirror.stem(int(RT[t]), int(S[j - 1]) if j != c else -1, int(S[i + 1]) if i + 1 != c else -1, True) + ext_stems(br)
        elif not br:
            assert j - i - 1 >= MIN_HP
            e += mirror.hairpin(seq, S, i, j)
        elif len(br) == 1:
            (p, q), = br
            e += int(mirror.interior(p - i - 1, j - q - 1, t, int(RT[PT[S[p], S[q]]]), S[i + 1], S[j - 1], S[p - 1], S[q + 1]))
        else:
            u = j - i - 1 - sum(q - p + 1 for p, q in br)
            e += sc["ml_closing"] + u * sc["ml_base"] + mirror.stem(int(RT[t]), int(S[j - 1]), int(S[i + 1]), False)
            e += sum(mirror.stem(int(PT[S[p], S[q]]), int(S[p - 1]), int(S[q + 1]), False) for p, q in br)
    return int(e)


def multiloop_with_cross_branch(row, c):
    """whether a real multiloop of the row (two branches or more, the nick not in it) has a branch that spans the nick"""
    pt = pair_table(row)
    for i, j in enumerate(pt):
        if j > i:
            br = branches(pt, i + 1, j - 1)
            if len(br) >= 2 and any(p < c <= q for p, q in br):
                return True
    return False


TIE_KINDS = ("F", "FA", "FB", "M", "M1", "C_intra", "C_cross")
TIE_NICK = ("C_cross_nick_interior", "C_cross_nick_split")


class CutMirror(Mirror):
    def __init__(self, tables, duplex_init, defect=None):
        super().__init__(tables)
        assert defect in (None, "split_k", "branch_start", "fa_two_rounds", "fb_two_rounds")
        self.dinit = int(duplex_init)
        self.defect = defect
        self.ties = dict.fromkeys(TIE_KINDS + TIE_NICK, 0)
        self._cut_filled = {}

    def _stem_ext(self, S, c, i, j):
        L = len(S)
        s5 = int(S[i - 1]) if i > 0 and i != c else -1
        s3 = int(S[j + 1]) if j < L - 1 and j + 1 != c else -1
        return self.stem(int(PT[S[i], S[j]]), s5, s3, True) + (self.dinit if i < c <= j else 0)

    def _nick(self, S, c, G, i, j, t):
        return self.stem(int(RT[t]), int(S[j - 1]) if j != c else -1, int(S[i + 1]) if i + 1 != c else -1, True) + G[i + 1] + G[j]

    def _interior(self, S, C, c, i, j):
        """interior-loop candidate x of the cell (i,j): inside a cross pair only a cross pair leaves a real loop"""
        L = len(S)
        t = int(PT[S[i], S[j]])
        p, q = i + 1 + _N1, j - 1 - _N2
        good = ((p < c) & (c <= q) if i < c <= j else (q - p >= MIN_HP + 1)) & (t > 0)
        pc, qc = np.where(good, p, 1), np.where(good, q, 1)
        t2 = PT[S[pc], S[qc]]
        inner = C[pc, qc]
        good &= (t2 > 0) & (inner < BIG)
        e = self.interior(_N1, _N2, t, RT[t2], S[i + 1], S[j - 1], S[pc - 1], S[np.minimum(qc + 1, L - 1)])
        return np.where(good, e + inner, INF)

    def _bonds(self, k, c):
        """which of the positions k have the bond before them"""
        return np.ones(len(k), dtype=bool) if self.defect in ("split_k", "branch_start") else k != c

    def _cell(self, seq, S, c, C, M, M1, G, a, b):
        L, sc = len(S), self.sc
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        cross = a < c <= b
        if b - a < MIN_HP + 1 and not cross:
            return
        t = int(PT[S[a], S[b]])
        if t:
            best = self._nick(S, c, G, a, b, t) if cross else self.hairpin(seq, S, a, b)
            best = min(best, int(self._interior(S, C, c, a, b).min()))
            if b - a >= 3 and a + 1 != c and b != c:
                k = np.arange(a + 2, b)
                ml = np.where(self._bonds(k, c), M[a + 1, k - 1] + M1[k, b - 1], INF).min()
                if ml < BIG:
                    best = min(best, int(ml) + sc["ml_closing"] + self.stem(int(RT[t]), int(S[b - 1]), int(S[a + 1]), False))
            if best < BIG:
                C[a, b] = best
        m1 = INF
        if C[a, b] < BIG and (a != c or self.defect == "branch_start") and b + 1 != c:
            m1 = int(C[a, b]) + self.stem(t, nb(a - 1), nb(b + 1), False)
        if M1[a, b - 1] < BIG and b != c:
            m1 = min(m1, int(M1[a, b - 1]) + sc["ml_base"])
        M1[a, b] = m1
        m = m1
        if M[a + 1, b] < BIG and a + 1 != c:
            m = min(m, int(M[a + 1, b]) + sc["ml_base"])
        k = np.arange(a + 1, b + 1)
        sp = int(np.where(self._bonds(k, c), M[a, k - 1] + M1[k, b], INF).min())
        M[a, b] = min(m, sp if sp < BIG else INF)

    def fill_cut(self, seq, c):
        """(S, C, M, M1, F, G): the tables in the three phases of section 22; G[i] = FA[i] for i < c, G[j + 1] = FB[j] for j >= c"""
        L = len(seq)
        assert 0 < c < L
        S = np.array([CODE[ch] for ch in seq], dtype=np.int64)
        C = np.full((L + 1, L + 1), INF, dtype=np.int64)
        M, M1 = C.copy(), C.copy()
        G = [0] * (L + 1)
        for d in range(MIN_HP + 1, max(c, L - c)):
            for a in range(0, L - d):
                if not a < c <= a + d:
                    self._cell(seq, S, c, C, M, M1, G, a, a + d)
        fb_end = c + 2 * 64 if self.defect == "fb_two_rounds" else L           # the candidates a loop of two rounds of 64 reaches
        fa_len = 2 * 64 if self.defect == "fa_two_rounds" else L
        for j in range(c, L):
            G[j + 1] = min([G[j]] + [G[i] + int(C[i, j]) + self._stem_ext(S, c, i, j) for i in range(c, min(j - MIN_HP, fb_end)) if C[i, j] < BIG])
        for i in range(c - 1, -1, -1):
            G[i] = min([G[i + 1]] + [int(C[i, j]) + self._stem_ext(S, c, i, j) + G[j + 1] for j in range(i + MIN_HP + 1, min(c, i + MIN_HP + 1 + fa_len))
                                     if C[i, j] < BIG])
        for d in range(1, L):
            for a in range(max(0, c - d), min(c, L - d)):
                self._cell(seq, S, c, C, M, M1, G, a, a + d)
        F = [0] * (L + 1)
        for j in range(L):
            F[j + 1] = min([F[j]] + [F[i] + int(C[i, j]) + self._stem_ext(S, c, i, j) for i in range(0, j) if C[i, j] < BIG])
        return S, C, M, M1, F, G

    def mfe_cut(self, seq, c):
        return self.fill_cut(seq, c)[4][len(seq)] if c else self.mfe(seq)

    def fold_cut(self, seq, c, order="first"):
        """(dcal, row, n_inter): the tables of fill_cut traced back as section 22 says - cross C: the nick loop, the interior loops
        (p ascending, then q descending), the splits (k ascending); FB as F: j unpaired, the stems with i ascending from c; FA: i
        unpaired, the stems (i,j) with j ascending; M, M1 and F as `Mirror.fold` - taking the first reproducing candidate, or the
        last one"""
        assert order in ("first", "last")
        if not c:
            dcal, row = self.fold(seq, order)
            return dcal, row, 0
        ties = self.ties = dict.fromkeys(TIE_KINDS + TIE_NICK, 0)
        take = (lambda hits: hits[0]) if order == "first" else (lambda hits: hits[-1])

        def pick(hits, kind):
            ties[kind] += len(hits) > 1
            return take(hits)
        L, sc = len(seq), self.sc
        if (seq, c) not in self._cut_filled:
            self._cut_filled[seq, c] = self.fill_cut(seq, c)
        S, C, M, M1, F, G = self._cut_filled[seq, c]
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        ext = lambda i, j: int(C[i, j]) + self._stem_ext(S, c, i, j)
        mlb = sc["ml_base"]
        stack, pt = [], [-1] * L
        j = L - 1
        while j >= 1:
            v = F[j + 1]
            hits = ([-1] if v == F[j] else []) + [i for i in range(0, j) if C[i, j] < BIG and F[i] + ext(i, j) == v]
            i = pick(hits, "F")
            if i < 0:
                j -= 1
                continue
            stack.append((i, j, "C"))
            j = i - 1
        while stack:
            i, j, kind = stack.pop()
            if kind == "FA":
                while i <= j:
                    hits = ([-1] if G[i] == G[i + 1] else []) + [y for y in range(i + MIN_HP + 1, j + 1) if C[i, y] < BIG and ext(i, y) + G[y + 1] == G[i]]
                    y = pick(hits, "FA")
                    if y < 0:
                        i += 1
                        continue
                    stack.append((i, y, "C"))
                    i = y + 1
                continue
            if kind == "FB":
                while j >= i:
                    hits = ([-1] if G[j + 1] == G[j] else []) + [y for y in range(i, j - MIN_HP) if C[y, j] < BIG and G[y] + ext(y, j) == G[j + 1]]
                    y = pick(hits, "FB")
                    if y < 0:
                        j -= 1
                        continue
                    stack.append((y, j, "C"))
                    j = y - 1
                continue
            if kind == "M":
                while True:
                    v = int(M[i, j])
                    assert v < BIG
                    hits = [("M1", 0)] if M1[i, j] == v else []
                    if j > i and M[i + 1, j] < BIG and i + 1 != c and int(M[i + 1, j]) + mlb == v:
                        hits.append(("skip", 0))
                    k = np.arange(i + 1, j + 1)
                    a, b = M[i, k - 1], M1[k, j]
                    hits += [("split", int(x)) for x in k[(a < BIG) & (b < BIG) & (k != c) & (a + b == v)]]
                    what, k = pick(hits, "M")
                    if what == "skip":
                        i += 1
                        continue
                    if what == "split":
                        stack.append((i, k - 1, "M"))
                        i = k
                    break
                kind = "M1"
            if kind == "M1":
                while True:
                    v = int(M1[i, j])
                    assert v < BIG
                    hits = []
                    if C[i, j] < BIG and i != c and j + 1 != c and int(C[i, j]) + self.stem(int(PT[S[i], S[j]]), nb(i - 1), nb(j + 1), False) == v:
                        hits.append("C")
                    if j > i and M1[i, j - 1] < BIG and j != c and int(M1[i, j - 1]) + mlb == v:
                        hits.append("skip")
                    if pick(hits, "M1") == "C":
                        break
                    j -= 1
            pt[i], pt[j] = j, i
            v, t = int(C[i, j]), int(PT[S[i], S[j]])
            assert t and v < BIG
            cross = i < c <= j
            if cross:
                hits = [("nick", 0)] if self._nick(S, c, G, i, j, t) == v else []
            else:
                hits = [("hairpin", 0)] if self.hairpin(seq, S, i, j) == v else []
            hits += [("interior", int(x)) for x in np.nonzero(self._interior(S, C, c, i, j) == v)[0]]
            if j - i >= 3 and i + 1 != c and j != c:
                k = np.arange(i + 2, j)
                close = sc["ml_closing"] + self.stem(int(RT[t]), int(S[j - 1]), int(S[i + 1]), False)
                a, b = M[i + 1, k - 1], M1[k, j - 1]
                hits += [("split", int(x)) for x in k[(a < BIG) & (b < BIG) & (k != c) & (a + b + close == v)]]
            what, x = pick(hits, "C_cross" if cross else "C_intra")
            if cross and len(hits) > 1 and hits[0][0] == "nick":
                ties["C_cross_nick_interior"] += any(h[0] == "interior" for h in hits)
                ties["C_cross_nick_split"] += any(h[0] == "split" for h in hits)
            if what == "nick":
                if i + 1 < c:
                    stack.append((i + 1, c - 1, "FA"))
                if j > c:
                    stack.append((c, j - 1, "FB"))
            elif what == "interior":
                stack.append((i + 1 + int(_N1[x]), j - 1 - int(_N2[x]), "C"))
            elif what == "split":
                stack.append((i + 1, x - 1, "M"))
                stack.append((x, j - 1, "M1"))
        row = "".join("." if y < 0 else "(" if y > x else ")" for x, y in enumerate(pt))
        return F[L], row, sum(1 for x, y in enumerate(pt) if x < c <= y)


# the 8-nt hairpins below 0 under the built-in tables (two pairs over a special tetraloop): what a strand of at most 8 nt needs for a
# disconnected optimum below 0
STABLE_HAIRPINS = ("GCCUCGGC", "CCCUCGGG", "GCUCCGGC", "CCUCCGGG", "GCUACGGC", "GCUGCGGC", "CCUACGGG", "CCUGCGGG")


def draw_dimers(seed, n, n_hairpin=0, n_two=0):
    """n dimers (seq, c) with strands of 3-8 nt and at most 14 nt in all, G/C/U-rich so that pairs exist; the last n_hairpin of them
    hold one of STABLE_HAIRPINS as one strand, on either side, beside an A/C-rich strand of 3-6 nt; the n_two before them are
    x H u | H x' with x-x' and the ends of both 5-nt H able to pair: two hairpins in the loop with the nick, the second one
    beginning at c - what a recurrence that forgets the nick takes for a multiloop"""
    rng = np.random.default_rng(seed)
    out = []
    pair = lambda: ("GC", "CG", "GU", "UG", "AU", "UA")[int(rng.integers(6))]
    hair = lambda: (lambda p: p[0] + "".join(rng.choice(list("ACGU"), 3)) + p[1])(pair())
    while len(out) < n - n_hairpin - n_two:
        la, lb = (int(v) for v in rng.integers(3, 9, size=2))
        if la + lb > 14:
            continue
        out.append(("".join(rng.choice(list("GCUA"), la + lb, p=[0.35, 0.3, 0.25, 0.1])), la))
    while len(out) < n - n_hairpin:
        x = pair()
        out.append((x[0] + hair() + "ACGU"[int(rng.integers(4))] + hair() + x[1], 7))
    while len(out) < n:
        hp = STABLE_HAIRPINS[int(rng.integers(len(STABLE_HAIRPINS)))]
        other = "".join(rng.choice(list("ACU"), int(rng.integers(3, 7)), p=[0.6, 0.3, 0.1]))
        out.append((hp + other, 8) if rng.integers(2) else (other + hp, len(other)))
    return out
