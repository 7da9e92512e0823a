"""Minimum free energy, twice, for the tests of rafft_mfe_batch (test infrastructure; pure Python / numpy: no GPU, no product code).

* `enumerate_structures(seq)`: every secondary structure of a sequence as a dot-bracket string - canonical pairs (CG GC GU UG AU UA),
  hairpins of at least 3, nothing else forbidden (lonely pairs, interior loops of any size).  A 20-nt random sequence has at most
  a few thousand, "G" * 10 + "U" * 10 has 51 766.
* `Mirror(tables)`: a plain restatement of the recurrences of DESIGN.md section 9 over the tables tests/_par_reader.py reads (the
  dict `tables_at` returns - the source tests/_loops.py uses), with the loop energies written out again here:
      C[i][j]  = min(hairpin, min over inner pairs (p,q) with n1 + n2 <= 30 of interior + C[p][q],
                     ml_closing + stem(closing pair, read from inside) + min_k M[i+1][k-1] + M1[k][j-1])
      M1[i][j] = min(C[i][j] + stem(i,j), M1[i][j-1] + ml_base)
      M[i][j]  = min(M1[i][j], M[i+1][j] + ml_base, min_k M[i][k-1] + M1[k][j])
      F[j]     = min(F[j-1], min_i F[i-1] + C[i][j] + exterior stem(i,j)),  MFE = F[L-1]
  `Mirror.mfe(seq)` is the energy in dcal.  The interior-loop candidates of a whole anti-diagonal are evaluated as one numpy
  expression, so a 90-nt sequence takes a fraction of a second.
  `Mirror.fold(seq, order)` is `(dcal, row)`: the same tables traced back in the candidate order section 9 documents ("first"), or
  with the last reproducing candidate of every cell ("last").
"""
import math
from functools import lru_cache

import numpy as np

CODE = {c: i for i, c in enumerate("NACGU")}
PAIRS = {"CG": 1, "GC": 2, "GU": 3, "UG": 4, "AU": 5, "UA": 6}
PT = np.zeros((5, 5), dtype=np.int64)
for _k, _v in PAIRS.items():
    PT[CODE[_k[0]], CODE[_k[1]]] = _v
RT = np.array([0, 2, 1, 4, 3, 6, 5], dtype=np.int64)
INF = 10 ** 9
BIG = INF // 2          # every real energy lies below, every sum with an INF above
MAXLOOP = 30
MIN_HP = 3


# ---------------------------------------------------------------- (a) enumeration

def enumerate_structures(seq):
    L = len(seq)
    ok = [[(seq[i] + seq[j]) in PAIRS for j in range(L)] for i in range(L)]

    @lru_cache(maxsize=None)
    def rec(i, j):
        """pair sets on positions i..j"""
        if j - i < MIN_HP + 1:
            return ((),)
        out = list(rec(i + 1, j))
        for k in range(i + MIN_HP + 1, j + 1):
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


# ---------------------------------------------------------------- (b) the recurrences

_N1, _N2 = np.array([(a, b) for a in range(MAXLOOP + 1) for b in range(MAXLOOP + 1 - a)], dtype=np.int64).T


class Mirror:
    def __init__(self, tables):
        self.T = tables
        self.sc = tables["scalars"]
        self.special = {s: e for ent in tables["special"].values() for s, e in reversed(ent)}     # (the first entry of a table wins)
        self._filled = {}                       # fill() of the sequences fold() was asked for: "first" and "last" share the tables

    def hairpin(self, seq, S, i, j):
        n, t = j - i - 1, PT[S[i], S[j]]
        if n in (3, 4, 6) and seq[i:j + 1] in self.special:
            return self.special[seq[i:j + 1]]
        e = int(self.T["hairpin"][min(n, 30)])
        if n > 30:
            e += int(self.sc["lxc"] * math.log(n / 30.))
        if n == 3:
            return e + (self.sc["term_au"] if t > 2 else 0)
        return e + int(self.T["mismatch_hairpin"][t, S[i + 1], S[j - 1]])

    def interior(self, n1, n2, t, u, si1, sj1, sp1, sq1):
        """loop between a pair of type t and an inner pair whose type read from the other side is u; n1 / n2 unpaired on the 5' / 3'
        strand; si1, sj1 the bases inside the outer pair, sp1, sq1 those outside the inner pair.  Arrays, broadcast."""
        T, sc = self.T, self.sc
        nl, ns = np.maximum(n1, n2), np.minimum(n1, n2)
        size = np.minimum(nl + ns, 30)
        stack = T["stack"][t, u]
        au = np.where(t > 2, sc["term_au"], 0) + np.where(u > 2, sc["term_au"], 0)
        bulge = T["bulge"][size] + np.where(nl == 1, stack, au)
        i11 = T["int11"][t, u, si1, sj1]
        i21 = np.where(n1 == 1, T["int21"][t, u, si1, sq1, sj1], T["int21"][u, t, sq1, si1, sp1])
        i22 = T["int22"][t, u, si1, sp1, sq1, sj1]
        c23 = (ns == 2) & (nl == 3)
        name = lambda k: T[k][t, si1, sj1] + T[k][u, sq1, sp1]
        mm = np.where(ns == 1, name("mismatch_interior_1n"), np.where(c23, name("mismatch_interior_23"), name("mismatch_interior")))
        ninio = np.where(c23, sc["ninio"], np.minimum(sc["max_ninio"], (nl - ns) * sc["ninio"]))
        generic = T["interior"][size] + ninio + mm
        return np.where(nl == 0, stack, np.where(ns == 0, bulge, np.where(nl == 1, i11, np.where(nl > 2, generic, np.where(ns == 2, i22, i21)))))

    def stem(self, t, s5, s3, ext):
        """a stem of type t in the exterior loop or a multiloop; s5 / s3: the base before its 5' / after its 3' end, -1 = none"""
        T = self.T
        e = 0
        if s5 >= 0 and s3 >= 0:
            e += int(T["mismatch_exterior" if ext else "mismatch_multi"][t, s5, s3])
        elif s5 >= 0:
            e += int(T["dangle5"][t, s5])
        elif s3 >= 0:
            e += int(T["dangle3"][t, s3])
        if t > 2:
            e += self.sc["term_au"]
        return e if ext else e + self.sc["ml_intern"]

    def interior_candidates(self, S, C, i, j):
        """interior-loop candidate x = (n1, n2) of the cells (i[a], j[a]): its energy with C[p][q], INF where there is no such loop.
        Rows = cells, columns = candidates with n1 ascending, then n2 ascending: p ascending, then q descending."""
        L = len(S)
        t = PT[S[i], S[j]]
        p, q = i[:, None] + 1 + _N1[None, :], j[:, None] - 1 - _N2[None, :]
        good = (q - p >= MIN_HP + 1) & (t[:, None] > 0)
        pc, qc = np.where(good, p, 1), np.where(good, q, 1)
        t2 = PT[S[pc], S[qc]]
        inner = C[pc, qc]
        good &= (t2 > 0) & (inner < BIG)
        e = self.interior(_N1[None, :], _N2[None, :], t[:, None], RT[t2], S[i + 1][:, None], S[j - 1][:, None], S[pc - 1], S[np.minimum(qc + 1, L - 1)])
        return np.where(good, e + inner, INF)

    def fill(self, seq):
        """(S, C, M, M1, F): the three tables, (L + 1) x (L + 1) with INF where there is no structure, and F[j + 1] of positions 0..j"""
        L = len(seq)
        S = np.array([CODE[c] for c in seq], dtype=np.int64)
        sc = self.sc
        C = np.full((L + 1, L + 1), INF, dtype=np.int64)
        M, M1 = C.copy(), C.copy()
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        for d in range(MIN_HP + 1, L):
            i = np.arange(0, L - d)
            j = i + d
            t = PT[S[i], S[j]]
            best_int = self.interior_candidates(S, C, i, j).min(axis=1)
            for a in range(L - d):
                b = a + d
                if t[a]:
                    c = min(self.hairpin(seq, S, a, b), int(best_int[a]))
                    if d >= 2 * (MIN_HP + 2) + 1:
                        k = np.arange(a + 2, b)
                        ml = int((M[a + 1, k - 1] + M1[k, b - 1]).min())
                        if ml < BIG:
                            c = min(c, ml + sc["ml_closing"] + self.stem(int(RT[t[a]]), int(S[b - 1]), int(S[a + 1]), False))
                    C[a, b] = c
                m1 = int(M1[a, b - 1]) + sc["ml_base"] if M1[a, b - 1] < INF else INF
                if C[a, b] < INF:
                    m1 = min(m1, int(C[a, b]) + self.stem(int(t[a]), nb(a - 1), nb(b + 1), False))
                M1[a, b] = m1
                m = min(m1, int(M[a + 1, b]) + sc["ml_base"] if M[a + 1, b] < INF else INF)
                k = np.arange(a + 1, b + 1)
                sp = int((M[a, k - 1] + M1[k, b]).min())
                M[a, b] = min(m, sp if sp < BIG else INF)
        F = [0] * (L + 1)                       # F[j + 1]: positions 0..j
        for j in range(L):
            best = F[j]
            for i in range(0, j - MIN_HP):
                if C[i, j] < INF:
                    best = min(best, F[i] + int(C[i, j]) + self.stem(int(PT[S[i], S[j]]), nb(i - 1), nb(j + 1), True))
            F[j + 1] = best
        return S, C, M, M1, F

    def mfe(self, seq):
        return self.fill(seq)[4][len(seq)]

    def fold(self, seq, order="first"):
        """(dcal, row): the tables of `fill`, traced back as DESIGN.md section 9 says.  A cell's candidates are visited in the documented
        order - C: the hairpin, the interior loops (p ascending, then q descending), the multiloop splits (k ascending); M1: the stem,
        j unpaired; M: M1, i unpaired, the splits (k ascending); F: j unpaired, the stems (i ascending) - a term is a candidate only
        if its parts are below BIG, and the FIRST candidate that reproduces the stored value is taken.  order="last" takes the last
        one instead: another co-optimal structure wherever a cell ties, there to show that an input discriminates.
        `self.offsets` then holds, per kind of multi-candidate choice, the largest candidate offset that was taken: "F" the 5' end i
        of an exterior stem, "M" k - (i + 5) of an M split, "C" k - (i + 6) of a C split, "I" the number x of an interior loop."""
        assert order in ("first", "last")
        pick = (lambda hits: hits[0]) if order == "first" else (lambda hits: hits[-1])
        L, sc = len(seq), self.sc
        if seq not in self._filled:
            self._filled[seq] = self.fill(seq)
        S, C, M, M1, F = self._filled[seq]
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        mlb = sc["ml_base"]
        off = self.offsets = dict(F=-1, M=-1, C=-1, I=-1)
        note = lambda key, x: off.__setitem__(key, max(off[key], int(x)))
        stack, pt = [], [-1] * L
        j = L - 1
        while j >= MIN_HP + 1:
            v = F[j + 1]
            hits = [-1] if v == F[j] else []
            for i in range(0, j - MIN_HP):
                if C[i, j] < BIG and F[i] + int(C[i, j]) + self.stem(int(PT[S[i], S[j]]), nb(i - 1), nb(j + 1), True) == v:
                    hits.append(i)
            i = pick(hits)
            if i < 0:
                j -= 1
                continue
            note("F", i)
            stack.append((i, j, "C"))
            j = i - 1
        while stack:
            i, j, kind = stack.pop()
            if kind == "M":
                while True:
                    v = int(M[i, j])
                    assert v < BIG
                    hits = [("M1", 0)] if M1[i, j] == v else []
                    if j > i and M[i + 1, j] < BIG and int(M[i + 1, j]) + mlb == v:
                        hits.append(("skip", 0))
                    k = np.arange(i + MIN_HP + 2, j - MIN_HP)
                    if len(k):
                        a, b = M[i, k - 1], M1[k, j]
                        hits += [("split", int(x)) for x in k[(a < BIG) & (b < BIG) & (a + b == v)]]
                    what, k = pick(hits)
                    if what == "skip":
                        i += 1
                        continue
                    if what == "split":
                        note("M", k - (i + MIN_HP + 2))
                        stack.append((i, k - 1, "M"))
                        i = k
                    break
                kind = "M1"
            if kind == "M1":
                while True:
                    v = int(M1[i, j])
                    assert v < BIG
                    hits = []
                    if C[i, j] < BIG and int(C[i, j]) + self.stem(int(PT[S[i], S[j]]), nb(i - 1), nb(j + 1), False) == v:
                        hits.append("C")
                    if j > i and M1[i, j - 1] < BIG and int(M1[i, j - 1]) + mlb == v:
                        hits.append("skip")
                    if pick(hits) == "C":
                        break
                    j -= 1
            pt[i], pt[j] = j, i
            v, t = int(C[i, j]), int(PT[S[i], S[j]])
            assert t and v < BIG
            hits = [("hairpin", 0)] if self.hairpin(seq, S, i, j) == v else []
            il = self.interior_candidates(S, C, np.array([i]), np.array([j]))[0]
            hits += [("interior", int(x)) for x in np.nonzero(il == v)[0]]
            k = np.arange(i + MIN_HP + 3, j - MIN_HP - 1)
            if len(k):
                close = sc["ml_closing"] + self.stem(int(RT[t]), int(S[j - 1]), int(S[i + 1]), False)
                a, b = M[i + 1, k - 1], M1[k, j - 1]
                hits += [("split", int(x)) for x in k[(a < BIG) & (b < BIG) & (a + b + close == v)]]
            what, x = pick(hits)
            if what == "interior":
                note("I", x)
                stack.append((i + 1 + int(_N1[x]), j - 1 - int(_N2[x]), "C"))
            elif what == "split":
                note("C", x - (i + MIN_HP + 3))
                stack.append((i + 1, x - 1, "M"))
                stack.append((x, j - 1, "M1"))
        return F[L], "".join("." if y < 0 else "(" if y > x else ")" for x, y in enumerate(pt))
