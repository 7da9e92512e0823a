"""Constrained minimum free energy for the tests of rafft_mfe_constrained_batch (test infrastructure; pure Python / numpy: no GPU,
no product code).  DESIGN.md section 20.

* `satisfies(row, con)`: the row obeys every character of the constraint string (. x | < > ( )).
* `pseudo(row, u, b)`: the soft terms of a row - u[k] per unpaired position, b[i] + b[j] + b[i+1] + b[j-1] per pair (i,j) stacked
  directly on (i+1,j-1).
* `ConMirror(tables)`: `_mfe_np.Mirror` with the constrained recurrences:
      ok(i,j)   canonical, j - i - 1 >= 3, con[i] one of . | < or a ( whose partner is j, con[j] one of . | > or a ) whose partner is i
      C[i][j]   no structure unless ok(i,j); the hairpin only if free(i+1,j-1), plus U(i+1,j-1); an interior loop with (p,q) only if
                free(i+1,p-1) and free(q+1,j-1), plus both U terms, plus the stack term when n1 = n2 = 0; the multiloop unchanged
      M1[i][j]  = min(C[i][j] + stem, M1[i][j-1] + ml_base + u[j] if up(j))
      M[i][j]   = min(M1[i][j], M[i+1][j] + ml_base + u[i] if up(i), splits)
      F[j]      = min(F[j-1] + u[j] if up(j), stems)
  `fold(seq, con, u, b, order)` is `(dcal, row)` - `(None, None)` when no structure satisfies the constraints - traced back in the
  candidate order of section 9 ("first") or with the last reproducing candidate ("last"); `self.pseudo` is then the soft part of
  dcal that the traceback summed, `self.offsets` as Mirror's.
* `draw_constraint(rng, seq)`: a seeded constraint string; `short_sequences()` / `exhaustive_cases(seed)`: the cases the CPU test
  checks against the enumeration and the GPU test runs in one batch.
"""
from functools import lru_cache

import numpy as np

import _mfe_np as MF
from _mfe_np import BIG, INF, MIN_HP, PT, RT, _N1, _N2

CHARS, PROBS = ". x | < >".split(), (0.80, 0.08, 0.06, 0.03, 0.03)


@lru_cache(maxsize=None)
def pair_table(row):
    """partners of the ( ) of a row or of a constraint string, -1 elsewhere; a tuple"""
    pt, stk = [-1] * len(row), []
    for k, c in enumerate(row):
        if c == "(":
            stk.append(k)
        elif c == ")":
            i = stk.pop()
            pt[i], pt[k] = k, i
    assert not stk
    return tuple(pt)


def satisfies(row, con):
    if con is None:
        return True
    pt, want = pair_table(row), pair_table(con)
    for k, c in enumerate(con):
        y = pt[k]
        if (c == "x" and y >= 0) or (c == "|" and y < 0) or (c == "<" and not y > k) or (c == ">" and not 0 <= y < k) or (c in "()" and y != want[k]):
            return False
    return True


def pseudo(row, u=None, b=None):
    pt, e = pair_table(row), 0
    for k, y in enumerate(pt):
        if y < 0:
            e += int(u[k]) if u is not None else 0
        elif y > k and b is not None and y - 1 > k + 1 and pt[k + 1] == y - 1:
            e += int(b[k]) + int(b[y]) + int(b[k + 1]) + int(b[y - 1])
    return e


def draw_constraint(rng, seq):
    """per position . x | < > with probabilities 0.80 / 0.08 / 0.06 / 0.03 / 0.03; with probability 1/2 one bracket pair, drawn
    uniformly from the canonical (i,j) with j - i >= 4"""
    con = list(rng.choice(CHARS, len(seq), p=PROBS))
    if rng.random() < 0.5:
        cand = [(i, j) for i in range(len(seq)) for j in range(i + 4, len(seq)) if seq[i] + seq[j] in MF.PAIRS]
        if cand:
            i, j = cand[int(rng.integers(len(cand)))]
            con[i], con[j] = "(", ")"
    return "".join(con)


def short_sequences():
    """24 sequences of 8-20 nt, every structure of which can be enumerated"""
    rng = np.random.default_rng(2020)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 20)]
    seqs += ["".join(rng.choice(list("GCU"), n)) for n in (12, 14, 16)]
    seqs += ["GGGACACCCAGGACCACCC", "GU" * 9, "GGGUUUGGGUUUCCC", "GCGCAAAGCGCAAAGCGC", "GGGAAACCCAGGGAAACCCA", "GGNGAAACNCC", "GGGGAAAACCCC"]
    return seqs


def exhaustive_cases(seed, n_con=6, soft=False):
    """(seq, con, u, b) per case: n_con drawn constraints for every sequence of short_sequences().  soft: random u in [-150, 150]
    and b in [-200, 100] as well, and for every sequence one case more with them alone (con None)."""
    rng = np.random.default_rng(seed)
    cases = []
    for s in short_sequences():
        for _ in range(n_con):
            con = draw_constraint(rng, s)
            u = rng.integers(-150, 151, len(s)).astype(np.int32) if soft else None
            b = rng.integers(-200, 101, len(s)).astype(np.int32) if soft else None
            cases.append((s, con, u, b))
        if soft:
            cases.append((s, None, rng.integers(-150, 151, len(s)).astype(np.int32), rng.integers(-200, 101, len(s)).astype(np.int32)))
    return cases


class ConMirror(MF.Mirror):
    def _state(self, seq, con, u, b):
        L = len(seq)
        con = con if con is not None else "." * L
        assert len(con) == L
        st = type("ConState", (), {})()
        st.up = np.array([c in ".x" for c in con], dtype=bool)
        st.partner = np.array(pair_table(con), dtype=np.int64)
        st.left = np.array([c in ".|<" for c in con], dtype=bool)
        st.right = np.array([c in ".|>" for c in con], dtype=bool)
        st.must = np.concatenate([[0], np.cumsum(~st.up)]).astype(np.int64)
        st.u = np.zeros(L, dtype=np.int64) if u is None else np.asarray(u, dtype=np.int64)
        st.b = np.zeros(L, dtype=np.int64) if b is None else np.asarray(b, dtype=np.int64)
        st.usum = np.concatenate([[0], np.cumsum(st.u)]).astype(np.int64)
        return st

    def ok(self, i, j):
        st = self._st
        return bool((st.left[i] or st.partner[i] == j) and (st.right[j] or st.partner[j] == i))

    def free(self, a, b):
        return self._st.must[b + 1] == self._st.must[a]

    def U(self, a, b):
        return int(self._st.usum[b + 1] - self._st.usum[a])

    def interior_candidates(self, S, C, i, j):
        st = self._st
        base = super().interior_candidates(S, C, i, j)
        good = base < BIG
        p, q = i[:, None] + 1 + _N1[None, :], j[:, None] - 1 - _N2[None, :]
        pc, qc = np.where(good, p, 1), np.where(good, q, 1)
        i1, j0 = (i + 1)[:, None], j[:, None]
        good &= (st.must[pc] == st.must[i1]) & (st.must[j0] == st.must[qc + 1])
        soft = (st.usum[pc] - st.usum[i1]) + (st.usum[j0] - st.usum[qc + 1])
        stack = st.b[i][:, None] + st.b[j][:, None] + st.b[pc] + st.b[qc]
        soft = soft + np.where((_N1 == 0) & (_N2 == 0), stack, 0)
        return np.where(good, base + soft, INF)

    def fill(self, seq):
        st, sc = self._st, self.sc
        L = len(seq)
        S = np.array([MF.CODE[c] for c in seq], dtype=np.int64)
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
                if t[a] and self.ok(a, b):
                    c = int(best_int[a])
                    if self.free(a + 1, b - 1):
                        c = min(c, self.hairpin(seq, S, a, b) + self.U(a + 1, b - 1))
                    if d >= 2 * (MIN_HP + 2) + 1:
                        k = np.arange(a + 2, b)
                        ml = int((M[a + 1, k - 1] + M1[k, b - 1]).min())
                        if ml < BIG:
                            c = min(c, ml + sc["ml_closing"] + self.stem(int(RT[t[a]]), int(S[b - 1]), int(S[a + 1]), False))
                    C[a, b] = c if c < BIG else INF
                m1 = int(M1[a, b - 1]) + sc["ml_base"] + int(st.u[b]) if M1[a, b - 1] < BIG and st.up[b] else INF
                if C[a, b] < BIG:
                    m1 = min(m1, int(C[a, b]) + self.stem(int(t[a]), nb(a - 1), nb(b + 1), False))
                M1[a, b] = m1
                m = min(m1, int(M[a + 1, b]) + sc["ml_base"] + int(st.u[a]) if M[a + 1, b] < BIG and st.up[a] else INF)
                k = np.arange(a + 1, b + 1)
                sp = int((M[a, k - 1] + M1[k, b]).min())
                M[a, b] = min(m, sp if sp < BIG else INF)
        F = [0] * (L + 1)                       # F[j + 1]: positions 0..j
        for j in range(L):
            best = F[j] + int(st.u[j]) if F[j] < BIG and st.up[j] else INF
            for i in range(0, j - MIN_HP):
                if C[i, j] < BIG and F[i] < BIG:
                    best = min(best, F[i] + int(C[i, j]) + self.stem(int(PT[S[i], S[j]]), nb(i - 1), nb(j + 1), True))
            F[j + 1] = best
        return S, C, M, M1, F

    def mfe(self, seq, con=None, u=None, b=None):
        return self.fold(seq, con, u, b)[0]

    def fold(self, seq, con=None, u=None, b=None, order="first"):
        assert order in ("first", "last")
        pick = (lambda hits: hits[0]) if order == "first" else (lambda hits: hits[-1])
        key = (seq, con, None if u is None else tuple(int(x) for x in u), None if b is None else tuple(int(x) for x in b))
        st = self._st = self._state(seq, con, u, b)
        if key not in self._filled:
            self._filled[key] = self.fill(seq)
        S, C, M, M1, F = self._filled[key]
        L, sc = len(seq), self.sc
        self.pseudo = 0
        off = self.offsets = dict(F=-1, M=-1, C=-1, I=-1)
        if F[L] >= BIG:
            return None, None
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        mlb = sc["ml_base"]
        note = lambda key, x: off.__setitem__(key, max(off[key], int(x)))
        stack, pt, soft = [], [-1] * L, 0
        j = L - 1
        while j >= MIN_HP + 1:
            v = F[j + 1]
            hits = [-1] if F[j] < BIG and st.up[j] and v == F[j] + int(st.u[j]) else []
            for i in range(0, j - MIN_HP):
                if C[i, j] < BIG and F[i] < BIG and F[i] + int(C[i, j]) + self.stem(int(PT[S[i], S[j]]), nb(i - 1), nb(j + 1), True) == v:
                    hits.append(i)
            i = pick(hits)
            if i < 0:
                soft += int(st.u[j])
                j -= 1
                continue
            note("F", i)
            stack.append((i, j, "C"))
            j = i - 1
        if j >= 0:
            soft += self.U(0, j)
        while stack:
            i, j, kind = stack.pop()
            if kind == "M":
                while True:
                    v = int(M[i, j])
                    assert v < BIG
                    hits = [("M1", 0)] if M1[i, j] == v else []
                    if j > i and M[i + 1, j] < BIG and st.up[i] and int(M[i + 1, j]) + mlb + int(st.u[i]) == v:
                        hits.append(("skip", 0))
                    k = np.arange(i + MIN_HP + 2, j - MIN_HP)
                    if len(k):
                        a, bb = M[i, k - 1], M1[k, j]
                        hits += [("split", int(x)) for x in k[(a < BIG) & (bb < BIG) & (a + bb == v)]]
                    what, k = pick(hits)
                    if what == "skip":
                        soft += int(st.u[i])
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
                    if j > i and M1[i, j - 1] < BIG and st.up[j] and int(M1[i, j - 1]) + mlb + int(st.u[j]) == v:
                        hits.append("skip")
                    if pick(hits) == "C":
                        break
                    soft += int(st.u[j])
                    j -= 1
            pt[i], pt[j] = j, i
            v, t = int(C[i, j]), int(PT[S[i], S[j]])
            assert t and v < BIG
            hits = []
            if self.free(i + 1, j - 1) and self.hairpin(seq, S, i, j) + self.U(i + 1, j - 1) == v:
                hits.append(("hairpin", 0))
            il = self.interior_candidates(S, C, np.array([i]), np.array([j]))[0]
            hits += [("interior", int(x)) for x in np.nonzero(il == v)[0]]
            k = np.arange(i + MIN_HP + 3, j - MIN_HP - 1)
            if len(k):
                close = sc["ml_closing"] + self.stem(int(RT[t]), int(S[j - 1]), int(S[i + 1]), False)
                a, bb = M[i + 1, k - 1], M1[k, j - 1]
                hits += [("split", int(x)) for x in k[(a < BIG) & (bb < BIG) & (a + bb + close == v)]]
            what, x = pick(hits)
            if what == "hairpin":
                soft += self.U(i + 1, j - 1)
            elif what == "interior":
                note("I", x)
                p, q = i + 1 + int(_N1[x]), j - 1 - int(_N2[x])
                soft += self.U(i + 1, p - 1) + self.U(q + 1, j - 1)
                if p == i + 1 and q == j - 1:
                    soft += int(st.b[i] + st.b[j] + st.b[p] + st.b[q])
                stack.append((p, q, "C"))
            elif what == "split":
                note("C", x - (i + MIN_HP + 3))
                stack.append((i + 1, x - 1, "M"))
                stack.append((x, j - 1, "M1"))
        self.pseudo = soft
        return F[L], "".join("." if y < 0 else "(" if y > x else ")" for x, y in enumerate(pt))
