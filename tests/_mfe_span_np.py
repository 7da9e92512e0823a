"""The mirror of tests/_mfe_np.py under a maximum base-pair span, for the tests of rafft_mfe_span_batch (test infrastructure; pure
Python / numpy: no GPU, no product code).

A pair (i, j), i < j, is allowed iff j - i + 1 <= span.  `SpanMirror` is `Mirror` with that: the cells with j - i + 1 > span stay
INF, everything else is Mirror's recurrences and Mirror's traceback in the documented candidate order.  The exterior stems that end
at j are visited with i ascending from max(0, j - span + 1); the cells before that window are INF, so Mirror's loop from 0 meets the
same first candidate.  `rows_within(rows, span)` filters an enumeration to the structures that obey the span.
"""
import numpy as np

from _mfe_np import BIG, CODE, INF, MIN_HP, PT, RT, Mirror


def pairs_of(row):
    """(i, j), i < j, of a dot-bracket row"""
    stack, out = [], []
    for x, c in enumerate(row):
        if c == "(":
            stack.append(x)
        elif c == ")":
            out.append((stack.pop(), x))
    assert not stack
    return out


def obeys(row, span):
    return all(j - i + 1 <= span for i, j in pairs_of(row))


def rows_within(rows, span):
    return [r for r in rows if obeys(r, span)]


class SpanMirror(Mirror):
    def __init__(self, tables):
        super().__init__(tables)
        self.span = None
        self._by_span = {}

    def fill(self, seq):
        """Mirror.fill with the anti-diagonals d = j - i of span - 1 at most; the others stay INF"""
        span = self.span
        L = len(seq)
        S = np.array([CODE[c] for c in seq], dtype=np.int64)
        sc = self.sc
        C = np.full((L + 1, L + 1), INF, dtype=np.int64)
        M, M1 = C.copy(), C.copy()
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        for d in range(MIN_HP + 1, min(L, span)):
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
        F = [0] * (L + 1)                       # F[j + 1]: positions 0..j; the exterior loop is not restricted
        for j in range(L):
            best = F[j]
            for i in range(max(0, j - span + 1), j - MIN_HP):
                if C[i, j] < INF:
                    best = min(best, F[i] + int(C[i, j]) + self.stem(int(PT[S[i], S[j]]), nb(i - 1), nb(j + 1), True))
            F[j + 1] = best
        return S, C, M, M1, F

    def fold(self, seq, span, order="first"):
        """(dcal, row) under `span`, traced back as Mirror.fold does.  Besides `self.offsets` (Mirror's), `self.window_offset` holds
        the largest i - max(0, j - span + 1) of an exterior stem (i, j) taken in a window that does not start at 0, -1: none."""
        assert span >= 1
        self.span = span
        self._filled = self._by_span.setdefault(span, {})
        dcal, row = super().fold(seq, order)
        assert obeys(row, span)
        self.window_offset = -1
        open_at = []
        for x, c in enumerate(row):
            if c == "(":
                open_at.append(x)
            elif c == ")":
                i = open_at.pop()
                if not open_at and x - span + 1 > 0:         # an exterior stem
                    self.window_offset = max(self.window_offset, i - (x - span + 1))
        return dcal, row

    def mfe(self, seq, span):
        self.span = span
        return self.fill(seq)[4][len(seq)]
