"""The mirror of tests/_pf_np.py under a maximum base-pair span, for the tests of rafft_pf_span_batch (test infrastructure; pure
Python / numpy: no GPU, no product code).

A pair (i, j), i < j, is allowed iff j - i + 1 <= span.  `PfSpanMirror` is `PfMirror` with that: the anti-diagonals d = j - i >= span
of all six tables stay 0, the exterior windows start at max(0, j - span + 1) (and end at min(L - 1, i + span - 1) from the 3' end),
the outside sums run over enclosing cells with q - p < span only; everything else is PfMirror's recurrences over Mirror's loop
energies, unscaled fp64.  `run` also returns unpaired[i] = 1 - sum_j P(i,j) - sum_h P(h,i), clamped to [0, 1].
`rows_within` / `obeys` (tests/_mfe_span_np.py) filter an enumeration to the structures that obey the span.
"""
import numpy as np

from _mfe_np import MIN_HP, PT, RT, _N1, _N2, CODE
from _mfe_span_np import obeys, rows_within     # noqa: F401
from _pf_np import PfMirror


def unpaired_of(P):
    """1 - the share of the structures in which position i is paired, from an L x L array with P[i][j], i < j"""
    return np.clip(1.0 - P.sum(axis=1) - P.sum(axis=0), 0.0, 1.0)


def dense_to_band(P, W):
    """the (L, W) banded array of an L x L one: P[i][i + d] at [i][d]"""
    L = P.shape[0]
    band = np.zeros((L, W))
    for d in range(min(W, L)):
        band[:L - d, d] = P[np.arange(L - d), np.arange(d, L)]
    return band


class PfSpanMirror(PfMirror):
    def __init__(self, tables, span, temp=37.0):
        super().__init__(tables, temp)
        assert span >= 1
        self.span = span

    def inside(self, seq):
        m, sc, w, span = self.m, self.sc, self.w, self.span
        L = self.L = len(seq)
        S = self.S = np.array([CODE[c] for c in seq], dtype=np.int64)
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        b = w(sc["ml_base"])
        bp = self.bp = b ** np.arange(L + 1, dtype=np.float64)
        C, M, M1 = (np.zeros((L + 1, L + 1)) for _ in range(3))
        WM, WE, WC = (np.zeros((L + 1, L + 1)) for _ in range(3))
        for i in range(L):
            for j in range(i + MIN_HP + 1, min(L, i + span)):
                t = int(PT[S[i], S[j]])
                if t:
                    WM[i, j] = w(m.stem(t, nb(i - 1), nb(j + 1), False))
                    WE[i, j] = w(m.stem(t, nb(i - 1), nb(j + 1), True))
                    WC[i, j] = w(sc["ml_closing"] + m.stem(int(RT[t]), int(S[j - 1]), int(S[i + 1]), False))
        for d in range(MIN_HP + 1, min(L, span)):           # anti-diagonals >= span stay 0
            i = np.arange(0, L - d)
            j = i + d
            t = PT[S[i], S[j]]
            p, q = i[:, None] + 1 + _N1[None, :], j[:, None] - 1 - _N2[None, :]
            good = (q - p >= MIN_HP + 1) & (t[:, None] > 0)
            pc, qc = np.where(good, p, 1), np.where(good, q, 1)
            t2 = PT[S[pc], S[qc]]
            good &= t2 > 0
            e = m.interior(_N1[None, :], _N2[None, :], t[:, None], RT[t2], S[i + 1][:, None], S[j - 1][:, None], S[pc - 1], S[np.minimum(qc + 1, L - 1)])
            il = np.where(good, np.exp(-e * self.beta) * C[pc, qc], 0.0).sum(axis=1)
            for a in range(L - d):
                z = a + d
                if t[a]:
                    c = w(m.hairpin(seq, S, a, z)) + float(il[a])
                    k = np.arange(a + 6, z - 4)
                    if len(k):
                        c += WC[a, z] * float(M[a + 1, k - 1] @ M1[k, z - 1])
                    C[a, z] = c
                M1[a, z] = C[a, z] * WM[a, z] + M1[a, z - 1] * b
                k = np.arange(a, z - 3)
                M[a, z] = float((bp[k - a] + M[a, k - 1]) @ M1[k, z])
        F = np.zeros(L + 1)
        F[0] = 1.0
        for j in range(L):
            i = np.arange(max(0, j - span + 1), max(j - MIN_HP, 0))
            F[j + 1] = F[j] + float((F[i] * C[i, j]) @ WE[i, j])
        Fr = np.zeros(L + 2)
        Fr[L] = 1.0
        for i in range(L - 1, -1, -1):
            j = np.arange(i + MIN_HP + 1, min(L, i + span))
            Fr[i] = Fr[i + 1] + float((C[i, j] * WE[i, j]) @ Fr[j + 1])
        self.C, self.M, self.M1, self.F, self.Fr, self.WM, self.WE, self.WC, self.b = C, M, M1, F, Fr, WM, WE, WC, b
        return float(F[L])

    def run(self, seq):
        """(Z, P, unpaired): the partition function under the span, the L x L array of pair probabilities, the L unpaired ones"""
        Z = self.inside(seq)
        L, S, m, span = self.L, self.S, self.m, self.span
        C, M, M1, F, Fr, WM, WE, WC, b, bp = self.C, self.M, self.M1, self.F, self.Fr, self.WM, self.WE, self.WC, self.b, self.bp
        Co, Mo, M1o = (np.zeros((L + 1, L + 1)) for _ in range(3))
        for d in range(min(L, span) - 1, MIN_HP, -1):
            i = np.arange(0, L - d)
            j = i + d
            t = PT[S[i], S[j]]
            p, q = i[:, None] - 1 - _N1[None, :], j[:, None] + 1 + _N2[None, :]
            good = (p >= 0) & (q <= L - 1) & (q - p < span) & (t[:, None] > 0)
            pc, qc = np.where(good, p, 0), np.where(good, q, L - 1)
            t2 = PT[S[pc], S[qc]]
            good &= t2 > 0
            e = m.interior(_N1[None, :], _N2[None, :], t2, RT[t][:, None], S[np.minimum(pc + 1, L - 1)], S[qc - 1], S[i - 1][:, None], S[np.minimum(j + 1, L - 1)][:, None])
            il = np.where(good, np.exp(-e * self.beta) * Co[pc, qc], 0.0).sum(axis=1)
            for a in range(L - d):
                z = a + d
                mo = 0.0
                if a >= 1:
                    qq = np.arange(z + 6, min(L, a - 1 + span))
                    if len(qq):
                        mo += float((Co[a - 1, qq] * WC[a - 1, qq]) @ M1[z + 1, qq - 1])
                qq = np.arange(z + 5, min(L, a + span))
                if len(qq):
                    mo += float(Mo[a, qq] @ M1[z + 1, qq])
                Mo[a, z] = mo
                m1o = mo
                ii = np.arange(max(0, z - span + 1), a)
                if len(ii):
                    m1o += float(Mo[ii, z] @ (bp[a - ii] + M[ii, a - 1]))
                if z + 1 < L:
                    if d + 1 < span:
                        m1o += b * M1o[a, z + 1]
                    ii = np.arange(max(0, z + 2 - span), a - 5)
                    if len(ii):
                        m1o += float((Co[ii, z + 1] * WC[ii, z + 1]) @ M[ii + 1, a - 1])
                M1o[a, z] = m1o
                if t[a]:
                    Co[a, z] = F[a] * WE[a, z] * Fr[z + 1] + float(il[a]) + WM[a, z] * m1o
        P = np.zeros((L, L))
        P[:, :] = C[:L, :L] * Co[:L, :L] / Z
        return Z, P, unpaired_of(P)
