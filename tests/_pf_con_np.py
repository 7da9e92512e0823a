"""The partition function under hard constraints and soft terms, twice, for the tests of rafft_pf_constrained_batch (test
infrastructure; pure Python / numpy: no GPU, no product code).  DESIGN.md section 21.

* `exact_con(seq, con, u, b, rows, dcal, kt)`: `_pf_np.exact` over the rows that `_mfe_con_np.satisfies`, with `_mfe_con_np.pseudo`
  added to their energies: `(Z, P, best)` - best the smallest objective of the filtered set - or `(0.0, zeros, None)` when no row
  satisfies the constraint.
* `PfConMirror(tables)`: `PfMirror` with the constrained recurrences, unscaled fp64.  With w(e) = exp(-e / (100 kT)), b = w(ml_base)
  and ok, up, free, U, stack of section 20:
      C[i][j]   0 unless ok(i,j); hairpin only if free(i+1,j-1): w(hairpin + U(i+1,j-1)); interior with (p,q) only if free(i+1,p-1) and
                free(q+1,j-1): w(interior + both U + stack when p = i+1, q = j-1) C[p][q]; the multiloop term unchanged
      M1[i][j]  = C[i][j] w(stem) + [up(j)] M1[i][j-1] b w(u[j])
      M[i][j]   = sum_{k=i..j} ([free(i,k-1)] b^(k-i) w(U(i,k-1)) + M[i][k-1]) M1[k][j]
      F[j]      = [up(j)] F[j-1] w(u[j]) + sum_i F[i-1] C[i][j] w(stem_ext);  Fr the same from the 3' end
      Mo        unchanged
      M1o[k][j] = [up(j+1)] b w(u[j+1]) M1o[k][j+1] + (the Co term, unchanged) + sum_{i<=k} Mo[i][j] ([free(i,k-1)] b^(k-i) w(U(i,k-1)) + M[i][k-1])
      Co[i][j]  0 unless ok(i,j); else F[i-1] w(stem_ext) Fr[j+1] + sum over enclosing (p,q) with free(p+1,i-1) and free(j+1,q-1) of
                Co[p][q] w(interior + soft) + w(stem) M1o[i][j]
      P(i,j)    = C[i][j] Co[i][j] / Z;   unpaired[k] = 1 - sum_j P(k,j) - sum_i P(i,k)
  `run(seq, con, u, b)` is `(Z, P, unpaired)`; Z = 0.0 (P and unpaired zeros) when no structure satisfies the constraints.
  `drop_free=True` switches one defect on: the free(i,k-1) test of the b^(k-i) term of M is dropped, so a multiloop may leave
  positions unpaired that have to pair.  The tests feed it to the same check to show they see it (as `ambiguous=True` of PfMirror).
"""
import numpy as np

import _mfe_con_np as MC
from _mfe_np import CODE, PT, RT, MIN_HP, _N1, _N2
from _pf_np import PfMirror, exact


def exact_con(seq, con, u, b, rows, dcal, kt):
    keep = [(r, e + MC.pseudo(r, u, b)) for r, e in zip(rows, dcal) if MC.satisfies(r, con)]
    if not keep:
        return 0.0, np.zeros((len(seq), len(seq))), None
    Z, P = exact([r for r, _ in keep], [e for _, e in keep], kt)
    return Z, P, min(e for _, e in keep)


def unpaired_of(P):
    return 1.0 - P.sum(axis=1) - P.sum(axis=0)


class PfConMirror(PfMirror):
    def __init__(self, tables, temp=37.0, drop_free=False):
        super().__init__(tables, temp)
        self.drop_free = drop_free

    def _range_w(self, a, k, in_m=False):
        """[free(a,k-1)] w(U(a,k-1)) for arrays a, k (the empty range: 1)"""
        st = self.st
        wU = np.exp(-(st.usum[k] - st.usum[a]) * self.beta)
        if in_m and self.drop_free:
            return wU
        return np.where(st.must[k] == st.must[a], wU, 0.0)

    def inside(self, seq, con=None, u=None, b=None):
        m, sc, w = self.m, self.sc, self.w
        st = self.st = MC.ConMirror._state(None, seq, con, u, b)
        L = self.L = len(seq)
        S = self.S = np.array([CODE[c] for c in seq], dtype=np.int64)
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        bb = w(sc["ml_base"])
        bp = self.bp = bb ** np.arange(L + 1, dtype=np.float64)
        upw = self.upw = np.where(st.up, np.exp(-st.u * self.beta), 0.0)     # [up(k)] w(u[k])
        idx = np.arange(L)
        OK = self.OK = (st.left[:, None] | (st.partner[:, None] == idx[None, :])) & (st.right[None, :] | (st.partner[None, :] == idx[:, None]))
        C, M, M1 = (np.zeros((L + 1, L + 1)) for _ in range(3))
        WM, WE, WC = (np.zeros((L + 1, L + 1)) for _ in range(3))
        for i in range(L):
            for j in range(i + MIN_HP + 1, L):
                t = int(PT[S[i], S[j]])
                if t:
                    WM[i, j] = w(m.stem(t, nb(i - 1), nb(j + 1), False))
                    WE[i, j] = w(m.stem(t, nb(i - 1), nb(j + 1), True))
                    WC[i, j] = w(sc["ml_closing"] + m.stem(int(RT[t]), int(S[j - 1]), int(S[i + 1]), False))
        for d in range(MIN_HP + 1, L):
            i = np.arange(0, L - d)
            j = i + d
            t = PT[S[i], S[j]]
            p, q = i[:, None] + 1 + _N1[None, :], j[:, None] - 1 - _N2[None, :]
            good = (q - p >= MIN_HP + 1) & (t[:, None] > 0)
            pc, qc = np.where(good, p, 1), np.where(good, q, 1)
            t2 = PT[S[pc], S[qc]]
            good &= t2 > 0
            i1, j0 = (i + 1)[:, None], j[:, None]
            good &= (st.must[pc] == st.must[i1]) & (st.must[j0] == st.must[qc + 1])
            soft = (st.usum[pc] - st.usum[i1]) + (st.usum[j0] - st.usum[qc + 1])
            soft = soft + np.where((_N1 == 0) & (_N2 == 0), st.b[i][:, None] + st.b[j][:, None] + st.b[pc] + st.b[qc], 0)
            e = m.interior(_N1[None, :], _N2[None, :], t[:, None], RT[t2], S[i + 1][:, None], S[j - 1][:, None], S[pc - 1], S[np.minimum(qc + 1, L - 1)])
            il = np.where(good, np.exp(-(e + soft) * self.beta) * C[pc, qc], 0.0).sum(axis=1)
            for a in range(L - d):
                z = a + d
                if t[a] and OK[a, z]:
                    c = float(il[a])
                    if st.must[z] == st.must[a + 1]:
                        c += w(m.hairpin(seq, S, a, z) + int(st.usum[z] - st.usum[a + 1]))
                    k = np.arange(a + 6, z - 4)
                    if len(k):
                        c += WC[a, z] * float(M[a + 1, k - 1] @ M1[k, z - 1])
                    C[a, z] = c
                M1[a, z] = C[a, z] * WM[a, z] + M1[a, z - 1] * bb * upw[z]
                k = np.arange(a, z - 3)
                M[a, z] = float((bp[k - a] * self._range_w(a, k, in_m=True) + M[a, k - 1]) @ M1[k, z])
        F = np.zeros(L + 1)
        F[0] = 1.0
        for j in range(L):
            i = np.arange(0, max(j - MIN_HP, 0))
            F[j + 1] = F[j] * upw[j] + float((F[i] * C[i, j]) @ WE[i, j])
        Fr = np.zeros(L + 2)
        Fr[L] = 1.0
        for i in range(L - 1, -1, -1):
            j = np.arange(i + MIN_HP + 1, L)
            Fr[i] = Fr[i + 1] * upw[i] + float((C[i, j] * WE[i, j]) @ Fr[j + 1])
        self.C, self.M, self.M1, self.F, self.Fr, self.WM, self.WE, self.WC, self.b = C, M, M1, F, Fr, WM, WE, WC, bb
        return float(F[L])

    def run(self, seq, con=None, u=None, b=None):
        """(Z, P, unpaired)"""
        Z = self.inside(seq, con, u, b)
        L, S, m, st = self.L, self.S, self.m, self.st
        if Z == 0.0:
            return 0.0, np.zeros((L, L)), np.zeros(L)
        C, M, M1, F, Fr, WM, WE, WC, bb, bp, upw, OK = self.C, self.M, self.M1, self.F, self.Fr, self.WM, self.WE, self.WC, self.b, self.bp, self.upw, self.OK
        Co, Mo, M1o = (np.zeros((L + 1, L + 1)) for _ in range(3))
        for d in range(L - 1, MIN_HP, -1):
            i = np.arange(0, L - d)
            j = i + d
            t = PT[S[i], S[j]]
            p, q = i[:, None] - 1 - _N1[None, :], j[:, None] + 1 + _N2[None, :]
            good = (p >= 0) & (q <= L - 1) & (t[:, None] > 0)
            pc, qc = np.where(good, p, 0), np.where(good, q, L - 1)
            t2 = PT[S[pc], S[qc]]
            good &= t2 > 0
            i0, j1 = i[:, None], (j + 1)[:, None]
            good &= (st.must[i0] == st.must[pc + 1]) & (st.must[qc] == st.must[j1])
            soft = (st.usum[i0] - st.usum[pc + 1]) + (st.usum[qc] - st.usum[j1])
            soft = soft + np.where((_N1 == 0) & (_N2 == 0), st.b[pc] + st.b[qc] + st.b[i][:, None] + st.b[j][:, None], 0)
            e = m.interior(_N1[None, :], _N2[None, :], t2, RT[t][:, None], S[np.minimum(pc + 1, L - 1)], S[qc - 1], S[i - 1][:, None], S[np.minimum(j + 1, L - 1)][:, None])
            il = np.where(good, np.exp(-(e + soft) * self.beta) * Co[pc, qc], 0.0).sum(axis=1)
            for a in range(L - d):
                z = a + d
                mo = 0.0
                if a >= 1:
                    qq = np.arange(z + 6, L)
                    if len(qq):
                        mo += float((Co[a - 1, qq] * WC[a - 1, qq]) @ M1[z + 1, qq - 1])
                qq = np.arange(z + 5, L)
                if len(qq):
                    mo += float(Mo[a, qq] @ M1[z + 1, qq])
                Mo[a, z] = mo
                m1o = mo
                ii = np.arange(0, a)
                if len(ii):
                    m1o += float(Mo[ii, z] @ (bp[a - ii] * self._range_w(ii, a) + M[ii, a - 1]))
                if z + 1 < L:
                    m1o += bb * upw[z + 1] * M1o[a, z + 1]
                    ii = np.arange(0, a - 5)
                    if len(ii):
                        m1o += float((Co[ii, z + 1] * WC[ii, z + 1]) @ M[ii + 1, a - 1])
                M1o[a, z] = m1o
                if t[a] and OK[a, z]:
                    Co[a, z] = F[a] * WE[a, z] * Fr[z + 1] + float(il[a]) + WM[a, z] * m1o
        P = C[:L, :L] * Co[:L, :L] / Z
        return Z, P, unpaired_of(P)
