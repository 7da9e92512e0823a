"""The partition function, twice, for the tests of rafft_pf_batch (test infrastructure; pure Python / numpy: no GPU, no product code).

* `exact(rows, dcal, kt)`: Z and P(i,j) of an enumerated ensemble - the structures `rows` with the energies `dcal` - summed with
  math.fsum, so the result is the correctly rounded sum of the weights exp(-dcal / (100 kT)).
* `PfMirror(tables)`: a plain fp64 restatement, unscaled, of the recurrences of DESIGN.md section 10 over the tables
  tests/_par_reader.py reads.  The loop energies are `Mirror`'s of tests/_mfe_np.py (hairpin / interior / stem): the model is not
  written out again.  With b = w(ml_base), w(e) = exp(-e / (100 kT)):
      C[i][j]  = w(hairpin) + sum over inner pairs (p,q), n1 + n2 <= 30, of w(interior) C[p][q]
                 + w(ml_closing + stem(closing pair, read from inside)) sum_k M[i+1][k-1] M1[k][j-1]
      M1[i][j] = C[i][j] w(stem(i,j)) + M1[i][j-1] b
      M[i][j]  = sum_{k=i..j} (b^(k-i) + M[i][k-1]) M1[k][j]
      F[j]     = F[j-1] + sum_i F[i-1] C[i][j] w(exterior stem(i,j)),  Z = F[L-1];  Fr the same from the 3' end
  and, descending over j - i, one outside variable per inside one (Mo before M1o before Co within a cell):
      Mo[i][j]  = sum_{q>j+1} Co[i-1][q] w(close(i-1,q)) M1[j+1][q-1] + sum_{q>j} Mo[i][q] M1[j+1][q]
      M1o[k][j] = b M1o[k][j+1] + sum_{i<k} Co[i][j+1] w(close(i,j+1)) M[i+1][k-1] + sum_{i<=k} Mo[i][j] (b^(k-i) + M[i][k-1])
      Co[i][j]  = F[i-1] w(exterior stem(i,j)) Fr[j+1] + sum over enclosing (p,q), n1 + n2 <= 30, of Co[p][q] w(interior)
                  + w(stem(i,j)) M1o[i][j]
      P(i,j)    = C[i][j] Co[i][j] / Z
  `ambiguous=True` replaces M by the MFE's M of DESIGN.md section 9 (M1[i][j] + M[i+1][j] b + sum_k M[i][k-1] M1[k][j]), which
  derives "i unpaired, two stems" twice: right under min, wrong under +.  The tests feed it to the same check to show they see it.
"""
import math

import numpy as np

from _mfe_np import CODE, PT, RT, MAXLOOP, MIN_HP, Mirror, _N1, _N2

GAS = 1.98717e-3            # kcal / (mol K)


def kt_of(temp=37.0):
    return (temp + 273.15) * GAS


def pairs_of(db):
    stack, out = [], []
    for x, c in enumerate(db):
        if c == "(":
            stack.append(x)
        elif c == ")":
            out.append((stack.pop(), x))
    return out


def exact(rows, dcal, kt):
    """(Z, P) of the ensemble `rows` with energies `dcal` (dcal/mol): Z a float, P an L x L array, P[i][j] for i < j"""
    L = len(rows[0])
    w = [math.exp(-e / (100.0 * kt)) for e in dcal]
    Z = math.fsum(w)
    per = {}
    for r, x in zip(rows, w):
        for ij in pairs_of(r):
            per.setdefault(ij, []).append(x)
    P = np.zeros((L, L))
    for (i, j), xs in per.items():
        P[i, j] = math.fsum(xs) / Z
    return Z, P


def has_leading_unpaired_multiloop(db):
    """True when some multiloop of `db` has an unpaired base between its closing pair's 5' end and its first inner stem"""
    pt = [-1] * len(db)
    for i, j in pairs_of(db):
        pt[i], pt[j] = j, i
    for i, j in enumerate(pt):
        if j > i:
            k, br, first = i + 1, 0, None
            while k < j:
                if pt[k] > k:
                    if first is None:
                        first = k
                    br += 1
                    k = pt[k] + 1
                else:
                    k += 1
            if br >= 2 and first > i + 1:
                return True
    return False


class PfMirror:
    def __init__(self, tables, temp=37.0, ambiguous=False):
        self.m = Mirror(tables)
        self.sc = tables["scalars"]
        self.kt = kt_of(temp)
        self.beta = 1.0 / (100.0 * self.kt)
        self.ambiguous = ambiguous

    def w(self, e):
        return math.exp(-e * self.beta)

    def inside(self, seq):
        m, sc, w = self.m, self.sc, self.w
        L = self.L = len(seq)
        S = self.S = np.array([CODE[c] for c in seq], dtype=np.int64)
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        b = w(sc["ml_base"])
        bp = self.bp = b ** np.arange(L + 1, dtype=np.float64)
        # column L of every table stays 0: index -1 reads it
        C, M, M1 = (np.zeros((L + 1, L + 1)) for _ in range(3))
        WM, WE, WC = (np.zeros((L + 1, L + 1)) for _ in range(3))       # w(stem in a multiloop), w(exterior stem), w(closing a multiloop)
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
                if self.ambiguous:
                    M[a, z] = M1[a, z] + M[a + 1, z] * b + float(M[a, k - 1] @ M1[k, z])
                else:
                    M[a, z] = float((bp[k - a] + M[a, k - 1]) @ M1[k, z])
        F = np.zeros(L + 1)                     # F[j + 1]: positions 0..j
        F[0] = 1.0
        for j in range(L):
            i = np.arange(0, max(j - MIN_HP, 0))
            F[j + 1] = F[j] + float((F[i] * C[i, j]) @ WE[i, j])
        Fr = np.zeros(L + 2)                    # Fr[i]: positions i..L-1
        Fr[L] = 1.0
        for i in range(L - 1, -1, -1):
            j = np.arange(i + MIN_HP + 1, L)
            Fr[i] = Fr[i + 1] + float((C[i, j] * WE[i, j]) @ Fr[j + 1])
        self.C, self.M, self.M1, self.F, self.Fr, self.WM, self.WE, self.WC, self.b = C, M, M1, F, Fr, WM, WE, WC, b
        return float(F[L])

    def run(self, seq):
        """(Z, P): the partition function and the L x L array of pair probabilities"""
        Z = self.inside(seq)
        assert not self.ambiguous
        L, S, m = self.L, self.S, self.m
        C, M, M1, F, Fr, WM, WE, WC, b, bp = self.C, self.M, self.M1, self.F, self.Fr, self.WM, self.WE, self.WC, self.b, self.bp
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
            e = m.interior(_N1[None, :], _N2[None, :], t2, RT[t][:, None], S[np.minimum(pc + 1, L - 1)], S[qc - 1], S[i - 1][:, None], S[np.minimum(j + 1, L - 1)][:, None])
            il = np.where(good, np.exp(-e * self.beta) * Co[pc, qc], 0.0).sum(axis=1)
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
                    m1o += float(Mo[ii, z] @ (bp[a - ii] + M[ii, a - 1]))
                if z + 1 < L:
                    m1o += b * M1o[a, z + 1]
                    ii = np.arange(0, a - 5)
                    if len(ii):
                        m1o += float((Co[ii, z + 1] * WC[ii, z + 1]) @ M[ii + 1, a - 1])
                M1o[a, z] = m1o
                if t[a]:
                    Co[a, z] = F[a] * WE[a, z] * Fr[z + 1] + float(il[a]) + WM[a, z] * m1o
        P = np.zeros((L, L))
        P[:, :] = C[:L, :L] * Co[:L, :L] / Z
        return Z, P

    def energy(self, Z):
        return -self.kt * math.log(Z)
