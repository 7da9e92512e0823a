"""Inputs that reach the third and the fourth round of the 64-candidate loops of the dynamic-programming kernels, and the mirrors'
results on them (test infrastructure; pure Python / numpy: no GPU, no product code apart from what `_loops.builtin_par` uses).

Every inner sum and search of those kernels runs as `for (x = first + lane; x <= last; x += 64)`: a cell takes round r when it has
more than 64 (r - 1) candidates.  The C and M splits of a cell (i,j) have about j - i candidates, the exterior loop at j has j - 3,
the outside loops of (i,j) have L - j or i.

* `SEQS`: uniform random sequences of 133, 197 and 261 nt - their longest splits take two rounds (133 is a length the MFE driver
  still folds in LDS), three and four, their exterior loops three, four and five - and FAR_BRANCH, constructed: a closing helix
  around a hairpin and a helix that closes 190 random bases.  The last branch of that multiloop is 202 nt long, so the sum of Mo
  over the enclosing pairs (i-1,q) finds its only large term in its fourth round; on the random sequences that sum alone does not
  lose enough after three rounds (tests/test_lane_rounds.py measures each).
* `stretched_tie_sequences()`: the two constructed forms of `_loops.tie_long_sequences()` with the run that separates their stems
  longer by 64 and by 128, and with one more base on the 5' side of the far hairpins: the far stem can start at k or at k + 1, so
  the tie lies between two candidates of the third (fourth) ballot round and only the order within that round decides the row.
* `ScaledPfMirror`: the recurrences of `PfMirror` over scaled quantities (every table entry times scale^(positions it covers)),
  as DESIGN.md section 10 has them.  At scale 1 it is `PfMirror` bit for bit; under the `multiloops_win` tables a 197-nt sequence
  has a minimum near -535 kcal/mol, exp(868) in an unscaled sum, and only the scaled form stays in the fp64 range.
* `RoundsMirror`: that mirror with one of its seven sums cut after `rounds_kept` rounds of 64 candidates, candidates counted from
  the end the kernel starts at.  It states what a loop that stops early computes, so that tests/test_lane_rounds.py can show that
  these inputs tell it from the right one by far more than the bounds of the GPU tests.  It is never compared with the device.
* one cache of the mirrors' results per process: `fold`, `pf`, `band`, `span_fold`, `span_pf`, `con_fold` compute a (tables,
  sequence) result once, whichever test file asks first.
"""
import math

import numpy as np

import _loops as LP
import _mfe_con_np as MC
import _mfe_np as MF
import _mfe_span_np as MS
import _par_reader as PR
import _pf_np as PF
import _pf_span_np as PS
import _subopt_np as SB
from _mfe_np import CODE, MAXLOOP, MIN_HP, PT, RT, _N1, _N2

SEED, LENGTHS = 129, (133, 197, 261)


def _draw():
    rng = np.random.default_rng(SEED)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in LENGTHS]
    arm = "GGCGCG" + "".join(np.random.default_rng(SEED + 1).choice(list("ACGU"), 190)) + "CGCGCC"
    return seqs, "GGGGCC" + "GCGCGAAACGCGC" + "A" + arm + "GGCCCC"


RANDOM_SEQS, FAR_BRANCH = _draw()
SEQS = RANDOM_SEQS + [FAR_BRANCH]
SHORT = ["GGGAAACCC", "".join(np.random.default_rng(64).choice(list("ACGU"), 64))]    # 9 and 64 nt: beside SEQS, Lmax differs from L


def stretched_tie_sequences():
    """[two hairpins k = 1, k = 2, multiloop k = 1, k = 2], 146-234 nt.  Under tie_par a hairpin of n pairs costs 400 - 100 n whatever
    its loop, so one of five pairs and more is strictly favourable and cannot be traded for unpaired bases:
    * a GC hairpin of five pairs, 55 + 64 k N, and UUUUUUNNNAAAAA: its five pairs start at 132 / 196 around a loop of four or at
      133 / 197 around a loop of three, two exterior stems that end at the same j (G pairs with U, but no multiloop can form: after
      a helix of G and U nothing inside it has a partner);
    * a closing helix around a hairpin of 24 pairs, 18 + 64 k N, a CG hairpin of five pairs with six C on its 5' side, and a GU
      hairpin of five pairs: where multiloops cost nothing the M split has its last stem at candidate 129 or 130 (193 or 194) and
      the C split at 145 (209); where they win, other cells tie and the C split is the far one.  (With six G on the GU hairpin as
      well, a hairpin of six pairs over both ties with the two and the M split is never taken.)"""
    hp = lambda n, loop: "C" * n + loop + "G" * n
    two = ["GGGGGNNNCCCCC" + "N" * (55 + 64 * k) + "UUUUUUNNNAAAAA" for k in (1, 2)]
    multi = ["GGG" + "N" + hp(24, "NNNN") + "N" * (18 + 64 * k) + "CCCCCCNNNGGGGG" + "N" + "GGGGGNNNUUUUU" + "N" + "CCC" for k in (1, 2)]
    return two + multi


# ---------------------------------------------------------------- the table sets and one cache

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def par_sets():
    """{name: parameter set}: the sets the GPU test files install - built-in, index-sensitive with winning multiloops, the two flat
    ones, made-up enthalpies"""
    def make():
        builtin = LP.builtin_par()
        idx = LP.index_sensitive_par(builtin)
        idx.update(ml_closing=-700, ml_intern=-300)
        return dict(builtin=builtin, multiloops_win=idx, tie0=LP.tie_par(builtin, LP.TIE_ML[0]), tie1=LP.tie_par(builtin, LP.TIE_ML[1]),
                    synthetic=PR.synthetic_par(builtin))
    return _once("par", make)


def tables(which, temp=37.0):
    return _once(("tables", which, temp), lambda: PR.tables_at(par_sets()[which], temp))


def mirror(which, temp=37.0):
    """the one Mirror of a table set: `fold` and `band` share its filled tables"""
    return _once(("Mirror", which, temp), lambda: MF.Mirror(tables(which, temp)))


def fold(which, seq, order="first", temp=37.0):
    """((dcal, row), offsets) of Mirror.fold"""
    def make():
        m = mirror(which, temp)
        return m.fold(seq, order), dict(m.offsets)
    return _once(("fold", which, temp, seq, order), make)


def base_mirror(which, seq, temp=37.0):
    """a PfMirror of the table set that has run on `seq` (its tables are what RoundsMirror.run starts from), and its (Z, P)"""
    def make():
        m = PF.PfMirror(tables(which, temp), temp)
        return m, m.run(seq)
    return _once(("pf", which, temp, seq), make)


def pf(which, seq, temp=37.0):
    """(ensemble energy in kcal/mol, P) of PfMirror.run"""
    m, (Z, P) = base_mirror(which, seq, temp)
    return m.energy(Z), P


def scaled_pf(which, seq, temp=37.0):
    """(ensemble energy in kcal/mol, P) of ScaledPfMirror.run under the scale that brings the minimum's weight to 1"""
    def make():
        ln_scale = fold(which, seq, temp=temp)[0][0] / (100.0 * PF.kt_of(temp) * len(seq))
        m = ScaledPfMirror(tables(which, temp), temp, ln_scale)
        lnz, P = m.run(seq)
        return -m.kt * lnz, P
    return _once(("scaled pf", which, temp, seq), make)


def band(which, seq, delta):
    return _once(("band", which, seq, delta), lambda: SB.band(mirror(which), seq, delta))


def span_fold(which, seq, span):
    """(dcal, row) of SpanMirror.fold"""
    m = _once(("SpanMirror", which), lambda: MS.SpanMirror(tables(which)))
    return _once(("span_fold", which, seq, span), lambda: m.fold(seq, span))


def span_pf(which, seq, span):
    """(Z, P, unpaired) of PfSpanMirror.run"""
    return _once(("span_pf", which, seq, span), lambda: PS.PfSpanMirror(tables(which), span).run(seq))


CON_DRAW = {133: 7, 197: 3}     # the first draw of a sequence's stream that some structure satisfies; most at these lengths leave none


def con_cases():
    """one (seq, con, u, b) for the 133- and for the 197-nt sequence: draw CON_DRAW[L] of `draw_constraint` from the stream seeded
    (SEED, L), and a soft u on every position drawn before it"""
    out = []
    for s in SEQS[:2]:
        rng = np.random.default_rng((SEED, len(s)))
        u = rng.integers(-150, 151, len(s)).astype(np.int32)
        for _ in range(CON_DRAW[len(s)] + 1):
            con = MC.draw_constraint(rng, s)
        out.append((s, con, u, None))
    return out


def con_fold(case):
    """((dcal, row), pseudo_dcal, offsets) of ConMirror.fold on a case of con_cases()"""
    def make():
        m = MC.ConMirror(tables("builtin"))
        got = m.fold(*case)
        return got, m.pseudo, dict(m.offsets)
    return _once(("con_fold", case[0], case[1]), make)


# ---------------------------------------------------------------- the scaled sums, and a sum that stops early

INSIDE_LOOPS = ("C split", "M split", "exterior F")
OUTSIDE_LOOPS = ("Mo over Co", "Mo over Mo", "M1o over Mo", "M1o over Co")
LOOPS = INSIDE_LOOPS + OUTSIDE_LOOPS


class ScaledPfMirror(PF.PfMirror):
    """PfMirror over X'[i][j] = X[i][j] s^(j - i + 1) for the inside tables, F'[j + 1] = F[j + 1] s^(j + 1), Fr'[i] = Fr[i] s^(L - i),
    and X'[i][j] = X[i][j] s^(L - (j - i + 1)) for the outside tables, s = exp(ln_scale): a hairpin takes s^(d + 1), an interior loop
    s^(n1 + n2 + 2), an unpaired base of a multiloop or of the exterior loop s, a closing pair s^2.  `run` returns (ln Z, P).
    `cut(name, x)` is the candidate list of the sum `name`: all of x here."""

    def __init__(self, tables, temp=37.0, ln_scale=0.0):
        super().__init__(tables, temp)
        self.ln_scale = ln_scale

    def cut(self, name, x):
        return x

    def inside(self, seq, base=None, first_d=MIN_HP + 1):
        """base: a PfMirror that has run on `seq`, unscaled - the cells of the anti-diagonals below first_d are taken from it"""
        m, sc, w, cut = self.m, self.sc, self.w, self.cut
        L = self.L = len(seq)
        S = self.S = np.array([CODE[c] for c in seq], dtype=np.int64)
        nb = lambda x: int(S[x]) if 0 <= x < L else -1
        s = math.exp(self.ln_scale)
        sp = self.sp = s ** np.arange(max(L, MAXLOOP) + 3, dtype=np.float64)
        b = w(sc["ml_base"]) * s
        bp = self.bp = b ** np.arange(L + 1, dtype=np.float64)
        if base is not None:
            assert self.ln_scale == 0.0 and base.L == L
            WM, WE, WC = base.WM, base.WE, base.WC
            C, M, M1 = base.C.copy(), base.M.copy(), base.M1.copy()
        else:
            C, M, M1 = (np.zeros((L + 1, L + 1)) for _ in range(3))
            WM, WE, WC = (np.zeros((L + 1, L + 1)) for _ in range(3))
            for i in range(L):
                for j in range(i + MIN_HP + 1, L):
                    t = int(PT[S[i], S[j]])
                    if t:
                        WM[i, j] = w(m.stem(t, nb(i - 1), nb(j + 1), False))
                        WE[i, j] = w(m.stem(t, nb(i - 1), nb(j + 1), True))
                        WC[i, j] = w(sc["ml_closing"] + m.stem(int(RT[t]), int(S[j - 1]), int(S[i + 1]), False)) * sp[2]
        for d in range(first_d, L):
            i = np.arange(0, L - d)
            j = i + d
            t = PT[S[i], S[j]]
            p, q = i[:, None] + 1 + _N1[None, :], j[:, None] - 1 - _N2[None, :]
            good = (q - p >= MIN_HP + 1) & (t[:, None] > 0)
            pc, qc = np.where(good, p, 1), np.where(good, q, 1)
            t2 = PT[S[pc], S[qc]]
            good &= t2 > 0
            e = m.interior(_N1[None, :], _N2[None, :], t[:, None], RT[t2], S[i + 1][:, None], S[j - 1][:, None], S[pc - 1], S[np.minimum(qc + 1, L - 1)])
            il = np.where(good, np.exp(-e * self.beta) * sp[_N1 + _N2 + 2][None, :] * C[pc, qc], 0.0).sum(axis=1)
            for a in range(L - d):
                z = a + d
                if t[a]:
                    c = w(m.hairpin(seq, S, a, z)) * sp[d + 1] + float(il[a])
                    k = cut("C split", np.arange(a + 6, z - 4))
                    if len(k):
                        c += WC[a, z] * float(M[a + 1, k - 1] @ M1[k, z - 1])
                    C[a, z] = c
                M1[a, z] = C[a, z] * WM[a, z] + M1[a, z - 1] * b
                k = np.concatenate([[a], cut("M split", np.arange(a + 1, z - 3))])
                M[a, z] = float((bp[k - a] + M[a, k - 1]) @ M1[k, z])
        F = np.zeros(L + 1)                     # F[j + 1]: positions 0..j
        F[0] = 1.0
        for j in range(L):
            i = cut("exterior F", np.arange(0, max(j - MIN_HP, 0)))
            F[j + 1] = F[j] * s + float((F[i] * C[i, j]) @ WE[i, j])
        Fr = np.zeros(L + 2)                    # Fr[i]: positions i..L-1
        Fr[L] = 1.0
        for i in range(L - 1, -1, -1):
            j = np.arange(i + MIN_HP + 1, L)
            Fr[i] = Fr[i + 1] * s + float((C[i, j] * WE[i, j]) @ Fr[j + 1])
        self.C, self.M, self.M1, self.F, self.Fr, self.WM, self.WE, self.WC, self.b = C, M, M1, F, Fr, WM, WE, WC, b
        return float(F[L])

    def run(self, seq, base=None, first_d=MIN_HP + 1):
        """(ln Z, P): the logarithm of the unscaled partition function and the L x L array of pair probabilities"""
        Z = self.inside(seq, base, first_d)
        cut = self.cut
        L, S, m, sp = self.L, self.S, self.m, self.sp
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
            il = np.where(good, np.exp(-e * self.beta) * sp[_N1 + _N2 + 2][None, :] * Co[pc, qc], 0.0).sum(axis=1)
            for a in range(L - d):
                z = a + d
                mo = 0.0
                if a >= 1:
                    qq = cut("Mo over Co", np.arange(z + 6, L))
                    if len(qq):
                        mo += float((Co[a - 1, qq] * WC[a - 1, qq]) @ M1[z + 1, qq - 1])
                qq = cut("Mo over Mo", np.arange(z + 5, L))
                if len(qq):
                    mo += float(Mo[a, qq] @ M1[z + 1, qq])
                Mo[a, z] = mo
                m1o = mo
                ii = cut("M1o over Mo", np.arange(0, a))
                if len(ii):
                    m1o += float(Mo[ii, z] @ (bp[a - ii] + M[ii, a - 1]))
                if z + 1 < L:
                    m1o += b * M1o[a, z + 1]
                    ii = cut("M1o over Co", np.arange(0, a - 5))
                    if len(ii):
                        m1o += float((Co[ii, z + 1] * WC[ii, z + 1]) @ M[ii + 1, a - 1])
                M1o[a, z] = m1o
                if t[a]:
                    Co[a, z] = F[a] * WE[a, z] * Fr[z + 1] + float(il[a]) + WM[a, z] * m1o
        P = np.zeros((L, L))
        P[:, :] = C[:L, :L] * Co[:L, :L] / Z
        return math.log(Z) - L * self.ln_scale, P


class RoundsMirror(ScaledPfMirror):
    """ScaledPfMirror at scale 1 whose sum `which` (one of LOOPS) keeps its first 64 * rounds_kept candidates only, counted as the
    kernel counts them: C split k from i + 6, M split k from i + 1 (k = i is M1 itself), exterior i from 0, the two sums of Mo q from
    j + 6 and j + 5, the two sums of M1o h from 0.  `run(seq, base)` takes the inside cells below the anti-diagonal 64 * rounds_kept,
    which have fewer candidates than are kept, from `base` - all of them where the cut sum is none of the two splits."""

    def __init__(self, tables, which, rounds_kept, temp=37.0):
        super().__init__(tables, temp)
        assert which in LOOPS
        self.which, self.n_kept = which, 64 * rounds_kept
        self.n_cut = 0                                          # candidates dropped

    def cut(self, name, x):
        if name != self.which or len(x) <= self.n_kept:
            return x
        self.n_cut += len(x) - self.n_kept
        return x[:self.n_kept]

    def run(self, seq, base):
        return super().run(seq, base, self.n_kept if self.which in ("C split", "M split") else len(seq))
