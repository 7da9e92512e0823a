"""Constructed loops for the energy model (test infrastructure; pure Python: no GPU, no oracle).

* `index_sensitive_par(par)`: a parameter set whose table entries are pairwise distinct within their table (only the
  symmetries the file format and ViennaRNA impose are kept) - with it any transposed index changes an energy.
* `loop_cases()`: (name, target, seq, db) - one smallest structure per table entry / rule of the model.  `target` is
  `(table, index tuple)` in the oracle's layout (pair types CG=1 GC=2 GU=3 UG=4 AU=5 UA=6, bases N=0 A=1 C=2 G=3 U=4), a scalar
  `(name, ())`, a special hairpin `("special", (kind, k))` or `("none", ())`.
* `reads(seq, db, special)`: which entries the nearest-neighbour model reads for a structure, and how often (a plain
  restatement of the loop decomposition; tests/test_energy_model.py checks it against the oracle entry by entry).
* `bad_rows()`: malformed rows and what an evaluator has to say about them.
* `parent_cases()`: (name, seq, db, pos) - hand-made parents for the expand seam.
"""
import os
import tempfile
from collections import Counter

import numpy as np

import _par_reader as PR

B = "NACGU"
CODE = {c: i for i, c in enumerate(B)}
PT = {1: "CG", 2: "GC", 3: "GU", 4: "UG", 5: "AU", 6: "UA"}
TYPE = {v: k for k, v in PT.items()}
RT = {1: 2, 2: 1, 3: 4, 4: 3, 5: 6, 6: 5}
TYPES = (1, 2, 3, 4, 5, 6)
ACGU = (1, 2, 3, 4)
MM_TABLES = ("mismatch_hairpin", "mismatch_interior", "mismatch_interior_1n", "mismatch_interior_23", "mismatch_multi",
             "mismatch_exterior")
SCALARS = ("ml_base", "ml_closing", "ml_intern", "ninio", "max_ninio", "term_au")
KINDS = ("Triloops", "Tetraloops", "Hexaloops")
OWN_SPECIAL = {"Triloops": ["GACAC", "AUGUU"], "Tetraloops": ["GACCAC", "UGUGUA"], "Hexaloops": ["GACACCAC", "CAUUGUUG"]}
HIGH_NRJ = 1.0e6          # kcal/mol: above any dE, the forbidden hairpins' INF terms (1e5 kcal/mol each) included


# ---------------------------------------------------------------- parameter sets

def builtin_par():
    """the built-in set, written by the product and read back by the tests' own reader"""
    from rafft_amd import params
    params.reset_params()
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "builtin.par")
        params.save_params(p)
        return PR.read_par(p)


def _flat_index(shape):
    return np.arange(int(np.prod(shape))).reshape(shape)


def index_sensitive_par(par, seed=2004):
    rng = np.random.default_rng(seed)
    out = {k: (v.copy() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, list) else v)) for k, v in par.items()
           if not k.endswith("_enthalpies") and not k.endswith("_dH")}
    for k in ("ninio_dH", "ml_base_dH", "ml_closing_dH", "ml_intern_dH", "duplex_init_dH", "terminal_au_dH"):
        out[k] = 0

    def distinct(name, lo, step, sym=None, sl=slice(None)):
        old = np.asarray(par[name])[sl]
        v = lo + step * rng.permutation(old.size).reshape(old.shape)
        if sym is not None:                      # both members of an orbit take the value drawn for the smaller flat index
            idx = _flat_index(old.shape)
            v = v.reshape(-1)[np.minimum(idx, idx.transpose(sym))]
        new = np.where(old >= PR.INF, old, v)
        a = np.asarray(par[name]).copy()
        a[sl] = new
        out[name] = a

    distinct("stack", -60, -9, sym=(1, 0))
    distinct("mismatch_hairpin", -190, 2)
    distinct("mismatch_interior", -171, 2)
    distinct("mismatch_interior_1n", -260, 3)
    distinct("mismatch_interior_23", -301, 3)
    distinct("mismatch_multi", -5, -2)           # (dangles = 2: positive multi / exterior mismatches and dangles are clipped to 0)
    distinct("mismatch_exterior", -6, -2)
    distinct("dangle5", -11, -4)
    distinct("dangle3", -13, -4)
    distinct("int11", -300, 1, sym=(1, 0, 3, 2))
    distinct("int21", -2000, 1)
    distinct("int22", -3000, 1, sym=(1, 0, 4, 5, 2, 3))
    distinct("hairpin", 300, 13, sl=slice(3, None))
    distinct("bulge", 250, 11, sl=slice(1, None))
    distinct("interior", 150, 7, sl=slice(2, None))
    out.update(ml_base=7, ml_closing=931, ml_intern=-91, ninio=61, max_ninio=307, terminal_au=53, lxc=109.0)
    k = 0
    for name in KINDS:
        have = [s for s, _, _ in par[name]]
        assert not set(have) & set(OWN_SPECIAL[name])
        ent = []
        for s in have + OWN_SPECIAL[name]:
            ent.append((s, -400 + 11 * k, 0))
            k += 1
        out[name] = ent
    return out


TIE_ML = ((0, 0, 0), (0, -400, -200))     # (ml_base, ml_closing, ml_intern): multiloops cost nothing / multiloops win


def tie_par(par, ml):
    """a flat parameter set, under which many structures of a sequence share the minimum and only the traceback's candidate order
    decides the row: every stack -100, every mismatch and dangle 0, every loop table one constant whatever the size (hairpin 300,
    bulge and interior 200, the tabulated 1x1 / 2x1 / 2x2 loops 200 as well), no special loops, terminal_au = ninio = lxc = 0, and
    the multiloop scalars `ml` = (ml_base, ml_closing, ml_intern).  Built from index_sensitive_par's copy of `par` (no enthalpies)."""
    out = index_sensitive_par(par)

    def flat(name, value):
        old = np.asarray(out[name])
        out[name] = np.where(old >= PR.INF, old, value)

    flat("stack", -100)
    for name in MM_TABLES + ("dangle5", "dangle3"):
        flat(name, 0)
    flat("hairpin", 300)
    for name in ("bulge", "interior", "int11", "int21", "int22"):
        flat(name, 200)
    out.update(ml_base=ml[0], ml_closing=ml[1], ml_intern=ml[2], ninio=0, max_ninio=300, terminal_au=0, lxc=0.0)
    for name in KINDS:
        out[name] = []
    return out


def tie_short_sequences():
    """low-complexity, GC-only and random sequences of at most 20 nt (every structure can be enumerated), then N bases in a hairpin
    loop, beside a closing pair inside and outside, in an interior loop and between two stems of a multiloop"""
    rng = np.random.default_rng(4242)
    seqs = ["GU" * 9, "G" * 8 + "U" * 8, "GCGCAAAGCGCAAAGCGC", "GGGUUUGGGUUUCCC", "GGGAAACCCAGGGAAACCCA", "GCGCGCGCGCGCGCGC", "GGCCGGCCAAAAGGCCGGCC",
            "CCCCAAAAGGGGAAAACCCC", "GGGGAAAACCCCAAAAGGGG", "AU" * 9]
    seqs += ["".join(rng.choice(list("GC"), n)) for n in (14, 16, 18)]
    seqs += ["".join(rng.choice(list("ACGU"), n)) for n in (16, 18, 20)]
    return seqs + N_SEQS


# N pairs with nothing and reads row 0 of the mismatch and dangle tables
N_SEQS = ["GGGNAAACCC", "GGNGAAACNCC", "GGGAAANCCCAGGGNAACCC", "GNGAAACGAAACGNAACC"]


def tie_long_sequences():
    """40-105 nt: random, GU-only, GC-only, repeats, and two constructed ones.  Under tie_par a hairpin of n pairs costs 400 - 100 n,
    so one of five pairs and more is strictly favourable and cannot be traded for unpaired bases:
    * a closing helix around a hairpin of 24 pairs, 18 N, a CG and a GU hairpin of five pairs (no helix between the two pairs as
      many bases): the M split of the multiloop has its last
      stem 69 positions after the first, the C split its last stem further still;
    * two hairpins of five and four + one pairs with 55 A between them: the second exterior stem starts at position 68."""
    rng = np.random.default_rng(99)
    rand = lambda n, letters="ACGU": "".join(rng.choice(list(letters), n))
    hp = lambda n, loop: "C" * n + loop + "G" * n
    seqs = [rand(40), rand(60), rand(80), rand(100), rand(64, "GU"), rand(90, "GU"), rand(60, "GC"), rand(96, "GC"), "GGGAAACCC" * 5, "GGGAAACCC" * 11]
    seqs.append("GGG" + "N" + hp(24, "NNNN") + "N" * 18 + hp(5, "NNN") + "N" + "GGGGGNNNUUUUU" + "N" + "CCC")
    seqs.append("GGGGGAAACCCCC" + "A" * 55 + "GGGGCAAAGCCCC")
    return seqs


def special_lists(par):
    """{kind: [loop with its closing pair, ...]} in table order, duplicates dropped (the first entry wins)"""
    out = {}
    for kind, name in enumerate(KINDS):
        seen = []
        for s, _, _ in par[name]:
            if s not in seen:
                seen.append(s)
        out[kind] = seen
    return out


# ---------------------------------------------------------------- which entries a structure reads

def pair_table(db):
    pt, stk = [-1] * len(db), []
    for i, c in enumerate(db):
        if c == "(":
            stk.append(i)
        elif c == ")":
            j = stk.pop()
            pt[i], pt[j] = j, i
    assert not stk
    return pt


def _stem(c, t, si1, sj1, ext):
    if si1 >= 0 and sj1 >= 0:
        c[("mismatch_exterior" if ext else "mismatch_multi", (t, si1, sj1))] += 1
    elif si1 >= 0:
        c[("dangle5", (t, si1))] += 1
    elif sj1 >= 0:
        c[("dangle3", (t, sj1))] += 1
    if t > 2:
        c[("term_au", ())] += 1
    if not ext:
        c[("ml_intern", ())] += 1


def _size(c, table, n):
    c[(table, (min(n, 30),))] += 1
    if n > 30:
        c[("lxc", (n,))] += 1            # the loop's size goes through lxc * log(n / 30)


def _intloop(c, n1, n2, t, t2, si1, sj1, sp1, sq1, ninio, max_ninio):
    nl, ns = max(n1, n2), min(n1, n2)
    if nl == 0:
        c[("stack", (t, t2))] += 1
    elif ns == 0:
        _size(c, "bulge", nl)
        if nl == 1:
            c[("stack", (t, t2))] += 1
        else:
            c[("term_au", ())] += (t > 2) + (t2 > 2)
    elif nl == 1:
        c[("int11", (t, t2, si1, sj1))] += 1
    elif ns == 1 and nl == 2:
        c[("int21", (t, t2, si1, sq1, sj1) if n1 == 1 else (t2, t, sq1, si1, sp1))] += 1
    elif ns == 2 and nl == 2:
        c[("int22", (t, t2, si1, sp1, sq1, sj1))] += 1
    else:
        c23 = ns == 2 and nl == 3
        _size(c, "interior", 5 if c23 else nl + ns)
        if c23 or (nl - ns) * ninio <= max_ninio:
            c[("ninio", ())] += 1 if c23 else nl - ns
        else:
            c[("max_ninio", ())] += 1
        mm = "mismatch_interior_1n" if ns == 1 else "mismatch_interior_23" if c23 else "mismatch_interior"
        c[(mm, (t, si1, sj1))] += 1
        c[(mm, (t2, sq1, sp1))] += 1


def reads(seq, db, special=None, ninio=60, max_ninio=300):
    """Counter of (table, index) -> number of times the energy of (seq, db) adds that entry.  `ninio`/`max_ninio` decide which
    of the two the asymmetry term reads (a positive ninio; the smaller value wins, ninio on a tie)."""
    special = special or {}
    S = [CODE[x] for x in seq]
    pt, L, c = pair_table(db), len(seq), Counter()
    p = 0
    while p < L:
        q = pt[p]
        if q < 0:
            p += 1
            continue
        _stem(c, TYPE[seq[p] + seq[q]], S[p - 1] if p > 0 else -1, S[q + 1] if q < L - 1 else -1, True)
        p = q + 1
    for i in range(L):
        j = pt[i]
        if j <= i:
            continue
        t = TYPE[seq[i] + seq[j]]
        br, p = [], i + 1
        while p < j:
            if pt[p] < 0:
                p += 1
                continue
            br.append((p, pt[p]))
            p = pt[p] + 1
        if not br:
            n = j - i - 1
            hit = None
            if n in (3, 4, 6):
                kind = {3: 0, 4: 1, 6: 2}[n]
                lst = special.get(kind, [])
                if seq[i:j + 1] in lst:
                    hit = ("special", (kind, lst.index(seq[i:j + 1])))
            if hit:
                c[hit] += 1
                continue
            _size(c, "hairpin", n)
            if n == 3:
                c[("term_au", ())] += t > 2
            elif n > 3:
                c[("mismatch_hairpin", (t, S[i + 1], S[j - 1]))] += 1
        elif len(br) == 1:
            p, q = br[0]
            _intloop(c, p - i - 1, j - q - 1, t, RT[TYPE[seq[p] + seq[q]]], S[i + 1], S[j - 1], S[p - 1], S[q + 1], ninio, max_ninio)
        else:
            u = j - i - 1
            for p, q in br:
                _stem(c, TYPE[seq[p] + seq[q]], S[p - 1], S[q + 1], False)
                u -= q - p + 1
            _stem(c, RT[t], S[j - 1], S[i + 1], False)
            c[("ml_closing", ())] += 1
            c[("ml_base", ())] += u
    return +c


# ---------------------------------------------------------------- loop cases

_FILL = "ACAUCCAAUC"


def filler(n, k=0):
    return "".join(_FILL[(k + i) % len(_FILL)] for i in range(n))


def _all_special(par=None):
    sp = special_lists(index_sensitive_par(par if par is not None else builtin_par()))
    return sp


def plain_hairpin(t, n, special, l5="A", l3="A"):
    """a hairpin of n >= 0 unpaired bases under a pair of type t whose loop is no special loop; its two ends as given"""
    if n == 0:
        return PT[t], "()"
    if n == 1:
        return PT[t][0] + l5 + PT[t][1], "(.)"
    flat = {s for lst in special.values() for s in lst}
    for k in range(len(_FILL)):
        s = PT[t][0] + l5 + filler(n - 2, k) + l3 + PT[t][1]
        if s not in flat:
            return s, "(" + "." * n + ")"
    raise AssertionError("no plain hairpin")


def hp(t=2):
    """the plain GAAA hairpin under a pair of type t"""
    return PT[t][0] + "GAAA" + PT[t][1], "(....)"


def interior(t, u, left, right):
    """the loop closed by a pair of type t whose inner pair makes the table's second pair index u (= the type of the inner pair read
    from the other side), with `left` / `right` unpaired on the two strands; the inner pair closes a GAAA hairpin"""
    s, d = hp(RT[u])
    return PT[t][0] + left + s + right + PT[t][1], "(" + "." * len(left) + d + "." * len(right) + ")"


GENERIC_SIZES = (2, 3, 4, 5, 10, 15, 16, 28)
ML_K = (2, 3, 4, 16, 17, 32, 33, 64, 65, 128, 129, 200)
HAIRPIN_SIZES = tuple(range(0, 36)) + (64, 200, 2000)
BULGE_SIZES = tuple(range(1, 33)) + (40,)
ONE_N_SIZES = tuple(range(2, 32)) + (40,)


def _with_n(s, k):
    return s[:k] + "N" + s[k + 1:]


def loop_cases(par=None):
    """every case of the issue's list; the special loops are those of index_sensitive_par (the built-in ones plus six)"""
    special = _all_special(par)
    out = []
    add = lambda name, target, sd: out.append((name, target, sd[0], sd[1]))
    bs = lambda *codes: "".join(B[x] for x in codes)

    # ---- hairpins
    for n in HAIRPIN_SIZES:
        add(f"hairpin/size{n}", ("hairpin", (min(n, 30),)), plain_hairpin(2, n, special))
    for n in (4, 5):
        for t in TYPES:
            for a in ACGU:
                for b in ACGU:
                    add(f"hairpin/mm/size{n}/{PT[t]}/{B[a]}{B[b]}", ("mismatch_hairpin", (t, a, b)), plain_hairpin(t, n, special, B[a], B[b]))
    for t in TYPES:
        add(f"hairpin/size3/{PT[t]}", ("term_au", ()) if t > 2 else ("hairpin", (3,)), plain_hairpin(t, 3, special))
    flat = {s for lst in special.values() for s in lst}
    for kind, lst in special.items():
        for k, s in enumerate(lst):
            add(f"hairpin/special/{s}", ("special", (kind, k)), (s, "(" + "." * (len(s) - 2) + ")"))
            miss = None
            for pos in range(2, len(s) - 2):                       # an inner base of the loop: not its first, not its last
                for x in "ACGU":
                    cand = s[:pos] + x + s[pos + 1:]
                    if cand not in flat:
                        miss = cand
                        break
                if miss:
                    break
            assert miss, s
            t = TYPE[s[0] + s[-1]]
            target = ("mismatch_hairpin", (t, CODE[s[1]], CODE[s[-2]])) if len(s) > 5 else (("term_au", ()) if t > 2 else ("hairpin", (3,)))
            add(f"hairpin/near_miss/{s}/{miss}", target, (miss, "(" + "." * (len(s) - 2) + ")"))

    # ---- stacks and bulges
    for t in TYPES:
        for u in TYPES:
            add(f"stack/{PT[t]}/{u}", ("stack", (t, u)), interior(t, u, "", ""))
    for n in BULGE_SIZES:
        add(f"bulge/left{n}", ("bulge", (min(n, 30),)), interior(2, 1, filler(n, n), ""))
        add(f"bulge/right{n}", ("bulge", (min(n, 30),)), interior(2, 1, "", filler(n, n + 3)))
    for n in (1, 2):
        for t in TYPES:
            for u in TYPES:
                target = ("stack", (t, u)) if n == 1 else (("term_au", ()) if (t > 2 or u > 2) else ("bulge", (2,)))
                add(f"bulge/types/left{n}/{t}/{u}", target, interior(t, u, filler(n, t + u), ""))
                add(f"bulge/types/right{n}/{t}/{u}", target, interior(t, u, "", filler(n, t + u)))

    # ---- interior loops: the tabulated ones
    for t in TYPES:
        for u in TYPES:
            for a in ACGU:
                for b in ACGU:
                    add(f"int11/{t}/{u}/{B[a]}{B[b]}", ("int11", (t, u, a, b)), interior(t, u, B[a], B[b]))
                    for c in ACGU:
                        add(f"int21/n1/{t}/{u}/{B[a]}{B[b]}{B[c]}", ("int21", (t, u, a, b, c)), interior(t, u, B[a], bs(b, c)))
                        add(f"int21/n2/{t}/{u}/{B[a]}{B[b]}{B[c]}", ("int21", (t, u, a, b, c)), interior(u, t, bs(b, c), B[a]))
                        for d in ACGU:
                            add(f"int22/{t}/{u}/{B[a]}{B[b]}{B[c]}{B[d]}", ("int22", (t, u, a, b, c, d)), interior(t, u, bs(a, b), bs(c, d)))

    # ---- 1 x n, 2 x 3, generic
    for n in ONE_N_SIZES:
        for side in ("1xn", "nx1"):
            l, r = ("C", filler(n, n)) if side == "1xn" else (filler(n, n), "C")
            if n == 2:
                sd = interior(2, 1, l, r)
                target = [k for k in reads(*sd) if k[0] == "int21"][0]
            else:
                sd, target = interior(2, 1, l, r), ("interior", (min(n + 1, 30),))
            add(f"int{side}/{n}", target, sd)
    for name, table, shapes in (("1x3", "mismatch_interior_1n", ((1, 3), (3, 1))), ("2x3", "mismatch_interior_23", ((2, 3), (3, 2))),
                                ("3x3", "mismatch_interior", ((3, 3), (4, 6)))):
        for n1, n2 in shapes:
            for t in TYPES:
                for a in ACGU:
                    for b in ACGU:
                        # outer end: si1 = first base of the left strand, sj1 = last base of the right strand
                        l, r = B[a] + filler(n1 - 1, a), filler(n2 - 1, b) + B[b]
                        add(f"{name}/outer/{n1}x{n2}/{t}/{B[a]}{B[b]}", (table, (t, a, b)), interior(t, 1 + (t + a + b) % 6, l, r))
                        # inner end: sq1 = first base of the right strand, sp1 = last base of the left strand
                        l, r = filler(n1 - 1, a) + B[b], B[a] + filler(n2 - 1, b)
                        add(f"{name}/inner/{n1}x{n2}/{t}/{B[a]}{B[b]}", (table, (t, a, b)), interior(1 + (t + a + b) % 6, t, l, r))
    for n1 in GENERIC_SIZES:
        for n2 in GENERIC_SIZES:
            sd = interior(2, 1, filler(n1, n1), filler(n2, n2 + 5))
            if (n1, n2) == (2, 2):
                target = [k for k in reads(*sd) if k[0] == "int22"][0]
            elif (n1, n2) in ((2, 3), (3, 2)):
                target = ("interior", (5,))
            else:
                target = ("interior", (min(n1 + n2, 30),))
            add(f"generic/{n1}x{n2}", target, sd)

    # ---- multiloops
    for k in ML_K:
        for gap, g in (("adjacent", 0), ("spaced", 1)):
            s, d = "G" + filler(g, k), "(" + "." * g
            for j in range(k):
                hs, hd = hp(TYPES[j % 6])
                s += hs + filler(g + (j % 3 if g else 0), j)
                d += hd + "." * (g + (j % 3 if g else 0))
            add(f"multi/{k}/{gap}", ("ml_intern", ()), (s + "C", d + ")"))
    for t in TYPES:
        for a in ACGU:
            for b in ACGU:
                hs, hd = hp(t)
                h2, d2 = hp(2)
                add(f"multi/branch_mm/{t}/{B[a]}{B[b]}", ("mismatch_multi", (t, a, b)),
                    ("G" + B[a] + hs + B[b] + "A" + h2 + "A" + "C", "(." + hd + ".." + d2 + ".)"))
                # closing pair: read from inside, type rtype(closing), neighbours S[cj - 1], S[ci + 1]
                c5, c3 = PT[RT[t]]
                add(f"multi/closing_mm/{t}/{B[a]}{B[b]}", ("mismatch_multi", (t, a, b)),
                    (c5 + B[b] + h2 + "A" + h2 + B[a] + c3, "(." + d2 + "." + d2 + ".)"))

    # ---- exterior loop
    add("ext/1", ("none", ()), ("A", "."))
    add("ext/2", ("none", ()), ("AC", ".."))
    for t in TYPES:
        hs, hd = hp(t)
        add(f"ext/both_ends/{t}", ("term_au", ()) if t > 2 else ("hairpin", (4,)), (hs, hd))
        for a in ACGU:
            add(f"ext/5p_end/{t}/{B[a]}", ("dangle3", (t, a)), (hs + B[a], hd + "."))
            add(f"ext/3p_end/{t}/{B[a]}", ("dangle5", (t, a)), (B[a] + hs, "." + hd))
            for b in ACGU:
                add(f"ext/middle/{t}/{B[a]}{B[b]}", ("mismatch_exterior", (t, a, b)), (B[a] + hs + B[b], "." + hd + "."))
        for u in TYPES:
            us, ud = hp(u)
            add(f"ext/adjacent2/{t}/{u}", ("dangle3", (t, CODE[us[0]])), (hs + us, hd + ud))
            add(f"ext/adjacent3/{t}/{u}", ("mismatch_exterior", (t, CODE[us[-1]], CODE[us[0]])), (us + hs + us, ud + hd + ud))

    # ---- N as each of the four neighbours, in one loop of every kind
    def n_target(sd):
        ks = [k for k in reads(*sd, special=special) if k[0] not in ("stack", "hairpin", "bulge", "interior", "special") + SCALARS + ("lxc",)
              and 0 in k[1][(2 if k[0].startswith("int") else 1):]]
        assert len(ks) >= 1, sd
        return sorted(ks)[0]
    for n1, n2 in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 4), (4, 1), (2, 3), (3, 2), (3, 4)):
        l, r = filler(n1, 1), filler(n2, 2)
        for where, (ll, rr) in (("si1", (_with_n(l, 0), r)), ("sp1", (_with_n(l, n1 - 1), r)), ("sq1", (l, _with_n(r, 0))), ("sj1", (l, _with_n(r, n2 - 1)))):
            sd = interior(3, 6, ll, rr)
            add(f"N/{n1}x{n2}/{where}", n_target(sd), sd)
    for n in (4, 7):
        for where, k in (("l5", 1), ("l3", n)):
            s, d = plain_hairpin(5, n, special)
            sd = (_with_n(s, k), d)
            add(f"N/hairpin{n}/{where}", n_target(sd), sd)
    h2, d2 = hp(2)
    for where, k in (("branch5", 1), ("branch3", 8), ("closing5", 1), ("closing3", 15)):
        s, d = "GA" + h2 + "A" + h2 + "AC", "(." + d2 + "." + d2 + ".)"
        sd = (_with_n(s, k), d)
        add(f"N/multi/{where}", n_target(sd), sd)
    for where, s, d in (("ext5", "N" + h2 + "A", "." + d2 + "."), ("ext3", "A" + h2 + "N", "." + d2 + "."), ("d5", "N" + h2, "." + d2), ("d3", h2 + "N", d2 + ".")):
        add(f"N/{where}", n_target((s, d)), (s, d))
    # a structure two families arrive at (the 1 x 2 loop of the 1 x n series is an int21 case) is kept once, under its first name
    seen, uniq = set(), []
    for c in out:
        if (c[2], c[3]) not in seen:
            seen.add((c[2], c[3]))
            uniq.append(c)
    return uniq


def table_sizes():
    """number of entries over the six pair types and ACGU (sizes: those the cases must reach) per table"""
    out = {"stack": 36, "dangle5": 24, "dangle3": 24, "int11": 576, "int21": 2304, "int22": 9216, "hairpin": 31, "bulge": 30, "interior": 27}
    for k in MM_TABLES:
        out[k] = 96
    return out


# ---------------------------------------------------------------- malformed rows

def bad_rows():
    """(name, seq, db, kind): kind "struct" (malformed dot-bracket, found on the host), "char" (a letter outside ACGUN) or "pair" (a
    non-canonical or N-containing pair, found by the evaluator in the named loop)"""
    h2, d2 = hp(2)
    out = [("unbalanced_open", "GGGAAACCC", "(((....))", "struct"), ("unbalanced_close", "GGGAAACCC", "((....)))", "struct"),
           ("foreign_char", "GGGAAACCC", "((.x...))", "struct"), ("length", "GGGAAACCC", "((....))", "struct"),
           ("lowercase", "gggaaaccc", "(((...)))", "char"), ("T", "GGGTAACCC", "(((...)))", "char")]
    for tag, x, y in (("noncanonical", "A", "A"), ("N5", "N", "C"), ("N3", "G", "N")):
        bad, bd = x + "GAAA" + y, "(....)"
        out += [(f"pair/{tag}/hairpin", "G" + bad + "C", "(" + bd + ")", "pair"),
                (f"pair/{tag}/interior_inner", "GA" + x + h2 + y + "AC", "(.(" + d2 + ").)", "pair"),
                (f"pair/{tag}/multi_branch", "G" + bad + "A" + h2 + "C", "(" + bd + "." + d2 + ")", "pair"),
                (f"pair/{tag}/multi_closing", x + "A" + h2 + "A" + h2 + y, "(." + d2 + "." + d2 + ")", "pair"),
                (f"pair/{tag}/exterior_branch", "A" + h2 + "A" + x + h2 + y + "A", "." + d2 + ".(" + d2 + ").", "pair")]
    return out


# ---------------------------------------------------------------- parents for the expand seam

PARENT_K = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
PARENT_G = (1, 2, 5)
PARENT_EXTRA = ((200, 6),)        # (k + 1) g = 1206: no (k, g) of the two lists above reaches the 1024-position class limit


def _segment(i, k, g):
    """the g unpaired bases of segment i of k + 1.  Most segments are A and pair with nothing but segment 1, the only U segment: on
    lag 1 + j the one candidate is the stem between segments 1 and j, which encloses j - 1 branches - every count up to k - 1 comes up.
    G segments (2, and 3 mod 7) and C segments (6 mod 7) add G-U and G-C stems that win their lags by score, and a stem that
    runs from the end of segment 1 into segment 2 on one strand and from segment 7m into 7m - 1 on the other has a branch inside
    each strand.  The last segment is mixed: stems inside it enclose no branch."""
    if i == k and g >= 2:
        return ("AUAUG" * g)[:g] if k else ("GGAUCCAUC" * g)[:g]
    if i == 1:
        return "U" * g
    if i == 2 or i % 7 == 3:
        return "G" * g
    if i % 7 == 6:
        return "C" * g
    return "A" * g


def parent(k, g, closing):
    """k hairpin branches with mixed outer pairs and g unpaired bases around each, in the exterior loop (closing 0) or under a pair of
    type `closing` -> (seq, db, positions of the loop's unpaired bases)"""
    s, d = "", ""
    for i in range(k + 1):
        seg = _segment(i, k, g)
        s += seg
        d += "." * g
        if i < k:
            t = TYPES[(i * 5 + i // 6) % 6]
            if i % 4 == 2:                      # some branches are two pairs deep
                hs, hd = PT[t][0] + hp(2)[0] + PT[t][1], "(" + hp(2)[1] + ")"
            else:
                hs, hd = hp(t)
            s += hs
            d += hd
    if closing:
        s, d = PT[closing][0] + s + PT[closing][1], "(" + d + ")"
    pt = pair_table(d)
    lo, hi = (1, len(s) - 1) if closing else (0, len(s))
    pos, p = [], lo
    while p < hi:
        if pt[p] < 0:
            pos.append(p)
            p += 1
        else:
            p = pt[p] + 1
    assert len(pos) == (k + 1) * g
    return s, d, pos


def parent_cases(ks=PARENT_K):
    for k in ks:
        for g in PARENT_G + tuple(g for kk, g in PARENT_EXTRA if kk == k):
            for closing in (0,) + TYPES:
                s, d, pos = parent(k, g, closing)
                yield f"parent/k{k}/g{g}/{PT[closing] if closing else 'ext'}", s, d, pos


def branches_of(db, pos):
    """outermost pairs (p, q) of the helices hanging in the loop whose unpaired positions are `pos`"""
    pt = pair_table(db)
    out = []
    # the enclosing pair, if any: nearest pair around pos[0]
    lo, depth = -1, 0
    for x in range(pos[0] - 1, -1, -1):
        if pt[x] < 0:
            continue
        if pt[x] < x:
            depth += 1
        elif depth:
            depth -= 1
        else:
            lo = x
            break
    hi = pt[lo] if lo >= 0 else len(db)
    p = lo + 1
    while p < hi:
        if pt[p] < 0:
            p += 1
        else:
            out.append((p, pt[p]))
            p = pt[p] + 1
    return out
