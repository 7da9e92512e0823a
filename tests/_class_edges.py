"""Constructed parents and folds on the span and branch-count edges of the expand classes (test infrastructure; pure Python: no
GPU, no oracle).

`node_class()` (rafft_amd/csrc/rafft_kernels.h) routes a region by its number of unpaired positions n, by the span of its loop
(closing pair to closing pair: what the kernel stages in LDS) and by its number of branch helices.  The n edges are pinned by
tests/test_gpu_ties.py; this module builds loops on the other two:

* `span_parents()`: one loop under a pair (ci, cj) of exactly the wanted span - SM_SPAN = 448 of the small-region kernel,
  CLS01_L = 1280 of the one-wavefront class, one below and one above each - at every ci mod 4, at the 5' end of its sequence, at
  the 3' end of a 4096-nt one and of a 4097-nt one (there the span becomes the sequence and the routing changes).
* `tail_parents()`: small loops whose closing pair starts beyond position 4000 of a 4096-nt sequence (the staged bases are
  addressed through a pointer shifted back by ci).
* `branch_parents()`: k minimal hairpins in one loop, k on both sides of 256, of MAX_BR = 1024 and at BIG_BR = 4095; at 1024 once
  more with 1024 positions, the full branch list of the 256-thread class.
* `onions()`: sequences whose fold is forced through a loop of a given (n, span, 1), and `loops_of()`, the dot-bracket loop walker
  that says which loops a structure has.

Every parent is (name, seq, db, pos, want): `want` is the class the parent is built for under the seam's limits (teams of 16 / 32
lanes for up to 16 / 32 positions, nb_mode 100), and `None` where the call must be refused.
"""
import numpy as np

from _loops import filler, pair_table

SM_SPAN, CLS01_L, MAX_BR, BIG_BR, LDS_SEQ = 448, 1280, 1024, 4095, 4096      # rafft_kernels.h
COMP = {"A": "U", "U": "A", "G": "C", "C": "G"}

SMALL_SPANS = (SM_SPAN - 1, SM_SPAN, SM_SPAN + 1)
WAVE_SPANS = (CLS01_L - 1, CLS01_L, CLS01_L + 1)
SMALL_N = (16, 32)             # n <= 16: teams of 16 lanes; 17 <= n <= 32: teams of 32
WAVE_N = (33, 256)             # both ends of 33 <= n <= 256, what the one-wavefront class takes beyond the small teams
PLACES = ("5p", "3p4096", "3p4097")
BRANCH_K = (255, 256, 257, 1023, 1024, 1025, 4094, 4095)
BRANCH_G = (1, 2)


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def _ends(n, seed, letters="GCGCAU", off=(0, 0), even=False, cap=10 ** 6):
    """the unpaired bases at the two ends of a loop, n in all, split unevenly unless `even`: m bases of the 5' end, drawn from `letters`, pair with m
    of the 3' end (a G-U wobble now and then, never in the outermost two pairs); the outermost pair lies off[0] bases behind the
    start of the 5' end and off[1] bases before the end of the 3' end, everything else is A"""
    rng = np.random.default_rng(seed)
    a = n // 2 - (1 if n % 4 == 0 and not even else 0)
    b = n - a
    m = min(min(a - off[0], b - off[1]) - (1 if n >= 8 else 0), cap)
    left = "".join(rng.choice(list(letters), m))
    right = list(revcomp(left))
    for x in range(len(right) - 2):
        if right[x] == "C" and rng.random() < 0.25:
            right[x] = "U"
    return "A" * off[0] + left + "A" * (a - off[0] - m), "A" * (b - off[1] - m) + "".join(right) + "A" * off[1]


def _fill(F, two):
    """F nt of branch helices: a four-pair hairpin with a long loop, behind a GAAAC hairpin when `two`"""
    assert F >= 11 + (5 if two else 0)
    s, d = ("GAAAC", "(...)") if two else ("", "")
    F -= len(s)
    return s + "GCGG" + filler(F - 8, F) + "CCGC", d + "((((" + "." * (F - 8) + "))))"


def span_loop(span, n, seed, two=False):
    """(seq, db, region positions relative to ci) of one loop under a G-C pair: span nt from closing pair to closing pair, n unpaired
    positions at its two ends, one or two branch helices between them"""
    u5, u3 = _ends(n, seed)
    fs, fd = _fill(span - 2 - n, two)
    s = "G" + u5 + fs + u3 + "C"
    d = "(" + "." * len(u5) + fd + "." * len(u3) + ")"
    assert len(s) == len(d) == span
    pos = list(range(1, 1 + len(u5))) + list(range(span - 1 - len(u3), span - 1))
    return s, d, pos


def place(loop, where, r):
    """the loop at the 5' end behind r unpaired bases, or at the 3' end of a sequence of exactly 4096 / 4097 nt with ci mod 4 = r"""
    s, d, pos = loop
    if where == "5p":
        head, tail = r, 0
    else:
        L = int(where[2:])
        tail = (L - len(s) - r) % 4
        head = L - len(s) - tail
        assert head >= 0 and head % 4 == r
    seq = filler(head, 3) + s + filler(tail, 7)
    db = "." * head + d + "." * tail
    return seq, db, [head + p for p in pos]


def _span_want(span, n, where):
    if where == "3p4097":
        return 2                       # no LDS copy of the bases, no small teams: the 256-thread class whatever the loop
    if span <= SM_SPAN and n <= 32:
        return 4 if n <= 16 else 5
    return 1 if span <= CLS01_L else 2


def span_parents(spans=SMALL_SPANS + WAVE_SPANS):
    for span in spans:
        for n in (SMALL_N if span < 1000 else WAVE_N):
            for r in range(4):
                loop = span_loop(span, n, 1000 * span + 10 * n + r, two=r & 1)
                for where in PLACES:
                    seq, db, pos = place(loop, where, r)
                    yield f"span/{span}/n{n}/ci{r}/{where}", seq, db, pos, _span_want(span, n, where)


TAIL_SHAPES = ((40, 16, 4), (61, 32, 5), (90, 40, 1), (92, 64, 1))       # (span, n, class): cj is the last base or near it


def tail_parents():
    for span, n, want in TAIL_SHAPES:
        for r in range(4):
            seq, db, pos = place(span_loop(span, n, 77 * span + r, two=r & 1), "3p4096", r)
            assert pos[0] - 1 >= 4000
            yield f"tail/{span}/n{n}/ci{r}", seq, db, pos, want


# ---------------------------------------------------------------- many branches in one loop

def _marked(k):
    """which of the k + 1 segments hold pairing bases (every other one is N and pairs with nothing: the few lags with a stem are
    ranked whatever nb_mode, and every stem's branch count is known).  A stem between segments a < b encloses b - a branches:
    G0-C4 4, G3-C4 and A1-U2 one, G0-C(k-1) k - 1, G0-Ck all k; the others spread over the range between."""
    m = {}
    for i in (0, 3, k // 3, k // 2 - 5):
        m[i] = "G"
    for i in (4, 2 * k // 3 + 5, k - 1, k):
        m[i] = "C"
    for i in (1, 7, k // 4, k - 7):
        m[i] = "A"
    for i in (2, 9, 3 * k // 4 + 11, k - 3):
        m[i] = "U"
    assert len(m) == 16 and 11 not in m
    m[11] = "GC"                       # (g = 2: the one stem inside a segment - it encloses no branch; no other two marked segments share its lag)
    return m


def branch_parent(k, g, closing, last=True):
    """k GAAAC-like hairpins (mixed outer pairs, every fourth two pairs deep) with g unpaired bases around each (none behind the last
    one unless `last`), in the exterior loop or under a G-C pair -> (seq, db, region positions)"""
    pairs = ("GC", "CG", "GU", "UG", "AU", "UA")
    m = _marked(k)
    s, d, pos = [], [], []
    at = 1 if closing else 0
    for i in range(k + 1):
        seg = (m.get(i, "N") * g)[:g] if i < k or last else ""
        pos.extend(range(at, at + len(seg)))
        s.append(seg)
        d.append("." * len(seg))
        at += len(seg)
        if i < k:
            p = pairs[(i * 5 + i // 6) % 6]
            hs, hd = p[0] + "AAA" + p[1], "(...)"
            if i % 4 == 2:
                hs, hd = "G" + hs + "C", "(" + hd + ")"
            s.append(hs)
            d.append(hd)
            at += len(hs)
    seq, db = "".join(s), "".join(d)
    if closing:
        seq, db = "G" + seq + "C", "(" + db + ")"
    assert len(pos) == (k + 1 if last else k) * g
    return seq, db, pos


def _branch_want(k, g):
    if k > BIG_BR:
        return None
    if k > MAX_BR:
        return 0
    return 2 if (k + 1) * g <= 1024 else 3        # (FFT size of 2n - 1 lags up to 2048 | beyond; the span is far beyond CLS01_L)


def branch_parents(ks=BRANCH_K, gs=BRANCH_G):
    for k in ks:
        for g in gs:
            for closing in (False, True):
                seq, db, pos = branch_parent(k, g, closing)
                yield f"branches/k{k}/g{g}/{'GC' if closing else 'ext'}", seq, db, pos, _branch_want(k, g)
        if k == MAX_BR:
            # the only way to MAX_BR branches within the 1024 positions of the 256-thread class: no unpaired base behind the last helix
            for closing in (False, True):
                seq, db, pos = branch_parent(k, 1, closing, last=False)
                yield f"branches/k{k}/g1/{'GC' if closing else 'ext'}/full_list", seq, db, pos, 2


def stem_branch_counts(db, pos, node):
    """how many of the loop's branches every ranked stem of an expansion `node` encloses (None: the lag gave no stem)"""
    from _loops import branches_of
    br = branches_of(db, pos)
    out = []
    for nb, mi, mj in zip(node["nb"], node["mi"], node["mj"]):
        if nb <= 0:
            out.append(None)
            continue
        a, b = pos[mi], pos[mj]
        out.append(sum(1 for p, q in br if a < p and q < b))
    return out


# ---------------------------------------------------------------- whole folds through a loop on a span edge

ONION_SPANS = (SM_SPAN, SM_SPAN + 1, CLS01_L, CLS01_L + 1)
ONION_N = (16, 32, 40)
CLAMP2 = "GCCGGCGCCG"
ONION_PARAMS = ((100, 1, 100), (100, 3, 100))       # (nb_mode, max_stack, max_branch) the onions are folded with


def onion(span, n, r, fill="N"):
    """r unpaired bases, a 12-nt G clamp, u5, a second clamp around `fill`, u3, the 12-nt C clamp, 3 - r more bases: once both clamps
    are closed, the loop between them has n unpaired positions, one branch and `span` nt from its closing pair to its closing pair.
    The three helices are coaxial (one lag holds them all: it is ranked among the nb_mode best whatever the length of the filler)
    and an A.A mismatch apart, so each closes in a step of its own, the clamps first.  u5 is A and G, u3 is U and C: neither pairs
    with itself,
    and their helix is six pairs at the most: weaker than either clamp."""
    assert n % 2 == 0
    u5, u3 = _ends(n, 31 * span + n + r, "AAG", (1, 1), even=True, cap=6)
    F = span - 2 - n - 2 * len(CLAMP2)
    assert F >= 3
    return "ACA"[:r] + "G" * 12 + u5 + CLAMP2 + fill * F + revcomp(CLAMP2) + u3 + "C" * 12 + "A" * (3 - r)


def onions(fill="N"):
    for span in ONION_SPANS:
        for n in ONION_N:
            for r in range(4):
                yield f"onion/{span}/n{n}/flank{r}/{fill}", onion(span, n, r, fill), (n, span, 1)


def loops_of(db):
    """{(n unpaired positions, span, branches)} of every loop under a pair (span: closing pair to closing pair), and of the exterior
    loop with the whole row as its span"""
    pt = pair_table(db)
    out = set()

    def walk(lo, hi, span):
        n = nbr = 0
        p = lo
        while p < hi:
            if pt[p] < 0:
                n += 1
                p += 1
            else:
                nbr += 1
                walk(p + 1, pt[p], pt[p] + 1 - p)
                p = pt[p] + 1
        out.add((n, span, nbr))

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), len(db) + 100))
    walk(0, len(db), len(db))
    return out
