"""Dimers for the edges of rafft_cofold_batch that folded random dimers never take, and the mirror's results on them (test
infrastructure; pure Python / numpy: no GPU, no product code apart from what `_loops.builtin_par` uses).  DESIGN.md section 22.

The loops over a strand end - FA over the stems (i,j) with j ascending from i + 4, FB over the stems (i,j) with i ascending from
c, in the fill and in the traceback - run as `for (x = first + lane; x <= last; x += 64)`: they take round r when the strand has
more than 64 (r - 1) candidates, and their values reach the energy only through the loop that holds the nick.

* `third_round_cases()`: dimers whose nick loop holds a stem of one strand that only a candidate of the third round reaches - an FA
  stem of span 132 or more, an FB stem that begins 128 positions or more after c - in both size classes (up to RAFFT_MFE_LDS_LEN =
  146 nt and above), under the built-in tables and where multiloops win, and a random dimer of two strands of 140 nt.
  `CutMirror(defect="fa_two_rounds" / "fb_two_rounds")` states what a loop of two rounds computes: tests/test_cofold_cases.py shows
  that each case tells it from the right one.
* `tie_cases()`: dimers for the flat tables tie0 and tie1, under which many structures share the minimum and only the candidate
  order of the traceback decides the row: random ones of 40-150 nt, homodimers, repeats, dimers found by a scan of random G/C/U-rich
  dimers for ties in the nick loop, and constructed ones.  Under the flat tables a hairpin of n pairs costs 400 - 100 n, an exterior
  stem nothing, and a cross pair on top of another -100:
  - A9 pairs with U9 around a nick loop that holds a hairpin, on strand A (A9 first) or on strand B (U9 first), with the hairpin
    loop ACCA and a C before it on strand A, so that U9 finds no second run of nine partners among A and G.  G5 and C6: the FA
    stem at its first G ends at one of two C; G6 and C5: the FB stem at its last C begins at one of two G; G4 and C4: the
    hairpin costs 0 and ties with "unpaired".
  - a cross helix of six pairs around a hairpin and a C and a G that can pair across the nick: that lone pair costs nothing where
    multiloops cost nothing, so the nick loop ties with the split that makes it a multiloop.
* `sweep_cases()`: one 48-nt sequence at every cut, the 133-nt sequence of _lane_rounds at the cuts around 64 and 128.
* `limit_cases()`: random dimers of RAFFT_MFE_LDS_LEN and one more, cut near both ends and in the middle.
* one cache of the mirrors and their results per process: `fold` computes a (tables, dimer, order) once, whichever file asks first.
"""
import numpy as np

import _cofold_np as CF
import _lane_rounds as LR
import _par_reader as PR

DINIT = 410
SEED = 22
LDS_LEN = 146                   # RAFFT_MFE_LDS_LEN


def par_of(which):
    """the parameter set `which` of _lane_rounds with DuplexInit DINIT, as a .par file of the GPU tests holds it"""
    par = dict(LR.par_sets()[which])
    par.update(duplex_init=DINIT, duplex_init_dH=3 * DINIT + 70)
    return par


def mirror(which, defect=None):
    return LR._once(("CutMirror", which, defect), lambda: CF.CutMirror(PR.tables_at(par_of(which), 37.0), DINIT, defect))


def fold(which, seq, c, order="first"):
    """((dcal, row, n_inter), ties) of CutMirror.fold_cut"""
    def make():
        m = mirror(which)
        return m.fold_cut(seq, c, order), dict(m.ties)
    return LR._once(("fold_cut", which, seq, c, order), make)


def swapped(dimers):
    return [(s[c:] + s[:c], len(s) - c) for s, c in dimers]


def backwards(dimer):
    s, c = dimer
    return s[::-1], len(s) - c


def _rand(rng, n, letters="ACGU"):
    return "".join(rng.choice(list(letters), n))


# ---- (a) the third round of FA and FB

def third_round_cases():
    """[(name, table set, seq, cut, kind)]: kind "fa" / "fb" - the strand-end loop whose third round the optimum needs - or None"""
    hp = lambda n, m=None: "G" * n + "AAAA" + "C" * (m or n)
    built = [("fa_lds", "GCGAGC" + "GGGGGG" + "A" * 121 + "CCCCCC", "GCUCGC", "fa"),
             ("fb_lds", "GCGC", "A" * 128 + hp(3) + "GCGC", "fb"),
             ("fa_hbm", "GCGAGCGA" + "GGGGGG" + "A" * 60 + hp(4) + "A" * 60 + "CCCCCC" + "A", "UCGCUCGC", "fa"),
             ("fb_hbm", "GCGAGCGA", "A" * 130 + hp(5) + "A" + "UCGCUCGC", "fb")]
    wins = [("fa_wins", "GGGGGGGCCC" + "A" * 127 + "GGGCCC", "CCCC", "fa"),
            ("fb_wins", "CGGG", "A" * 129 + "GGGGGGC" + "AAAA" + "GCCCCCC" + "CCCG", "fb")]
    out = [(name, "builtin", a + b, len(a), kind) for name, a, b, kind in built]
    out += [(name, "multiloops_win", a + b, len(a), kind) for name, a, b, kind in wins]
    return out + [("random_280", "builtin", _rand(np.random.default_rng(SEED), 280), 140, None)]


# ---- (b) ties

FOUND = ("UUUUUUUUUGGUGUUGGGGUUGUGGUGUGUUGUGGUGUGU&UGGGUUGUUGUGUGUG",            # nick loop against interior loop
         "CCCCGGCCCGGCACACACGCGGAGAAGCG&AACGCAAGAAGGGGGCGCGAACGACCAGCCGGGACAG",
         "CUUGGGCCGUCCUUGGCUUGCUUCCUGG&CGCUGUUCCCCUCGUGGGCUGUUGGUCU",
         "CGGCGGCGGCGGGGCGCGGG&CGGCGCGGGGCCCCCCGGGCGGG",
         "GGUAUUUGAUAUUAUUCGGAAGCUUAAGCCUCA&GUAGAUAACCGCCUUUCGAUGUGUCG",
         "CGGCGGGCGGGCGGCGGCGCGCGCGGCCGCC&GGCCCGCGCC",                            # FA
         "GGCUUUCAAAGCAUAGUAAGAGGACGAAACGUCGGG&UCUUGCCUGCUUUCC",
         "GGUCGGCGCGUCC&GGGGCCUUGUCCGGGGCGUGCCCGGCUGU")                           # FB
HOMO = 3                        # tie_cases()["homo0" .. ] are h + h; "het_ab" and "het_ba" hold two different strands both ways


def tie_cases():
    """{name: (seq, cut)}, for tie0 and tie1 alike"""
    rng = np.random.default_rng(7)
    out = {}
    for n, c in ((40, 17), (56, 30), (72, 36), (90, 64), (110, 40), (150, 70)):
        out["random%d" % n] = (_rand(rng, n), c)
    for k, n in enumerate((20, 31, 44)):
        h = _rand(rng, n)
        out["homo%d" % k] = (h + h, n)
    h1, h2 = _rand(rng, 25), _rand(rng, 33)
    out.update(het_ab=(h1 + h2, 25), het_ba=(h2 + h1, 33), gc30=("GC" * 30, 30), cug_cag=("CUG" * 14 + "CAG" * 14, 42))
    for n, c in ((48, 20), (64, 33)):
        out["gu%d" % n] = (_rand(rng, n, "GU"), c)
    for n, c in ((50, 25), (70, 30)):
        out["gc%d" % n] = (_rand(rng, n, "GC"), c)
    out["hairpins"] = ("GGGAAACCC" * 6, 27)
    on_a = lambda hairpin: ("A" * 9 + "C" + hairpin + "A" + "AAA" + "U" * 9, 9 + 1 + len(hairpin) + 1)
    on_b = lambda hairpin: ("U" * 9 + "AAA" + "A" + hairpin + "A" + "A" * 9, 12)
    out["fa_two_stems"], out["fb_two_stems"] = on_a("GGGGG" + "ACCA" + "CCCCCC"), on_b("GGGGGG" + "ACCA" + "CCCCC")
    out["fa_unpaired"], out["fb_unpaired"] = on_a("GGGG" + "ACCA" + "CCCC"), on_b("GGGG" + "ACCA" + "CCCC")
    a, b = "GGGGGG" + "A" + "CCCCCAAAAGGGGG" + "A" + "C" + "A", "A" + "G" + "A" + "CCCCCC"
    out["nick_or_split"] = (a + b, len(a))
    out["nick_or_split_backwards"] = backwards(out["nick_or_split"])
    for k, text in enumerate(FOUND):
        out["found%d" % k] = (text.replace("&", ""), text.index("&"))
    return out


# ---- (c) every cut

SWEEP_CUTS_133 = (1, 63, 64, 65, 127, 128, 129, 132)


def sweep_cases():
    """[(seq, cut)]: 48 nt (G/C-rich, so that most cuts leave pairs between the strands) at the cuts 1 .. 47, then 133 nt"""
    s48 = _rand(np.random.default_rng(SEED + 1), 48, "GGCCAU")
    return [(s48, c) for c in range(1, 48)] + [(LR.RANDOM_SEQS[0], c) for c in SWEEP_CUTS_133]


# ---- (d) the limit of the LDS class

def limit_cases():
    """[(seq, cut)]: three dimers of LDS_LEN nt, then two of LDS_LEN + 1"""
    rng = np.random.default_rng(SEED + 2)
    return [(_rand(rng, LDS_LEN), c) for c in (4, 73, 142)] + [(_rand(rng, LDS_LEN + 1), c) for c in (4, 73)]
