"""Problems that take rafft_findpath_batch past 64 moves and past 64 beam states, and the mirrors' results on them (test
infrastructure; pure Python / numpy and the oracle: no GPU, no product code).  DESIGN.md section 13.

The loops of rafft_findpath.hip run in rounds of 64 lanes - the moves offered, the ranks compared for duplicates - over masks of
fp_mask_words(d) = ceil(d / 64) words.  Random short problems (d <= 10) stay in round one and word one.

* `removal_cases()` (a): n hairpins of k pairs, stems drawn over G, C, A and U, opened to the open chain: d = 64 (one word, move 63
  its last bit), 65 (the first d of two words), 66 and 70, at widths 64, 65, 66 and 80 (at 88 and above the duplicates
  that a mark in the wrong word leaves on the d = 70 problem only narrow the beam; the wider beams are those of (c)).
* `addition_cases()` (b): units G^10 AAAA Y^10 (Y drawn from C and U) whose helix (i, 23 - i) slips to (i + 1, 23 - i): every
  addition waits for two removals, and with more than 64 removals some of those are numbered 64 and above.  d = 128, 129 (three
  words), 144, and `half_opened`: seven units that are only opened (removals 0-62), then four that slip - most conflict masks are 0
  in word 0.  Widths 4-8: the mirrors over whole-structure energies take seconds beyond.
* `dedup_cases()` (c): six hairpins of 11 pairs (d 66) at width 100 on which a duplicate test that looks at the ranks below 64 only
  returns ANOTHER PATH, and five of 13 pairs (d 65) at width 160 on which one that looks at the ranks below 128 does;
  `find_dedup_seed` is the search that found DEDUP_SEEDS, and what it did not find is said there.
* `full_beam_cases()` (d): d = 12 at width 1024 - three hairpins of 4 pairs opened and folded (all C(12,6) = 924 states of level 6
  are live), two problems with a conflict that keep 672 - where the beam drops nothing and the result is the exact saddle.  (No
  test sees the beam's tail past rank 512: on such problems cutting the sorted keys at 512 changes no returned path.)
* `mixed_chunk()` (e): a 40-nt d = 12, a d = 144, a d = 65 problem and `half_opened` (the longest) next to each other: the expand
  kernel's LDS is laid out for the chunk's longest L and largest d, while each problem uses its own number of words.
* one cache per process: `mirror` (the definition, FP.search) and `marked` (the kernels' scheme, with its counts) compute a
  (tables, problem, width[, defect]) once, whichever file asks first, over one store of whole-structure energies per (tables,
  problem).  Both leave the oracle with the tables they were asked for; the callers' fixtures put the built-in ones back.
"""
import time

import numpy as np

import oracle
import _findpath_np as FP
import _lane_rounds as LR
import _loops as LP
import _par_reader as PR

SEED = 131
DEDUP_SEEDS = (2, 1)            # found by find_dedup_seed, see there
SMALL_WIDTHS = (1, 2, 7)
COMPLEMENT = {"G": "C", "C": "G", "A": "U", "U": "A"}
TIMES = {}                      # (kind, tables, name of the problem, width, defect) -> seconds of the mirror


def _install(which):
    """the oracle's tables: "builtin", or "index" - the index-sensitive set tests/test_gpu_findpath.py loads into the library.
    (The first use of "index" in a process reads the built-in set through _loops.builtin_par, which resets the LIBRARY's parameters:
    a GPU test asks for its "index" mirrors before it loads parameters into the library.)"""
    if which == "builtin":
        oracle.reset_tables()
    else:
        assert which == "index"
        oracle.set_tables(LR._once(("findpath tables", which), lambda: PR.tables_at(LP.index_sensitive_par(LP.builtin_par()), 37.0)))


def _energy(which, prob):
    """oracle.eval_structure with the store of mask -> energy of (tables, problem) that FP._energy_of shares among its searches"""
    def energy(seq, row):
        return oracle.eval_structure(seq, row)
    energy.masks = LR._once(("findpath energies", which, prob), dict)
    return energy


def _timed(key, make):
    def run():
        t0 = time.perf_counter()
        out = make()
        TIMES[key] = time.perf_counter() - t0
        return out
    return LR._once(key, run)


def mirror(which, prob, width):
    """FP.search(*prob, width) under the tables `which`"""
    def make():
        _install(which)
        return FP.search(*prob, width, energy=_energy(which, prob))
    return _timed(("findpath search", which, prob, width), make)


def marked(which, prob, width, defect=None):
    """(FP.search_marked(*prob, width, defect=defect), its stats) under the tables `which`"""
    def make():
        _install(which)
        stats = {}
        return FP.search_marked(*prob, width, energy=_energy(which, prob), defect=defect, stats=stats), stats
    return _timed(("findpath marked", which, prob, width, defect), make)


def mask_words(d):
    return max(1, (d + 63) // 64)


def dist(prob):
    """(d, n_rem)"""
    mv, n_rem = FP.move_list(prob[1], prob[2])
    return len(mv), n_rem


# ---- builders

def hairpins(rng, n, k, letters="GCGCAU", loop="GAAA", gap="A", flank=""):
    """(seq, folded, open): n hairpins of k pairs, the 5' side of each stem drawn from `letters`"""
    seq, row = [], []
    for _ in range(n):
        five = "".join(rng.choice(list(letters), k))
        seq.append(five + loop + "".join(COMPLEMENT[c] for c in reversed(five)))
        row.append("(" * k + "." * len(loop) + ")" * k)
    seq, row = flank + gap.join(seq) + flank, "." * len(flank) + ("." * len(gap)).join(row) + "." * len(flank)
    return seq, row, "." * len(seq)


def slipped(rng, units):
    """(seq, a, b): per (ka, kb) of `units` one unit G^10 AAAA Y^10 of 24 nt; A holds its pairs (i, 23 - i), i < ka, B the pairs
    (i + 1, 23 - i), i < kb: B's pair i shares a base with A's pairs i and i + 1"""
    seq, a, b = [], [], []
    for ka, kb in units:
        assert 0 <= kb <= ka <= 9
        seq.append("G" * 10 + "AAAA" + "".join(rng.choice(list("CCU"), 10)))
        ra, rb = ["."] * 24, ["."] * 24
        for i in range(ka):
            ra[i], ra[23 - i] = "(", ")"
        for i in range(kb):
            rb[i + 1], rb[23 - i] = "(", ")"
        a.append("".join(ra))
        b.append("".join(rb))
    return "A".join(seq), ".".join(a), ".".join(b)


# ---- (a) removals across the word edge

def removal_cases():
    """[(name, (seq, a, b), width)]"""
    def make():
        rng = np.random.default_rng(SEED)
        out = []
        for n, k, width in ((8, 8, 64), (5, 13, 65), (6, 11, 66), (7, 10, 80)):
            seq, folded, chain = hairpins(rng, n, k)
            out.append(("open%d" % (n * k), (seq, folded, chain), width))
        return out
    return LR._once(("findpath cases", "a"), make)


# ---- (b) additions across the word edge

def addition_cases():
    """[(name, (seq, a, b), width)]"""
    def make():
        rng = np.random.default_rng(SEED + 1)
        return [("slip128", slipped(rng, [(9, 8)] * 7 + [(5, 4)]), 8),
                ("slip129", slipped(rng, [(9, 8)] * 7 + [(5, 5)]), 8),
                ("slip144", slipped(rng, [(9, 9)] * 8), 4),
                ("half_opened", slipped(rng, [(9, 0)] * 7 + [(9, 9)] * 4), 4)]
    return LR._once(("findpath cases", "b"), make)


# ---- (c) duplicates that only a rank of the second, or third, round forms, and that matter

def dedup_cases():
    """[(name, (seq, a, b), width, defect)]: hairpins opened on which a duplicate test that stops after one round of 64 ranks, or
    after two, returns another path than the definition"""
    def make():
        return [("dedup66", hairpins(np.random.default_rng(DEDUP_SEEDS[0]), 6, 11), 100, "dedup_rounds:1"),
                ("dedup65", hairpins(np.random.default_rng(DEDUP_SEEDS[1]), 5, 13), 160, "dedup_rounds:2")]
    return LR._once(("findpath cases", "c"), make)


def find_dedup_seed(seeds, width, rounds, n=6, k=11, budget=400.0):
    """the seeds whose problem (n hairpins of k pairs, opened) returns another path at `width` when only the ranks below 64 `rounds`
    are examined for duplicates - survivor 0's moves or energies, not merely a narrower beam.  A search of its own, run by no test:
      find_dedup_seed(range(6), 100, 1)                 -> [2, 4]       (DEDUP_SEEDS[0])
      find_dedup_seed(range(10), 160, 2, n=5, k=13)     -> [1]          (DEDUP_SEEDS[1])
      find_dedup_seed(range(10), 200, 2)                -> [3, 4]
      find_dedup_seed(range(10), 130, 2, n=7, k=10)     -> []           (two ranks of a third round: none of ten seeds)"""
    hits, t0 = [], time.perf_counter()
    for seed in seeds:
        if time.perf_counter() - t0 > budget:
            break
        seq, folded, chain = hairpins(np.random.default_rng(seed), n, k)
        energy, stats = _energy("builtin", (seq, folded, chain)), {}
        right = FP.search_marked(seq, folded, chain, width, energy=energy, stats=stats)
        wrong = FP.search_marked(seq, folded, chain, width, energy=energy, defect="dedup_rounds:%d" % rounds)
        if wrong != right:
            hits.append(seed)
        print(seed, wrong != right, stats, "%.0f s" % (time.perf_counter() - t0), flush=True)
    return hits


# ---- (d) full beams at the largest width

FULL_WIDTH = 1024


def full_beam_cases():
    """[(name, (seq, a, b), live states at level 6)]: every problem has d = 12 and runs at FULL_WIDTH"""
    def make():
        seq, folded, chain = hairpins(np.random.default_rng(SEED + 2), 3, 4, flank="A")
        assert len(seq) == 40
        # ten free moves and an addition (3,9) of the last unit that waits for the removal (2,9): C(10,6) + C(10,5) + C(10,4) states
        two, f2, _ = hairpins(np.random.default_rng(SEED + 3), 2, 4)
        unit = "GCGGAAAAACGC"
        slip = (two + "A" + unit, f2 + "." + "(((......)))", "." * len(two) + "." + "...(.....)..")
        h4, f4, _ = hairpins(np.random.default_rng(SEED + 4), 1, 4)
        h5, f5, _ = hairpins(np.random.default_rng(SEED + 5), 1, 5)
        both = (h4 + "A" + unit + "A" + h5, f4 + "." + ".((......))." + "." + "." * len(h5), "." * len(h4) + "." + "...(.....).." + "." + f5)
        return [("open12", (seq, folded, chain), 924), ("fold12", (seq, chain, folded), 924), ("slip12", slip, 672), ("both12", both, 672)]
    return LR._once(("findpath cases", "d"), make)


# ---- (e) one chunk of problems with different L, d and mask words

def mixed_chunk():
    """[((seq, a, b), width)]: 40 nt with d = 12 (one word), d = 144 (three words, the chunk's largest d), d = 65 (two words), and
    `half_opened` (274 nt, the chunk's longest; d = 135)"""
    a, b = removal_cases(), addition_cases()
    return [(full_beam_cases()[0][1], FULL_WIDTH), b[2][1:], a[1][1:], b[3][1:]]
