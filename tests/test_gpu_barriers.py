"""rafft_barriers_batch on a real MI355X (`-m gpu`): on the full enumerations of tests/_descend_np.py, on bands of 40-80-nt
sequences, on deduplicated samples (incomplete landscapes) and on tie-heavy bands in both orders of their plateaus, minima, fathers,
saddles, basins and edges are those of the tests' mirror - the sequential flooding of `barriers`, where the library runs Kruskal
over a graph of minima; on bands of 10^4 rows and more at 100-200 nt the invariants of the definition, with neighbours generated a
third way, against descend_batch and against findpath; the edges of the shapes up to 4096 nt; same input - same bits across batch
position, order, duplicates, chunking and strides; statuses that stay with their sequence; Python and the command line.  Integers:
no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import rafft_amd
from rafft_amd import _native as N, barriers as BR, descend as DSm, findpath as FPm, mccaskill, params, rafft_kin, wuchty, zuker
from conftest import ROOT
import _barriers_np as BM
import _descend_np as DS
from _descend_np import all_neighbours, move_row
import _loops as LP
import _par_reader as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    out = dict(builtin=builtin, index=LP.index_sensitive_par(builtin), synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name in ("index", "synthetic"):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=name)
    return out


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()
    oracle.reset_tables()


def rand(rng, n, letters="ACGU"):
    return "".join(rng.choice(list(letters), n))


def texts(rows, L):
    """the rows of an (n, stride) uint8 array as strings"""
    return [r[:L].tobytes().decode("ascii") for r in rows]


def bands(seqs, deltas, max_structs=100000):
    """[(rows as strings, dcal as list)] per sequence: one subopt call per distinct delta (dcal)"""
    out = [None] * len(seqs)
    for delta in sorted(set(deltas)):
        idx = [k for k in range(len(seqs)) if deltas[k] == delta]
        recs, rows, dcal = wuchty.subopt_batch_raw([seqs[k] for k in idx], delta, max_structs)
        for k, r, a, d in zip(idx, recs, rows, dcal):
            assert r["status"] == 0, (seqs[k], delta, r)
            out[k] = (texts(a, len(seqs[k])), d.tolist())
    return out


def check_against_mirror(seqs, lands, what, **kw):
    """one call over all landscapes [(rows, dcal)]; every record equals the mirror's"""
    got = BR.barriers_batch_raw(list(seqs), [r for r, _ in lands], [d for _, d in lands], **kw)
    for k, (g, (rows, dcal)) in enumerate(zip(got, lands)):
        assert g["status"] == 0 and g["n_rows"] == len(rows), (what, k, g["status"], N.lib().rafft_last_error())
        want = BM.flood(rows, dcal)
        assert BM.matches(g, want) is None, (what, k, seqs[k], BM.matches(g, want))
    return got


# ---- equality with the mirror

@pytest.mark.parametrize("which", ["builtin", "index"])
def test_equals_the_mirror_on_every_enumeration(sets, which):
    if which == "index":
        oracle.set_tables(PR.tables_at(sets["index"], 37.0))
    groups = DS.start_sequences()
    lands = []
    for seq, rows in groups:
        en = [oracle.eval_structure(seq, r) for r in rows]
        order = sorted(range(len(rows)), key=lambda k: (en[k], k))
        lands.append(([rows[k] for k in order], [en[k] for k in order]))
    got = check_against_mirror([s for s, _ in groups], lands, which)
    assert all((g["father"] == -1).sum() == 1 for g in got)                # a full enumeration hangs together
    c = BR.barriers_counters()
    assert c["chunks"] == 1 and c["launches"] == 5 and c["rows"] == sum(len(r) for r, _ in lands)
    assert c["minima"] == sum(len(g["rank"]) for g in got) and c["edges"] == sum(len(g["edges"]) for g in got)
    # every neighbour relation is met from both sides in the pass that finds down
    assert c["hits"] == sum(len(nb) for rows, _ in lands for nb in BM.neighbour_ranks(rows))
    print(f"\n{which}: {c}")


# (sequence, delta in dcal): the bands have 200 to 5000 rows; the mirror takes well under a second on each
LONGER = [("GCCGUUUCUUUCAAGUCUGAGUGCCUUUUGAUAUACCAGU", 400), ("UACUCUACGUCUGCCUAAAACGGCGAUACAUUUCUAUAAAGAGACAUUUA", 500),
          ("GAGGUGAGCCCGGAACGGUAACUCCCUAUACGUUUUAUUAAACAUCGGGUCUUGCUGACC", 400),
          ("ACGAAUGUUUCGCCGCGUACUCAUGUACCACUCGUCUCAUCAUCUCGUAUUGCUCGAAGACUGGAUCUGC", 200),
          ("ACCCCGCCUAGCUACAGUAUUACUUUACAGUACACUUGCGACCUCCGGCGCAGGUAUAUCCCUUCAACUAUCUAGGGACC", 400)]


def test_equals_the_mirror_on_bands_of_longer_sequences():
    seqs, deltas = [s for s, _ in LONGER], [d for _, d in LONGER]
    lands = bands(seqs, deltas)
    assert all(200 <= len(r) <= 5000 for r, _ in lands), [len(r) for r, _ in lands]
    got = check_against_mirror(seqs, lands, "longer")
    print("\nrows", [len(r) for r, _ in lands], "minima", [len(g["rank"]) for g in got], "edges", [len(g["edges"]) for g in got])
    assert sum(len(g["edges"]) for g in got) >= 50 and any((g["father"] >= 0).sum() >= 10 for g in got)


def test_equals_the_mirror_on_incomplete_landscapes():
    rng = np.random.default_rng(20261025)
    seqs = [rand(rng, 60), rand(rng, 120)]
    _, rows, dcal = mccaskill.sample_batch_raw(seqs, 500, seeds=11)
    lands = []
    for s, a, d in zip(seqs, rows, dcal):
        uniq = sorted({(int(e), r) for r, e in zip(texts(a, len(s)), d.tolist())})
        lands.append(([r for _, r in uniq], [e for e, _ in uniq]))
    assert all(100 <= len(r) <= 500 for r, _ in lands), [len(r) for r, _ in lands]
    got = check_against_mirror(seqs, lands, "sampled")
    # most probes miss here: far fewer neighbours are in the list than a structure has
    hits = BR.barriers_counters()["hits"]
    probes = sum(len(all_neighbours(s, r)) for s, (rows_s, _) in zip(seqs, lands) for r in rows_s)
    print(f"\nrows {[len(r) for r, _ in lands]} minima {[len(g['rank']) for g in got]}: {hits} of {probes} probes hit")
    assert 0 < hits < probes // 4


# (sequence, delta in dcal): low-complexity sequences whose bands are plateaus - nearly every row has its energy in common with
# the row before or after it (0.98 and more of the rows on the CPU mirror), and reversing the plateaus changes the trees
TIES = [("GGGAAACCC" * 4, 1100), ("GC" * 12, 1600), ("GU" * 14, 1000), ("GGGUUUGGGUUUCCC" * 2, 800)]


def test_ties_and_plateaus_follow_the_order_of_the_list():
    seqs, deltas = [s for s, _ in TIES], [d for _, d in TIES]
    lands = bands(seqs, deltas)
    for rows, dcal in lands:
        n = len(dcal)
        shared = sum((x > 0 and dcal[x - 1] == dcal[x]) or (x + 1 < n and dcal[x + 1] == dcal[x]) for x in range(n))
        assert 3 * shared >= n and n >= 400, (n, shared)
    got = check_against_mirror(seqs, lands, "ties")
    # ... some of them between rows that are one move apart, where the order alone decides which is the minimum
    assert sum(BM.tie_share(BM.neighbour_ranks(r), d) > 0 for r, d in lands) >= 3
    turned = [BM.reverse_equal_runs(r, d) for r, d in lands]
    assert all(d == d2 and r != r2 for (r, d), (r2, d2) in zip(lands, turned))
    got2 = check_against_mirror(seqs, turned, "ties, plateaus reversed")
    assert any(len(a["rank"]) != len(b["rank"]) or a["basin_size"].tolist() != b["basin_size"].tolist() for a, b in zip(got, got2))


# ---- neighbours, stated a third way (_descend_np.all_neighbours: from the loops' members)

class Lookup:
    """the ranks of a row's neighbours in a band: neighbours from the loops' members, found through a sum of random 64-bit numbers
    per pair (drawn here; a row's number is checked to be its own)"""

    def __init__(self, seq, rows, seed=1):
        self.seq, self.rows, L = seq, rows, len(seq)
        self.h = np.random.default_rng(seed).integers(1, 1 << 62, size=(L, L)).tolist()
        self.key = [sum(self.h[i][j] for i, j in DS.pairs_of(r)) for r in rows]
        self.rank = {k: x for x, k in enumerate(self.key)}
        assert len(self.rank) == len(rows)

    def neighbours(self, x):
        k, out = self.key[x], []
        for i, j, rem in all_neighbours(self.seq, self.rows[x]):
            r = self.rank.get(k - self.h[i][j] if rem else k + self.h[i][j])
            if r is not None:
                out.append(r)
        return out


# (sequence, delta in dcal): bands of 10^4 rows and more at 100 and 150 nt
LARGE = [("UUACGCAGGGGAAUACGCUCUUACUAUCAGGGUUUGAGACCUGAUGAUGUUGACAUUGUUGUGAUCCAUUCCAGCGGGAGCGGACCGUCCAGAUUGAAUU", 550),
         ("CCUAGUCCAUUUGUCUCUUCCCACCUAGAUAAGAGUGAAGGGAUCUUCCCUACUGAACUCGAUCCCUAAAUACCUACAAUCACUUACUUGGGGUAAGAAGAAUAUGUGGAGGUAAUCCUAAACGCCGAACUGGACCUCGCACACGUAUUU", 500)]
_LARGE = {}


def large():
    """the large bands, their trees and their look-ups, computed once"""
    if not _LARGE:
        seqs, deltas = [s for s, _ in LARGE], [d for _, d in LARGE]
        lands = bands(seqs, deltas)
        got = BR.barriers_batch_raw(seqs, [r for r, _ in lands], [d for _, d in lands])
        _LARGE.update(seqs=seqs, deltas=deltas, lands=lands, got=got, look=[Lookup(s, r) for s, (r, _) in zip(seqs, lands)], counters=BR.barriers_counters())
    return _LARGE


def components_below(n, edges, limit):
    """union-find over the edges (a, b, t) with t <= limit: the root (lowest index) of every minimum"""
    up = np.arange(n)

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    for a, b, t in edges:
        if t <= limit:
            ra, rb = find(a), find(b)
            if ra != rb:
                up[max(ra, rb)] = min(ra, rb)
    return [find(x) for x in range(n)]


def test_invariants_on_large_bands():
    big = large()
    for seq, (rows, dcal), g, look in zip(big["seqs"], big["lands"], big["got"], big["look"]):
        n, nm = len(rows), len(g["rank"])
        assert g["status"] == 0 and 10000 <= n <= 100000, (n, g["status"])
        basin, rank, father, saddle = g["basin"].tolist(), g["rank"].tolist(), g["father"].tolist(), g["saddle_rank"].tolist()
        is_min = set(rank)
        assert rank == sorted(is_min) and rank[0] == 0 and g["dcal"].tolist() == [dcal[x] for x in rank]
        assert g["basin_size"].tolist() == np.bincount(g["basin"], minlength=nm).tolist() and int(g["basin_size"].sum()) == n
        direct = {}
        for x in range(n):
            nb = look.neighbours(x)
            low = min(nb) if nb else x
            if x in is_min:
                assert low >= x, (x, low)                                                     # no lower-ranked neighbour
                continue
            assert low < x and basin[x] == basin[low], (x, low)                               # its basin is its down neighbour's
            for r in nb:
                if r < x and basin[r] != basin[x]:
                    key = (min(basin[r], basin[x]), max(basin[r], basin[x]))
                    direct[key] = min(direct.get(key, x), x)
        assert all(basin[x] == m for m, x in enumerate(rank))
        edges = [(int(a), int(b), int(t)) for a, b, t in g["edges"]]
        assert sorted((t, a, b) for (a, b), t in direct.items()) == [(t, a, b) for a, b, t in edges]
        assert edges == sorted(edges, key=lambda e: (e[2], e[0], e[1])) and all(a < b and t >= max(rank[a], rank[b]) for a, b, t in edges)
        # the tree: father < index, the saddle at least both ranks, and the link is connected below saddle_rank but not one below
        for m in range(nm):
            assert (father[m] < 0) == (saddle[m] < 0) and father[m] < m
            if father[m] >= 0:
                assert saddle[m] >= rank[m] > rank[father[m]] and g["saddle_dcal"][m] == dcal[saddle[m]]
            else:
                assert g["saddle_dcal"][m] == 0
        for t in sorted({s for s in saddle if s >= 0}):
            at, before = components_below(nm, edges, t), components_below(nm, edges, t - 1)
            for m in range(nm):
                if saddle[m] == t:
                    assert at[m] == at[father[m]] == father[m] and before[m] == m, (m, t)
        last = components_below(nm, edges, n)
        assert all(last[m] == m for m in range(nm) if father[m] < 0)
        print(f"\n{len(seq)} nt: {n} rows, {nm} minima, {len(edges)} edges, {father.count(-1)} roots")
    assert big["counters"]["rows"] == sum(len(r) for r, _ in big["lands"])


def test_basins_are_the_ends_of_descend_batch_where_no_energies_tie(sets):
    """basin[x] follows the lowest-RANKED neighbour, descend_batch the lowest (dE, i, j): the two agree where energies decide alone.
    Under the built-in tables a row of these bands has two neighbours of one energy somewhere on its way more often than not (335
    and 292 of 400 sampled rows on the CPU mirror), so the bands are taken under the index-sensitive tables, whose loop terms differ
    by position: 44 and 43 of 400 there."""
    params.load_params(sets["paths"]["index"])
    seqs = [s for s, _ in LARGE]
    lands = bands(seqs, [1702, 1702])
    got = BR.barriers_batch_raw(seqs, [r for r, _ in lands], [d for _, d in lands])
    rng = np.random.default_rng(3)
    for seq, (rows, dcal), g in zip(seqs, lands, got):
        n = len(rows)
        assert g["status"] == 0 and 10000 <= n <= 100000, (n, g["status"])
        look = Lookup(seq, rows)
        pick = sorted(rng.choice(n, 400, replace=False).tolist())
        rec, row_rec, ends, moves = DSm.descend_batch_raw([seq], [[rows[x] for x in pick]])
        index = {r: x for x, r in enumerate(rows)}
        rank = g["rank"].tolist()
        used = left_out = 0
        for k, x in enumerate(pick):
            path = FPm.path_rows(rows[x], moves[0][k].reshape(-1, 2))
            on_way = [index.get(r) for r in path]
            # the walk stays inside the band's ensemble, and no two neighbours of any row on the way share an energy
            clean = all(y is not None for y in on_way)
            for y in on_way if clean else []:
                en = [dcal[r] for r in look.neighbours(y)]
                clean = clean and len(set(en)) == len(en)
            if not clean:
                left_out += 1
                continue
            used += 1
            assert rank[g["basin"][x]] == on_way[-1], (x, on_way)
        print(f"\n{len(seq)} nt: {used} rows compared, {left_out} left out")
        assert left_out <= 0.2 * len(pick)          # the cap: at most 20 % of the rows may be left out by the condition


def longest_interior(row):
    """the largest number of unpaired positions of any interior loop of the row"""
    pairs = dict(DS.pairs_of(row))
    worst = 0
    for i, j in pairs.items():
        p = i + 1
        while p < j and row[p] == ".":
            p += 1
        if p < j and row[p] == "(" and all(c == "." for c in row[pairs[p] + 1:j]):
            worst = max(worst, (p - i - 1) + (j - pairs[p] - 1))
    return worst


def test_findpath_saddles_are_never_below_the_trees():
    big = large()
    for seq, delta, (rows, dcal), g in zip(big["seqs"], big["deltas"], big["lands"], big["got"]):
        links = [(m, int(f)) for m, f in enumerate(g["father"].tolist()) if f >= 0][:400]
        a = [rows[g["rank"][m]] for m, _ in links]
        b = [rows[g["rank"][f]] for _, f in links]
        recs, paths, _ = FPm.findpath_batch([seq] * len(links), a, b, width=16, both=True)
        checked = equal = 0
        for (m, f), r, moves, start in zip(links, recs, paths, a):
            assert r["status"] == 0
            exact = int(g["saddle_dcal"][m])
            if r["saddle_dcal"] > dcal[0] + delta:
                continue
            if any(longest_interior(w) > 30 for w in FPm.path_rows(start, moves)):
                continue
            checked += 1
            assert r["saddle_dcal"] >= exact, (m, f, r["saddle_dcal"], exact)
            equal += r["saddle_dcal"] == exact
        print(f"\n{len(seq)} nt: findpath (width 16, both) reaches the exact saddle on {equal} of {checked} links ({len(links)} asked)")
        assert checked >= len(links) // 2


# ---- the edges of the shapes

def one(seq, rows, dcal, **kw):
    return BR.barriers_batch_raw([seq], [rows], [dcal], **kw)[0]


def test_edges_of_the_shapes():
    # lengths 1-4 and poly-A: one open row, one minimum, no edges
    for seq in ("A", "GC", "GCG", "GAAC", "A" * 30):
        g = one(seq, ["." * len(seq)], [0])
        assert g["status"] == 0 and g["rank"].tolist() == [0] and g["father"].tolist() == [-1] and g["saddle_rank"].tolist() == [-1]
        assert g["basin"].tolist() == [0] and g["basin_size"].tolist() == [1] and len(g["edges"]) == 0 and g["saddle_dcal"].tolist() == [0]
    # n_rows = 1 with pairs; two rows that are no neighbours: two roots
    g = one("GGGAAAACCC", ["(((....)))"], [-120])
    assert g["rank"].tolist() == [0] and g["dcal"].tolist() == [-120]
    g = one("GGGAAAACCC", ["(((....)))", ".........."], [-120, 0])
    assert g["rank"].tolist() == [0, 1] and g["father"].tolist() == [-1, -1] and g["basin"].tolist() == [0, 1] and len(g["edges"]) == 0
    # ... with the rows between them: one tree, and the second minimum hangs under the first at the highest row of the way
    way = ["(((....)))", "..........", "(.(....).)", "(........)", ".((....))."]
    g = one("GGGAAAACCC", way, [-120, 0, 10, 20, 30])
    assert BM.matches(g, BM.flood(way, [-120, 0, 10, 20, 30])) is None and g["father"].tolist() == [-1, 0] and g["saddle_rank"].tolist() == [-1, 3]
    # N pairs with nothing: the rows of a sequence with N that the band of its neighbours never holds
    seq = "GGGNAAAANCCC"
    rows = ["((........))", "(..........)", ".(........).", "............", "(((......)))"]
    g = one(seq, rows, [-50, -10, 0, 0, 5])
    assert g["status"] == 0 and BM.matches(g, BM.flood(rows, [-50, -10, 0, 0, 5])) is None
    assert one(seq, ["((((....))))"], [0])["status"] == N.ERR_STRUCT


@pytest.mark.parametrize("L", [63, 64, 65, 129])
def test_lengths_where_the_lanes_stride(L):
    rng = np.random.default_rng(L)
    seq = rand(rng, L)
    _, rows, dcal = mccaskill.sample_batch_raw([seq], 300, seeds=L)
    row0 = texts(rows[0], L)[0]
    # a sample and, so that the list hangs together, every row one removal away from its first row
    extra = {move_row(row0, i, j, True) for i, j in DS.pairs_of(row0)}
    en = dict(zip(texts(rows[0], L), dcal[0].tolist()))
    more = sorted(extra - set(en))
    if more:
        e2, st = rafft_amd.rafft.eval_structures([seq] * len(more), more)
        en.update(zip(more, [int(e) for e in e2]))
    uniq = sorted((e, r) for r, e in en.items())
    land = ([r for _, r in uniq], [e for e, _ in uniq])
    got = check_against_mirror([seq], [land], f"L = {L}")[0]
    assert len(got["edges"]) >= 1 or (got["father"] >= 0).any() or len(got["rank"]) < len(land[0])


def test_a_sequence_of_4096_nt():
    rng = np.random.default_rng(4096)
    seq = rand(rng, N.BARRIERS_MAX_LEN)
    mfe_row = zuker.mfe_batch_raw([seq])[0][0]
    pairs = DS.pairs_of(mfe_row)
    assert len(pairs) >= 20
    rows = [mfe_row] + [move_row(mfe_row, i, j, True) for i, j in pairs[::max(1, len(pairs) // 20)][:20]]
    g = one(seq, rows, list(range(len(rows))))            # (made-up energies in list order: the MFE row first)
    assert g["status"] == 0 and g["rank"].tolist() == [0] and g["basin"].tolist() == [0] * len(rows) and g["basin_size"].tolist() == [len(rows)]
    # the MFE row last: every other row is a minimum of its own and the MFE row, one move from each, joins them all under the first
    g = one(seq, rows[1:] + rows[:1], list(range(len(rows))))
    k = len(rows) - 1
    assert g["rank"].tolist() == list(range(k)) and g["father"].tolist() == [-1] + [0] * (k - 1) and g["saddle_rank"].tolist() == [-1] + [k] * (k - 1)
    assert g["basin"].tolist() == list(range(k)) + [0] and [tuple(e) for e in g["edges"].tolist()] == [(0, b, k) for b in range(1, k)]


def star(n):
    """n rows over a sequence of hairpins: the open chain first, then single pairs - every row after the first is one move from it"""
    unit = "GAAAC"
    seq = unit * 40
    rows = ["." * len(seq)]
    for a in range(40):
        for b in range(a, 40):
            if len(rows) < n:
                rows.append(move_row(rows[0], 5 * a, 5 * b + 4, False))
    assert len(rows) == n
    return seq, rows


def test_a_table_exactly_on_a_power_of_two_and_one_row_more():
    for n in (512, 513):
        seq, rows = star(n)
        g = one(seq, rows, [0] + [100] * (n - 1))
        assert g["status"] == 0 and g["rank"].tolist() == [0] and g["basin_size"].tolist() == [n]
        assert BR.barriers_counters()["hits"] == 2 * (n - 1)
        g = one(seq, rows[1:] + rows[:1], [0] * n)          # the hub last: n - 1 minima, all joined by it
        assert len(g["rank"]) == n - 1 and g["father"].tolist() == [-1] + [0] * (n - 2) and len(g["edges"]) == n - 2


def test_max_edges_is_exact():
    # 1200 single-pair rows, then the open chain: 1199 distinct edges, above the floor of 1024
    unit = "GAAAC"
    seq = unit * 50
    open_row = "." * len(seq)
    rows = []
    for a in range(50):
        for b in range(a, 50):
            if len(rows) < 1200:
                rows.append(move_row(open_row, 5 * a, 5 * b + 4, False))
    rows.append(open_row)
    dcal = [0] * len(rows)
    g = one(seq, rows, dcal)
    assert g["status"] == 0 and len(g["edges"]) == 1199 and len(g["rank"]) == 1200
    exact = one(seq, rows, dcal, max_edges=1199)
    assert exact["status"] == 0 and BM.matches(exact, {k: (g[k].tolist() if k != "edges" else [(t, a, b) for a, b, t in g[k].tolist()]) for k in
                                                    ("rank", "father", "saddle_rank", "saddle_dcal", "dcal", "basin_size", "basin", "edges")}) is None
    short = one(seq, rows, dcal, max_edges=1198)
    assert short["status"] == N.ERR_CAPACITY and len(short["rank"]) == 0
    assert "raise max_edges" in N.lib().rafft_last_error().decode()
    # below the floor the floor holds
    assert one(seq, rows[-300:], dcal[-300:], max_edges=1)["status"] == 0


# ---- same input, same bits

def same(a, b):
    return a["status"] == b["status"] and all(np.array_equal(a[k], b[k]) for k in ("rank", "father", "saddle_rank", "dcal", "saddle_dcal", "basin_size", "basin", "edges"))


def test_same_input_same_bits():
    seqs, deltas = [s for s, _ in LONGER[:3]], [d for _, d in LONGER[:3]]
    lands = bands(seqs, deltas)
    R, D = [r for r, _ in lands], [d for _, d in lands]
    base = BR.barriers_batch_raw(seqs, R, D)
    assert all(g["status"] == 0 and len(g["edges"]) for g in base)
    again = BR.barriers_batch_raw(seqs, R, D)
    assert all(same(a, b) for a, b in zip(base, again))
    for k in range(3):
        assert same(base[k], BR.barriers_batch_raw([seqs[k]], [R[k]], [D[k]])[0])
    rev = BR.barriers_batch_raw(seqs[::-1], R[::-1], D[::-1])
    assert all(same(a, b) for a, b in zip(base, rev[::-1]))
    dup = BR.barriers_batch_raw([seqs[0], seqs[1], seqs[0]], [R[0], R[1], R[0]], [D[0], D[1], D[0]])
    assert same(dup[0], base[0]) and same(dup[1], base[1]) and same(dup[2], base[0])
    # one sequence per chunk: a workspace that holds the largest work area and no two
    L = [len(s) for s in seqs]
    area = [len(R[k]) * (((2 * L[k] + 15) & ~15) + 24) + 8 * (1 << (2 * len(R[k]) - 1).bit_length()) + 12 * (1 << (2 * max(4 * len(R[k]), 1024) - 1).bit_length()) for k in range(3)]
    chunked = BR.barriers_batch_raw(seqs, R, D, workspace_bytes=max(area))
    assert BR.barriers_counters()["chunks"] == 3 and BR.barriers_counters()["launches"] == 15
    assert all(same(a, b) for a, b in zip(base, chunked))
    # strides L + 1 (the arrays of subopt_batch_raw) and L (strings)
    arrays = [np.frombuffer(b"".join(r.encode() + b"\0" for r in R[k]), dtype=np.uint8).reshape(len(R[k]), L[k] + 1) for k in range(3)]
    assert all(same(a, b) for a, b in zip(base, BR.barriers_batch_raw(seqs, arrays, D)))
    # a larger edge table
    assert all(same(a, b) for a, b in zip(base, BR.barriers_batch_raw(seqs, R, D, max_edges=50000)))


# ---- statuses beside untouched neighbours

def test_statuses_stay_with_their_sequence():
    good_seq, good_delta = LONGER[0]
    (rows, dcal), = bands([good_seq], [good_delta])
    alone = BR.barriers_batch_raw([good_seq], [rows], [dcal])[0]
    cases = [("", [""], [0], N.ERR_EMPTY, "empty"),
             ("GGGTAAAACCC", ["..........."], [0], N.ERR_BAD_CHAR, "character"),
             ("A" * 4097, ["." * 4097], [0], N.ERR_TOO_LONG, "longer"),
             ("GGGAAAACCC", [], [], N.ERR_EMPTY, "no rows"),
             ("GGGAAAACCC", ["(((....)))", "((.....).)"[:9]], [-120, 0], N.ERR_STRUCT, "row 1: malformed"),
             ("GGGAAAACCA", ["..........", "(........)"], [0, 10], N.ERR_STRUCT, "row 1: malformed"),
             ("GGGAAAACCC", ["(((....)))", ".........."], [0, -1], N.ERR_STRUCT, "row 1: its dcal"),
             ("GGGAAAACCC", ["(((....)))", "..........", "((......))", ".........."], [-120, 0, 0, 0], N.ERR_STRUCT, "rows 1 and 3 are the same structure")]
    for seq, r, d, status, text in cases:
        got = BR.barriers_batch_raw([good_seq, seq, good_seq], [rows, r, rows], [dcal, d, dcal])
        assert got[1]["status"] == status and len(got[1]["rank"]) == 0, (seq, r, got[1]["status"])
        assert N.lib().rafft_last_error().decode().startswith("sequence 1: ") and text in N.lib().rafft_last_error().decode(), N.lib().rafft_last_error()
        assert same(got[0], alone) and same(got[2], alone)
    # a work area above the workspace: the small neighbours run, the large one is refused with its bytes
    small = ("GGGAAAACCC", ["(((....)))", "((......))"], [-120, -50])
    got = BR.barriers_batch_raw([small[0], good_seq, small[0]], [small[1], rows, small[1]], [small[2], dcal, small[2]], workspace_bytes=30000)
    assert [g["status"] for g in got] == [0, N.ERR_CAPACITY, 0] and "its work area needs" in N.lib().rafft_last_error().decode()
    assert same(got[0], got[2]) and got[0]["rank"].tolist() == [0] and got[0]["basin"].tolist() == [0, 0]


def test_another_temperature_enters_through_subopt_only(sets):
    params.load_params(sets["paths"]["synthetic"])
    seq = LONGER[0][0]
    t25 = BR.barrier_tree(seq, delta=3.0, temp=25.0)
    recs, rows, dcal = wuchty.subopt_batch_raw([seq], 300, temp=25.0)
    want = BM.flood(texts(rows[0], len(seq)), dcal[0].tolist())
    assert [m.str_struct for m in t25.minima] == [texts(rows[0], len(seq))[x] for x in want["rank"]]
    assert t25.father.tolist() == want["father"] and t25.saddle_dcal.tolist() == want["saddle_dcal"] and t25.basin_of.tolist() == want["basin"]
    t37 = BR.barrier_tree(seq, delta=3.0)
    assert [m.dcal for m in t37.minima] != [m.dcal for m in t25.minima]


# ---- Python and the command line

def test_barrier_tree_prune_and_kinetics():
    seq, delta = LONGER[1]
    tree = BR.barrier_tree(seq, delta=delta / 100.0)
    (rows, dcal), = bands([seq], [delta])
    want = BM.flood(rows, dcal)
    assert [m.str_struct for m in tree.minima] == [rows[x] for x in want["rank"]] and [m.dcal for m in tree.minima] == want["dcal"]
    assert [m.father for m in tree.minima] == want["father"] and [m.basin_size for m in tree.minima] == want["basin_size"]
    assert tree.basin_of.tolist() == want["basin"] and tree.edges == [(a, b, dcal[t]) for t, a, b in want["edges"]]
    # the saddle between two minima is the lowest level at which the flooding has them in one component
    linked = [m for m, f in enumerate(want["father"]) if f >= 0]
    for m in linked[:20]:
        assert tree.saddle(m, want["father"][m]) == want["saddle_dcal"][m] / 100.0
    # prune: shallow minima and their subtrees go, their basins are kept
    cut = tree.prune(1.0)
    assert len(cut) < len(tree) and int(cut.basin_size.sum()) == len(rows) and all(m.barrier is None or m.barrier >= 1.0 for m in cut.minima)
    assert {m.str_struct for m in cut.minima} <= {m.str_struct for m in tree.minima}
    # into the kinetics: Arrhenius rates over the exact saddles, one solve that conserves population
    k = min(8, len(tree))
    sm = tree.saddle_matrix(k)
    energy = np.array([m.dcal for m in sm["minima"]], dtype=np.float64) / 100.0
    sad = sm["saddle_dcal"] / 100.0
    adj = np.array([[a != b and tree.saddle_dcal_between(a, b) is not None for b in range(k)] for a in range(k)])
    rate = np.where(adj, np.exp(-np.maximum(energy[None, :] - energy[:, None], 0.0) / rafft_kin.KT), 0.0)
    np.fill_diagonal(rate, 0.0)
    np.fill_diagonal(rate, -rate.sum(axis=1))
    brate = rafft_kin.barrier_rates(rate, energy, sad)
    import torch
    p0 = torch.zeros(k, dtype=torch.float64)            # (eight states: the solve itself stays on the host)
    p0[k - 1] = 1.0
    traj = rafft_kin.solve_master_equation(torch.as_tensor(brate, dtype=torch.float64), energy, p0, np.array([0.0, 1.0, 100.0, 1e4]))
    assert traj.shape == (4, k) and traj[0, k - 1] > 0.999
    assert np.allclose(traj.sum(axis=-1), 1.0, atol=1e-9) and (traj > -1e-12).all()


def test_command_line_as_a_process(tmp_path):
    seqs = [LONGER[0][0], LONGER[3][0]]
    f = tmp_path / "seqs.fa"
    f.write_text(f">one\n{seqs[0]}\n>two\n{seqs[1]}\n")
    exe = [sys.executable, os.path.join(ROOT, "bin", "rafft")]
    r = subprocess.run(exe + ["-sf", str(f), "--batch", "--subopt", "2.0", "--barriers"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    trees = BR.barrier_trees(seqs, delta=2.0)
    lines = r.stdout.splitlines()
    at = 0
    for seq, tree in zip(seqs, trees):
        while lines[at].startswith(">"):
            at += 1
        assert lines[at] == seq
        table = [ln.split() for ln in lines[at + 1:at + 1 + len(tree)]]
        at += 1 + len(tree)
        # the listing parses back to the tree
        assert [int(t[0]) for t in table] == list(range(1, len(tree) + 1)) and [t[1] for t in table] == [m.str_struct for m in tree.minima]
        assert [round(float(t[2]) * 100) for t in table] == [m.dcal for m in tree.minima] and [int(t[3]) - 1 for t in table] == [m.father for m in tree.minima]
        assert [round(float(t[4]) * 100) for t in table] == [0 if m.barrier is None else round(m.barrier * 100) for m in tree.minima]
    assert at == len(lines)
    r = subprocess.run(exe + ["-s", seqs[0], "--subopt", "2.0", "--barriers", "--minh", "1.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 1 + len(trees[0].prune(1.0)), r.stderr
    r = subprocess.run(exe + ["-s", seqs[0], "--barriers"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--barriers needs --subopt" in r.stderr
