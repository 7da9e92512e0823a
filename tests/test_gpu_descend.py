"""rafft_descend_batch on a real MI355X (`-m gpu`): on every structure of the enumerations of tests/_descend_np.py the end row, both
energies, the steps and the moves are those of the tests' own restatement of the walk over whole-structure oracle energies, under
the built-in tables and an index-sensitive set; at 60-200 nt, from sampled rows and from disturbed fold rows, every row of every path
evaluates back (eval_kernel), energies strictly fall, no neighbour of an end is lower and the move taken is the smallest
(dE, i, j) of all neighbours - neighbours generated here, from the loops' members; the edges of the move set up to 4096 nt and the
step bound; same input - same bits across batch position, order, duplicates, chunking, NULL moves and strides; errors that stay with
their item; another temperature; Python and the command line.  Integers and bytes: no tolerance."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import rafft_amd
from rafft_amd import _native as N, descend as DSm, findpath as FPm, mccaskill, params, rafft as R
from conftest import ROOT
import _descend_np as DS
from _descend_np import all_neighbours, move_row
import _loops as LP
import _par_reader as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    win = LP.index_sensitive_par(builtin)
    win.update(ml_closing=-700, ml_intern=-300)
    out = dict(builtin=builtin, index=idx, multiloops_win=win, synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name in ("index", "multiloops_win", "synthetic"):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=name)
    return out


def install(sets, which):
    if which == "builtin":
        params.reset_params()
        oracle.reset_tables()
    else:
        params.load_params(sets["paths"][which])
        oracle.set_tables(PR.tables_at(sets[which], 37.0))


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()
    oracle.reset_tables()


def rand(rng, n, letters="ACGU"):
    return "".join(rng.choice(list(letters), n))


def flat(seqs, rows, **kw):
    """one walk per entry of (seqs, rows): a list of dict(status, n_steps, start_dcal, end_dcal, end, moves) in input order"""
    srec, rrec, ends, moves = DSm.descend_batch_raw(list(seqs), [[r] for r in rows], **kw)
    out = []
    for s in range(len(seqs)):
        assert srec[s]["n_rows"] == 1 and srec[s]["row0"] == s
        out.append(dict(seq_status=srec[s]["status"], status=int(rrec[s]["status"][0]), n_steps=int(rrec[s]["n_steps"][0]), start_dcal=int(rrec[s]["start_dcal"][0]),
                        end_dcal=int(rrec[s]["end_dcal"][0]), end=DSm.end_rows(ends[s], srec[s]["length"])[0],
                        moves=None if moves is None else [tuple(m) for m in moves[s][0].tolist()]))
    return out


def same_as_mirror(got, want, what):
    assert got["status"] == want["status"] and got["end"] == want["end"] and got["n_steps"] == want["n_steps"], (what, got, want)
    assert got["start_dcal"] == want["start_dcal"] and got["end_dcal"] == want["end_dcal"] and got["moves"] == want["moves"], (what, got, want)


# ---- neighbours, stated a third way (_descend_np.all_neighbours: from the loops' members)

def disturbed(rng, seq, row, n_remove, n_add):
    """`row` with some pairs removed and random legal pairs added, one after the other"""
    for _ in range(n_remove):
        pairs = DS.pairs_of(row)
        if pairs:
            i, j = pairs[int(rng.integers(len(pairs)))]
            row = move_row(row, i, j, True)
    for _ in range(n_add):
        adds = [n for n in all_neighbours(seq, row) if not n[2]]
        if adds:
            i, j, _ = adds[int(rng.integers(len(adds)))]
            row = move_row(row, i, j, False)
    return row


def walk_checks(seqs, rows, got, temp=37.0, sampled_steps=3, seed=5):
    """for walks that ended: every row of every path evaluates back; energies strictly fall; no neighbour of an end is lower; on up
    to `sampled_steps` steps per walk the move taken is the smallest (dE, i, j) below 0 of all neighbours.  One eval_structures call."""
    rng = np.random.default_rng(seed)
    q_seq, q_row, plan = [], [], []

    def ask(seq, row):
        q_seq.append(seq)
        q_row.append(row)
        return len(q_row) - 1

    for seq, row, g in zip(seqs, rows, got):
        assert g["status"] == 0 and len(g["moves"]) == g["n_steps"]
        path = FPm.path_rows(row, np.array(g["moves"], dtype=np.int64).reshape(-1, 2))
        assert path[-1] == g["end"]
        at = [ask(seq, r) for r in path]
        look = sorted(set(rng.choice(g["n_steps"], min(sampled_steps, g["n_steps"]), replace=False).tolist())) if g["n_steps"] else []
        probes = []
        for k in look + [g["n_steps"]]:
            nb = all_neighbours(seq, path[k])
            probes.append((k, nb, [ask(seq, move_row(path[k], i, j, rem)) for i, j, rem in nb]))
        plan.append((g, at, probes))
    en, st = R.eval_structures(q_seq, q_row, temp=temp)
    assert not any(st)
    for g, at, probes in plan:
        e = [en[x] for x in at]
        assert e[0] == g["start_dcal"] and e[-1] == g["end_dcal"] and all(a > b for a, b in zip(e, e[1:])), (g, e)
        for k, nb, idx in probes:
            below = sorted((en[x] - e[k], i, j, rem) for (i, j, rem), x in zip(nb, idx) if en[x] < e[k])
            if k == g["n_steps"]:
                assert not below, (g, k, below[:3])
            else:
                dE, i, j, rem = below[0]
                assert g["moves"][k] == ((-i - 1, -j - 1) if rem else (i, j)) and e[k + 1] - e[k] == dE, (g, k, below[:3])
    return len(q_row)


# ---- the list of starts

@pytest.mark.parametrize("which", ["builtin", "index"])
def test_every_structure_of_the_enumerations_in_one_call(sets, which):
    install(sets, which)
    want = DS.mirror_walks(which)
    groups = DS.start_sequences()
    srec, rrec, ends, moves = DSm.descend_batch_raw([s for s, _ in groups], [rows for _, rows in groups])
    k = 0
    for s, (seq, rows) in enumerate(groups):
        assert srec[s] == dict(status=0, length=len(seq), n_rows=len(rows), row0=k)
        end = DSm.end_rows(ends[s], len(seq))
        for r, row in enumerate(rows):
            got = dict(status=int(rrec[s]["status"][r]), n_steps=int(rrec[s]["n_steps"][r]), start_dcal=int(rrec[s]["start_dcal"][r]),
                       end_dcal=int(rrec[s]["end_dcal"][r]), end=end[r], moves=[tuple(m) for m in moves[s][r].tolist()])
            same_as_mirror(got, want[k + r], (which, seq, row))
        k += len(rows)
    cnt = (ctypes.c_longlong * 4)()
    N.lib().rafft_descend_counters(ctypes.byref(cnt))
    assert list(cnt) == [1, 1, len(want), sum(w["n_steps"] for w in want)]
    # the neighbours as this file states them are those of the restatement
    for seq, row in DS.starts()[::97]:
        assert sorted(all_neighbours(seq, row)) == sorted((i, j, rem) for i, j, rem, _ in DS.neighbours(seq, row))


_LONG = {}


def longer_starts():
    """(seqs, rows): 60-200-nt sequences; per sequence four sampled rows (seeded) and four rows of the fold (the best of the final
    beam) with 3-7 pairs removed and 3-8 random legal pairs added"""
    if not _LONG:
        rng = np.random.default_rng(777)
        seqs = [rand(rng, n) for n in (60, 75, 90, 120, 150, 200)]
        samples = mccaskill.sample_batch(seqs, 4, seeds=11)
        folds = rafft_amd.fold_batch(seqs, nb_mode=50, max_stack=10, max_branch=100)
        out_s, out_r = [], []
        for s, sm, f in zip(seqs, samples, folds):
            best = min(f, key=lambda x: x.dcal).str_struct
            for st in sm:
                out_s.append(s); out_r.append(st.str_struct)
            for _ in range(4):
                out_s.append(s); out_r.append(disturbed(rng, s, best, int(rng.integers(3, 8)), int(rng.integers(3, 9))))
        _LONG["v"] = (out_s, out_r)
    return _LONG["v"]


def test_longer_sequences_from_sampled_and_disturbed_rows():
    seqs, rows = longer_starts()
    got = flat(seqs, rows)
    steps = [g["n_steps"] for g in got]
    kinds = {m[0] < 0 for g in got for m in g["moves"]}
    print(f"\nsteps: {steps}")
    assert max(steps) >= 10 and kinds == {True, False}
    en = DS.cached_energy()
    n_mirror = 0
    for seq, row, g in zip(seqs, rows, got):
        if len(seq) <= 120:
            same_as_mirror(g, DS.walk(seq, row, 0, en), (seq, row))
            n_mirror += 1
    assert n_mirror >= 24
    print(f"{walk_checks(seqs, rows, got)} rows evaluated back")


@pytest.mark.parametrize("L", DS.STRIDE_LENGTHS)
def test_lengths_where_the_lanes_stride(L):
    """63, 64, 65 and 129 positions, where a lane's share x = lane, lane + 64, ... gains a position: random rows from the open chain
    to one with no room left, exactly the restatement's walks"""
    seq, rows = DS.stride_rows(L)
    en = DS.cached_energy()
    want = [DS.walk(seq, row, 0, en) for row in rows]
    assert {m[0] < 0 for w in want for m in w["moves"]} == {True, False} and max(w["n_steps"] for w in want) >= 9
    got = flat([seq] * len(rows), rows)
    for row, g, w in zip(rows, got, want):
        same_as_mirror(g, w, (L, row))


# ---- edges

def test_edges_of_the_move_set(sets):
    hp = "GGGGAAAACCCC"
    long_loop = "GGG" + "A" * 34 + "CCC"
    cases = [
        ("A", "."), ("GC", ".."), ("GAC", "..."), ("GAAC", "...."),                 # lengths 1-4: nothing can pair
        ("A" * 40, "." * 40),                                                       # poly-A
        (hp, "............"),                                                       # the open chain of a sequence that folds
        ("AAAAAAAAAAAAUUUU" * 8, "." * 128),
        (hp, "((((....))))"),                                                       # a start that is a minimum
        ("GAAAAAAAAAAAAAAAAC", "(................)"),                               # a lonely pair that is removed
        (hp, "(..........)"),
        (long_loop, "(((" + "." * 34 + ")))"), (long_loop, "(.(" + "." * 34 + ").)"),      # a hairpin of 34, an interior loop of 34 + 1 ...
        ("GGGAAAAAAAAAAAAAAAAGGGAAAACCCAAAAAAAAAAAAAAAAAACCC", "(((................(((....)))..................)))"),      # an interior loop of 16 + 18 > 30
        ("NGGGAAAACCCN", ".(((....)))."), ("GGGNAAAANCCC", "(((......)))"), ("NNNNNNNNNNNN", "............"), ("GGGNAAAANCCC", "............"),      # N positions
    ]
    seqs, rows = map(list, zip(*cases))
    got = flat(seqs, rows)
    en = DS.cached_energy()
    for (seq, row), g in zip(cases, got):
        same_as_mirror(g, DS.walk(seq, row, 0, en), (seq, row))
    assert [g["n_steps"] for g in got[:5]] == [0] * 5 and all(g["end"] == r for g, (_, r) in zip(got[:5], cases))
    assert got[5]["n_steps"] == 0 and got[6]["n_steps"] == 0            # (a single pair costs energy: the open chain is a minimum)
    assert got[7]["n_steps"] == 0 and got[7]["end"] == cases[7][1]
    assert got[8]["moves"] == [(-1, -18)] and got[8]["end"] == "." * 18
    assert got[9]["n_steps"] >= 1
    walk_checks(seqs, rows, got)
    # a multiloop closing and opening, under tables under which multiloops win
    install(sets, "multiloops_win")
    ml = "GAGAAACGAAACGAAACC"
    ml_rows = ["..(...)(...)......", "(.(...)(...).....)", "(.(...)..........)", "." * 18]
    got = flat([ml] * 4, ml_rows)
    en = DS.cached_energy()
    for row, g in zip(ml_rows, got):
        same_as_mirror(g, DS.walk(ml, row, 0, en), (ml, row))
    assert got[0]["moves"] == [(0, 16)] and got[0]["end"] == "(.(...)(...)....)."           # a pair closes around two helices
    walk_checks([ml] * 4, ml_rows, got)
    # ... and under the built-in tables, where this multiloop costs energy, its closing pair is the first to go
    install(sets, "builtin")
    got = flat([ml] * 2, ml_rows[1:3])
    en = DS.cached_energy()
    for row, g in zip(ml_rows[1:3], got):
        same_as_mirror(g, DS.walk(ml, row, 0, en), (ml, row))
    assert got[0]["moves"][0] == (-1, -18) and got[0]["end"] == "." * 18
    walk_checks([ml] * 2, ml_rows[1:3], got)


def hairpin_chain(n_units, open_units):
    """n_units of GGGGAAAACCCC + AA; the units in open_units start with their two inner pairs missing"""
    seq = "".join("GGGGAAAACCCC" + "AA" for _ in range(n_units))
    row = "".join(("((........))" if u in open_units else "((((....))))") + ".." for u in range(n_units))
    return seq, row


def test_long_walks_and_the_step_bound():
    rng = np.random.default_rng(31)
    s1500 = rand(rng, 1500)
    best = min(rafft_amd.fold_batch([s1500], nb_mode=50, max_stack=10, max_branch=100)[0], key=lambda x: x.dcal).str_struct
    r1500 = disturbed(rng, s1500, best, 6, 6)
    s4096, r4096 = hairpin_chain(292, {3, 100, 291})
    s4096, r4096 = s4096 + "A" * 8, r4096 + "." * 8
    assert len(s4096) == len(r4096) == 4096
    short = [DS.starts()[k] for k in (5, 400, 1800, 3000)]
    seqs = [short[0][0], s1500, short[1][0], short[2][0], s4096, short[3][0]]
    rows = [short[0][1], r1500, short[1][1], short[2][1], r4096, short[3][1]]
    free = flat(seqs, rows)
    assert all(g["status"] == 0 for g in free) and free[4]["n_steps"] == 6 and free[1]["n_steps"] >= 4
    assert free[4]["end"] == hairpin_chain(292, set())[1] + "." * 8
    walk_checks(seqs, rows, free, sampled_steps=1)
    want = DS.mirror_walks()
    for k, at in zip((0, 2, 3, 5), (5, 400, 1800, 3000)):
        same_as_mirror(free[k], want[at], at)
    # max_steps = 3: the walks that need more stop with CAPACITY three steps along, the others are as before
    cut = flat(seqs, rows, max_steps=3)
    for row, g, f in zip(rows, cut, free):
        if f["n_steps"] <= 3:
            assert g == f
        else:
            assert g["status"] == N.ERR_CAPACITY and g["n_steps"] == 3 and g["moves"] == f["moves"][:3] and g["start_dcal"] == f["start_dcal"]
            assert g["end"] == FPm.path_rows(row, np.array(f["moves"][:3]))[-1]
    assert cut[4]["status"] == N.ERR_CAPACITY and cut[1]["status"] == N.ERR_CAPACITY
    assert N.lib().rafft_last_error().decode().startswith("sequence 1 row 0: not at a minimum after 3 steps")
    e3, st = R.eval_structures([s4096, s1500], [cut[4]["end"], cut[1]["end"]])
    assert not any(st) and e3 == [cut[4]["end_dcal"], cut[1]["end_dcal"]]
    # ... and a continuation from the rows they reached ends where the unbounded walk ends
    more = flat(seqs, [g["end"] for g in cut])
    for g, c, f in zip(more, cut, free):
        assert g["status"] == 0 and g["end"] == f["end"] and g["end_dcal"] == f["end_dcal"] and c["n_steps"] + g["n_steps"] == f["n_steps"]
        assert c["moves"] + g["moves"] == f["moves"] and g["start_dcal"] == c["end_dcal"]
    # a bound of exactly the steps a walk needs is no error
    exact = flat([s4096], [r4096], max_steps=6)[0]
    assert exact == free[4]


# ---- same input, same bits

def bits(srec, rrec, ends, moves, s, r):
    return (tuple(int(rrec[s][k][r]) for k in ("status", "n_steps", "start_dcal", "end_dcal")), ends[s][r].tobytes(),
            None if moves is None else moves[s][r].tobytes())


def test_same_input_same_bits():
    picks = [DS.starts()[k] for k in range(0, len(DS.starts()), 131)]
    ls, lr = longer_starts()
    picks += list(zip(ls, lr))[::5]
    seqs, rows = map(list, zip(*picks))
    base = DSm.descend_batch_raw(seqs, [[r] for r in rows])
    want = [bits(*base, s, 0) for s in range(len(seqs))]
    assert any(w[0][1] >= 3 for w in want)
    # reversed, with duplicates, one walk per chunk
    order = list(range(len(seqs)))[::-1] + [2, 2, 9]
    got = DSm.descend_batch_raw([seqs[k] for k in order], [[rows[k]] for k in order], workspace_bytes=1)
    cnt = (ctypes.c_longlong * 4)()
    N.lib().rafft_descend_counters(ctypes.byref(cnt))
    assert cnt[0] == cnt[1] == cnt[2] == len(order)
    assert [bits(*got, x, 0) for x in range(len(order))] == [want[k] for k in order]
    # alone
    for k in (0, 4, len(seqs) - 1):
        one = DSm.descend_batch_raw([seqs[k]], [[rows[k]]])
        assert bits(*one, 0, 0) == want[k]
    # several rows of one sequence in one block, duplicated, at strides L and L + 1
    seq, erows = DS.start_sequences()[2]
    sub = erows[::7] + erows[:3]
    each = DSm.descend_batch_raw([seq] * len(sub), [[r] for r in sub])
    for pad in (0, 1):
        block = np.zeros((len(sub), len(seq) + pad), dtype=np.uint8)
        for k, r in enumerate(sub):
            block[k, :len(seq)] = np.frombuffer(r.encode(), dtype=np.uint8)
        if pad:
            block[:, -1] = ord("(")             # (what lies between the rows is not read)
        tog = DSm.descend_batch_raw([seq], [block])
        assert [bits(*tog, 0, r) for r in range(len(sub))] == [bits(*each, r, 0) for r in range(len(sub))]
    # without the moves: the same records and rows
    bare = DSm.descend_batch_raw(seqs, [[r] for r in rows], moves=False)
    assert bare[3] is None and [bits(*bare, s, 0)[:2] for s in range(len(seqs))] == [w[:2] for w in want]
    # moves for some sequences only
    L = N.lib()
    n = 3
    enc, arr, lens = N.seq_arrays(seqs[:n])
    blocks = [np.frombuffer(rows[s].encode(), dtype=np.uint8).copy() for s in range(n)]
    outs = [np.zeros(len(rows[s]) + 1, dtype=np.uint8) for s in range(n)]
    mv1 = np.full((2 * len(rows[1]) + 16, 2), 77, dtype=np.int32)
    srec, rrec = (N.DescendSeq * n)(), np.zeros((n, 4), dtype=np.int32)
    rc = L.rafft_descend_batch(n, arr, lens, (ctypes.c_int * n)(1, 1, 1), (ctypes.c_void_p * n)(*[b.ctypes.data for b in blocks]), (ctypes.c_int * n)(*[len(r) for r in rows[:n]]),
                               37.0, 0, 0, srec, rrec.ctypes.data, (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs]), (ctypes.c_void_p * n)(None, mv1.ctypes.data, None))
    assert rc == 0
    for s in range(n):
        assert tuple(rrec[s].tolist()) == want[s][0] and outs[s].tobytes() == want[s][1]
    k1 = want[1][0][1]
    assert mv1[:k1].tobytes() == want[1][2] and (mv1[k1:] == 77).all()


# ---- statuses and parameters

def test_errors_stay_with_their_item():
    L = N.lib()
    good_seq, good_rows = DS.start_sequences()[1]
    good_rows = good_rows[3:40:6]
    alone = DSm.descend_batch_raw([good_seq], [good_rows], max_steps=5)
    want = [bits(*alone, 0, r) for r in range(len(good_rows))]
    long_open = hairpin_chain(4, {0, 1, 2, 3})
    seqs = ["", good_seq, "GGGTAAAACCC", "A" * (N.DESCEND_MAX_LEN + 1), good_seq, "GGGAAAACCC", long_open[0]]
    rows = [[""], good_rows, ["(((.....)))"], ["." * (N.DESCEND_MAX_LEN + 1)], good_rows[::-1],
            ["(((....)))", "(((....))", "(((....)).", "(((.[].)))", "(((..)..))", "..........", "((......))"], [long_open[1], hairpin_chain(4, set())[1]]]
    srec, rrec, ends, moves = DSm.descend_batch_raw(seqs, rows, max_steps=5)
    assert [q["status"] for q in srec] == [N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, N.ERR_TOO_LONG, 0, 0, 0]
    assert rrec[0]["status"].tolist() == [N.ERR_EMPTY] and rrec[2]["status"].tolist() == [N.ERR_BAD_CHAR] and rrec[3]["status"].tolist() == [N.ERR_TOO_LONG]
    assert rrec[5]["status"].tolist() == [0, N.ERR_STRUCT, N.ERR_STRUCT, N.ERR_STRUCT, N.ERR_STRUCT, 0, 0]
    assert rrec[6]["status"].tolist() == [N.ERR_CAPACITY, 0] and rrec[6]["n_steps"].tolist() == [5, 0]
    assert L.rafft_last_error().decode().startswith("sequence 0: empty")
    # rows with an error come back as they went in (a sequence's error: dots), and nothing is reported for them
    assert DSm.end_rows(ends[5], 10)[1:5] == ["(((....))\0", "(((....)).", "(((.[].)))", "(((..)..))"] and DSm.end_rows(ends[2], 11) == ["." * 11]
    for s in (0, 2, 3):
        assert not rrec[s]["n_steps"].any() and not rrec[s]["end_dcal"].any()
    assert not rrec[5]["n_steps"][1:5].any() and all(len(m) == 0 for m in moves[5][1:5])
    # the neighbours are untouched
    assert [bits(srec, rrec, ends, moves, 1, r) for r in range(len(good_rows))] == want
    assert [bits(srec, rrec, ends, moves, 4, r) for r in range(len(good_rows))] == want[::-1]
    # the three good rows between the bad ones
    e, st = R.eval_structures(["GGGAAAACCC"] * 3, [DSm.end_rows(ends[5], 10)[r] for r in (0, 5, 6)])
    assert not any(st) and e == [int(rrec[5]["end_dcal"][r]) for r in (0, 5, 6)]
    # nothing but erroneous items, and bad arguments: the device is not touched (no allocation)
    before, after = (ctypes.c_ulonglong * 5)(), (ctypes.c_ulonglong * 5)()
    L.rafft_alloc_counters(ctypes.byref(before))
    bad = DSm.descend_batch_raw([seqs[0], seqs[2], seqs[3], seqs[5]], [rows[0], rows[2], rows[3], rows[5][1:5]])
    assert [q["status"] for q in bad[0]] == [N.ERR_EMPTY, N.ERR_BAD_CHAR, N.ERR_TOO_LONG, 0] and bad[1][3]["status"].tolist() == [N.ERR_STRUCT] * 4
    seq = (ctypes.c_char_p * 1)(b"GGGAAAACCC")
    rowbuf = ctypes.create_string_buffer(b"(((....)))")
    rp = (ctypes.c_void_p * 1)(ctypes.addressof(rowbuf))
    out = ctypes.create_string_buffer(11)
    db = (ctypes.c_void_p * 1)(ctypes.addressof(out))
    i1 = lambda v: (ctypes.c_int * 1)(v)
    sr, rr = (N.DescendSeq * 1)(), (N.DescendRow * 1)()
    ra = ctypes.addressof(rr)
    call = L.rafft_descend_batch
    assert call(-1, seq, i1(10), i1(1), rp, i1(10), 37.0, 0, 0, sr, ra, db, None) == N.ERR_PARAM
    assert call(1, None, i1(10), i1(1), rp, i1(10), 37.0, 0, 0, sr, ra, db, None) == N.ERR_PARAM
    assert call(1, seq, i1(10), i1(1), None, i1(10), 37.0, 0, 0, sr, ra, db, None) == N.ERR_PARAM
    assert call(1, seq, i1(10), i1(1), rp, i1(10), 37.0, 0, 0, sr, None, db, None) == N.ERR_PARAM
    assert call(1, seq, i1(10), i1(-1), rp, i1(10), 37.0, 0, 0, sr, ra, db, None) == N.ERR_PARAM
    assert call(1, seq, i1(10), i1(1), rp, i1(9), 37.0, 0, 0, sr, ra, db, None) == N.ERR_PARAM
    assert call(1, seq, i1(10), i1(1), rp, i1(10), 37.0, -1, 0, sr, ra, db, None) == N.ERR_PARAM
    assert call(1, seq, i1(10), i1(1), rp, i1(10), 37.0, 0, -1, sr, ra, db, None) == N.ERR_PARAM
    assert call(1, seq, i1(10), i1(1), rp, i1(10), 25.0, 0, 0, sr, ra, db, None) == N.ERR_TEMP          # the built-in tables have no enthalpies
    L.rafft_alloc_counters(ctypes.byref(after))
    assert list(before) == list(after)
    assert call(1, seq, i1(10), i1(1), rp, i1(10), 37.0, 0, 0, sr, ra, db, None) == 0 and rr[0].status == 0 and out.value == b"(((....)))"


def test_another_temperature_with_a_loaded_parameter_file(sets):
    params.load_params(sets["paths"]["synthetic"])
    picks = [DS.starts()[k] for k in range(0, len(DS.starts()), 211)]
    ls, lr = longer_starts()
    picks += list(zip(ls, lr))[4::8]
    seqs, rows = map(list, zip(*picks))
    ends = {}
    for temp in (25.0, 60.0):
        got = flat(seqs, rows, temp=temp)
        walk_checks(seqs, rows, got, temp=temp)
        ends[temp] = [(g["start_dcal"], g["end"]) for g in got]
    assert ends[25.0] != ends[60.0]


# ---- Python and the command line

def test_minima_of_the_full_enumeration_are_the_structures_that_do_not_move():
    groups = DS.start_sequences()[:4]
    want = DS.mirror_walks()
    got = DSm.minima_batch([s for s, _ in groups], [rows for _, rows in groups])
    k = 0
    for (seq, rows), (minima, counts, basin_of) in zip(groups, got):
        mine = want[k:k + len(rows)]
        k += len(rows)
        still = [(w["end_dcal"], r, w["end"]) for r, w in enumerate(mine) if w["n_steps"] == 0]
        assert {m.str_struct for m in minima} == {row for _, _, row in still} and len(minima) == len(still)
        assert [m.dcal for m in minima] == sorted(e for e, _, _ in still) and sum(counts) == len(rows)
        assert [minima[b].str_struct for b in basin_of.tolist()] == [w["end"] for w in mine]
        assert counts == [sum(w["end"] == m.str_struct for w in mine) for m in minima]
        first = [next(r for r, w in enumerate(mine) if w["end"] == m.str_struct) for m in minima]
        assert all((a.dcal, x) < (b.dcal, y) for a, b, x, y in zip(minima, minima[1:], first, first[1:]))


def test_basin_graph_saddles_lie_above_both_minima():
    seq, rows = DS.start_sequences()[0]
    g = DSm.basin_graph(seq, rows, width=16, max_minima=6)
    m = len(g["minima"])
    assert 2 <= m <= 6 and g["saddle_dcal"].shape == (m, m) and (g["saddle_dcal"] == g["saddle_dcal"].T).all()
    for a in range(m):
        assert g["saddle_dcal"][a, a] == g["minima"][a].dcal
        for b in range(a + 1, m):
            assert g["saddle_dcal"][a, b] >= max(g["minima"][a].dcal, g["minima"][b].dcal)
    full = DSm.minima_batch([seq], [rows])[0]
    assert [x.str_struct for x in g["minima"]] == [x.str_struct for x in full[0][:m]] and g["counts"] == full[1][:m]
    assert ((g["basin_of"] == -1) == (full[2] >= m)).all() and (g["basin_of"][full[2] < m] == full[2][full[2] < m]).all()


def test_command_line_as_a_process(tmp_path):
    groups = DS.start_sequences()[:2]
    f = tmp_path / "rows.txt"
    f.write_text(f">first\n{groups[0][0]}\n" + "\n".join(groups[0][1][:60]) + f"\n\n{groups[1][0]}\n" + "\n".join(groups[1][1][:50]) + "\n")
    exe = [sys.executable, os.path.join(ROOT, "bin", "rafft")]
    r = subprocess.run(exe + ["-sf", str(f), "--descend"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = DSm.minima_batch([groups[0][0], groups[1][0]], [groups[0][1][:60], groups[1][1][:50]])
    want = []
    for name, (seq, _), (minima, counts, _) in zip((">first", None), groups, got):
        want += ([name] if name else []) + [seq] + [f"{m.str_struct} {m.dcal / 100.0:7.2f} {c}" for m, c in zip(minima, counts)]
    assert r.stdout.splitlines() == want
    # with --sample and with --subopt: a one-step graph of minima with counts that the graph reader takes
    seq = groups[0][0]
    for mode, total in ((["--sample", "200", "--seed", "3"], 200), (["--subopt", "3.0"], None)):
        out = tmp_path / "graph.out"
        r = subprocess.run(exe + ["-s", seq, "--descend", "-o", str(out)] + mode, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = out.read_text().splitlines()
        assert lines[0] == seq and lines[1].startswith("# --") and len(lines) >= 3
        table = [ln.split() for ln in lines[2:]]
        assert all(len(t) == 3 for t in table) and [float(t[1]) for t in table] == sorted(float(t[1]) for t in table)
        assert len({t[0] for t in table}) == len(table) and (total is None or sum(int(t[2]) for t in table) == total)
        ends = flat([seq] * len(table), [t[0] for t in table])
        assert all(g["n_steps"] == 0 for g in ends)
        steps, s2 = rafft_amd.parse_rafft_output(str(out))
        assert s2 == seq and [st.str_struct for st in steps[0]] == [t[0] for t in table]
    r = subprocess.run(exe + ["-sf", str(f), "--descend", "--max-steps", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "max_steps" in r.stderr
