"""rafft_barriers_batch before any kernel runs: the tests' mirror (`_barriers_np.flood`, the sequential flooding
of `barriers`) equals the definition of the tree taken literally on full enumerations, under the built-in tables and an
index-sensitive set; the host-pure part of the library (the tree from edges, sizes, chunk plans) in a stand-alone C++ program, plain
and under AddressSanitizer + UBSan; the records and limits against the header; bad arguments and all-erroneous batches without a
device; BarrierTree on a constructed tree.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from rafft_amd import _native, params
from rafft_amd import barriers as BR
from conftest import ROOT
import _barriers_np as BM
import _descend_np as DS
import _loops as LP
import _par_reader as PR


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def sorted_enumeration(seq, rows):
    """the enumeration as a band: sorted by (oracle energy, enumeration order)"""
    en = [oracle.eval_structure(seq, r) for r in rows]
    order = sorted(range(len(rows)), key=lambda k: (en[k], k))
    return [rows[k] for k in order], [en[k] for k in order]


@pytest.mark.parametrize("which", ["builtin", "index"])
def test_the_mirror_is_the_definition_on_full_enumerations(which):
    if which == "index":
        oracle.set_tables(PR.tables_at(LP.index_sensitive_par(LP.builtin_par()), 37.0))
    n_min = n_links = 0
    for seq, rows in DS.start_sequences():
        assert len(rows) <= 1000
        rows, dcal = sorted_enumeration(seq, rows)
        nbs = BM.neighbour_ranks(rows)
        # the dictionary's neighbours are those of the brute-force scan over all position pairs
        for x in range(0, len(rows), 37):
            assert sorted(rows.index(new) for _, _, _, new in DS.neighbours(seq, rows[x])) == nbs[x]
        got = BM.flood(rows, dcal, nbs)
        minima, father, saddle = BM.literal_tree(rows, nbs)
        assert got["rank"] == minima and got["father"] == father and got["saddle_rank"] == saddle, (which, seq)
        assert got["rank"][0] == 0 and got["father"][0] == -1 and all(f < m for m, f in enumerate(got["father"]))
        assert sum(got["basin_size"]) == len(rows)
        # a full enumeration is connected (every structure reaches the open chain by removals): one root
        assert got["father"].count(-1) == 1
        n_min += len(minima)
        n_links += len(minima) - 1
    print(f"\n{which}: {n_min} minima, {n_links} links")
    assert n_min >= 16


def tree_by_definition(n, edges):
    """(father, saddle) of a graph of minima with weighted edges, literally: for m the smallest weight t such that the component of
    m over the edges of weight <= t holds an index below m; father: the lowest index of that component"""
    father, saddle = [-1] * n, [-1] * n
    for m in range(n):
        for t in sorted({w for _, _, w in edges}):
            comp, grew = {m}, True
            while grew:
                grew = False
                for a, b, w in edges:
                    if w <= t and (a in comp) != (b in comp):
                        comp |= {a, b}
                        grew = True
            if min(comp) < m:
                father[m], saddle[m] = min(comp), t
                break
    return father, saddle


def random_graphs(n_graphs=300, seed=20261022):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_graphs):
        n = int(rng.integers(1, 9))
        ne = int(rng.integers(0, 2 * n + 1)) if n > 1 else 0
        edges = {}
        for _ in range(ne):
            a, b = sorted(int(v) for v in rng.choice(n, 2, replace=False))
            edges[(a, b)] = int(rng.integers(0, 6))         # few distinct weights: groups of equal saddle rank are common
        out.append((n, [(a, b, w) for (a, b), w in edges.items()]))
    return out


def test_host_pure_part_against_the_tests_values_under_sanitizers(tmp_path):
    argv = []
    for n, edges in random_graphs():
        father, saddle = tree_by_definition(n, edges)
        argv += [str(n), ",".join(f"{a}-{b}-{w}" for a, b, w in edges), ",".join(map(str, father)), ",".join(map(str, saddle))]
    # ... and the graphs of minima of two enumerations, with the trees the flooding gives
    for seq, rows in DS.start_sequences()[:2]:
        rows, dcal = sorted_enumeration(seq, rows)
        got = BM.flood(rows, dcal)
        argv += [str(len(got["rank"])), ",".join(f"{a}-{b}-{t}" for t, a, b in got["edges"]), ",".join(map(str, got["father"])), ",".join(map(str, got["saddle_rank"]))]
    src = os.path.join(ROOT, "tests", "hostcheck", "barriers_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("barriers_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"{len(argv) // 4} cases, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr
    # the program does tell a wrong tree from a right one
    r = subprocess.run([exe, "3", "0-1-4,1-2-2", "-1,0,0", "-1,4,2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "1 failures" in r.stdout
    r = subprocess.run([exe, "3", "0-1-4,1-2-2", "-1,0,1", "-1,4,2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0


def test_barriers_records_and_limits_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, cls, size in (("rafft_barriers_min", _native.BarriersMin, 24), ("rafft_barriers_edge", _native.BarriersEdge, 12)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", plain).group(1)
        names = [n.strip() for n in re.search(r"int32_t([^;]*);", body).group(1).split(",")]
        assert names == [n for n, _ in cls._fields_] and ctypes.sizeof(cls) == size
    body = re.search(r"typedef struct \{([^}]*)\}\s*rafft_barriers_seq;", plain).group(1)
    assert re.findall(r"\b(\w+)\s*[;,]", body) == [n for n, _ in _native.BarriersSeq._fields_]
    assert ctypes.sizeof(_native.BarriersSeq) == 48 and ctypes.sizeof(_native.BarriersResult) == 24
    assert re.search(r"#define RAFFT_BARRIERS_MAX_LEN\s+RAFFT_MFE_MAX_LEN", hdr) and _native.BARRIERS_MAX_LEN == 4096
    assert re.search(r"#define RAFFT_BARRIERS_MAX_ROWS\s+RAFFT_SUBOPT_MAX_STRUCTS", hdr) and _native.BARRIERS_MAX_ROWS == 1 << 24
    assert {"rafft_barriers_batch", "rafft_barriers_free", "rafft_barriers_counters"} <= set(_native.EXPORTS)
    proto = re.search(r"int\s+rafft_barriers_batch\(([^;]*)\);", plain).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_barriers_batch.argtypes) == 10


def test_bad_arguments_and_erroneous_batches_need_no_device():
    L = _native.lib()
    seq = (ctypes.c_char_p * 1)(b"GGGAAAACCC")
    rowbuf = ctypes.create_string_buffer(b"(((....)))")
    rows = (ctypes.c_void_p * 1)(ctypes.addressof(rowbuf))
    dc = (ctypes.c_int32 * 1)(-120)
    dcal = (ctypes.c_void_p * 1)(ctypes.addressof(dc))
    none1 = (ctypes.c_void_p * 1)(None)
    i1 = lambda v: (ctypes.c_int * 1)(v)
    res = ctypes.POINTER(_native.BarriersResult)()
    out = ctypes.byref(res)
    E = _native.ERR_PARAM
    call = L.rafft_barriers_batch
    assert call(-1, seq, i1(10), i1(1), rows, i1(10), dcal, 0, 0, out) == E
    assert call(1, None, i1(10), i1(1), rows, i1(10), dcal, 0, 0, out) == E
    assert call(1, seq, None, i1(1), rows, i1(10), dcal, 0, 0, out) == E
    assert call(1, seq, i1(10), None, rows, i1(10), dcal, 0, 0, out) == E
    assert call(1, seq, i1(10), i1(1), None, i1(10), dcal, 0, 0, out) == E
    assert call(1, seq, i1(10), i1(1), rows, None, dcal, 0, 0, out) == E
    assert call(1, seq, i1(10), i1(1), rows, i1(10), None, 0, 0, out) == E
    assert call(1, seq, i1(10), i1(1), rows, i1(10), dcal, 0, 0, None) == E
    assert call(1, seq, i1(10), i1(1), none1, i1(10), dcal, 0, 0, out) == E
    assert call(1, seq, i1(10), i1(1), rows, i1(10), none1, 0, 0, out) == E
    assert call(1, (ctypes.c_char_p * 1)(None), i1(10), i1(1), rows, i1(10), dcal, 0, 0, out) == E
    assert call(1, seq, i1(10), i1(-1), rows, i1(10), dcal, 0, 0, out) == E           # a negative count
    assert call(1, seq, i1(10), i1(1), rows, i1(9), dcal, 0, 0, out) == E             # a stride below the length
    assert call(1, seq, i1(10), i1(1), rows, i1(10), dcal, -1, 0, out) == E           # max_edges
    assert call(1, seq, i1(10), i1(1), rows, i1(10), dcal, 0, -1, out) == E           # workspace
    assert not res                                                                   # (*out is NULL after an error)
    assert call(0, None, None, None, None, None, None, 0, 0, out) == 0 and res.contents.n_seq == 0 and res.contents.n_failed == 0
    L.rafft_barriers_free(res)
    L.rafft_barriers_free(None)
    # a batch of nothing but erroneous sequences never reaches the device
    seqs = ["", "GGGTAAAACCC", "A" * 4097, "GGGAAAACCC", "GGGAAAACCC", "GGGAAAACCA", "GGGAAAACCC"]
    rows = [[""], ["..........."], ["." * 4097], [], ["..........", "(((....))"], ["(((....)))"], ["(((....)))", ".........."]]
    dcal = [[0], [0], [0], [], [0, 0], [0], [-100, -101]]
    recs = BR.barriers_batch_raw(seqs, rows, dcal)
    S = _native.ERR_STRUCT
    assert [r["status"] for r in recs] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG, _native.ERR_EMPTY, S, S, S]
    assert [(r["length"], r["n_rows"]) for r in recs] == [(0, 1), (11, 1), (4097, 1), (10, 0), (10, 2), (10, 1), (10, 2)]
    assert all(len(r["rank"]) == 0 and len(r["basin"]) == 0 and len(r["edges"]) == 0 for r in recs)
    assert L.rafft_last_error().decode().startswith("sequence 0: empty")
    recs = BR.barriers_batch_raw(seqs[3:], rows[3:], dcal[3:])
    assert L.rafft_last_error().decode() == "sequence 0: no rows"
    BR.barriers_batch_raw(seqs[4:], rows[4:], dcal[4:])
    assert L.rafft_last_error().decode().startswith("sequence 0: row 1: malformed")
    BR.barriers_batch_raw(seqs[6:], rows[6:], dcal[6:])
    assert L.rafft_last_error().decode().startswith("sequence 0: row 1: its dcal is below")
    # a work area above the workspace is refused with its bytes, before the device
    recs = BR.barriers_batch_raw(["GGGAAAACCC"], [["(((....)))"]], [[-120]], workspace_bytes=1000)
    assert recs[0]["status"] == _native.ERR_CAPACITY
    assert L.rafft_last_error().decode() == f"sequence 0: its work area needs {56 + 16 + 12 * 2048} bytes, workspace_bytes is 1000"
    assert BR.barriers_counters() == dict(chunks=0, launches=0, rows=0, hits=0, minima=0, edges=0)
    assert L.rafft_barriers_counters(None) == E
    with pytest.raises(ValueError, match="1 rows and 2 energies"):
        BR.barriers_batch_raw(["GGGAAAACCC"], [["(((....)))"]], [[0, 0]])
    with pytest.raises(ValueError, match="one list of rows"):
        BR.barriers_batch_raw(["GGGAAAACCC"], [], [])


def constructed_tree():
    #   minimum  dcal  father saddle     barrier
    #   0        -500  -1
    #   1        -400   0     -100       3.00
    #   2        -350   1     -300       0.50
    #   3        -340   2     -320       0.20
    #   4        -300   0     -250       0.50
    #   5        -200  -1                          (a second root)
    #   6        -150   5     -100       0.50
    rows = ["m%d" % k for k in range(7)]
    dcal = [-500, -400, -350, -340, -300, -200, -150]
    father = [-1, 0, 1, 2, 0, -1, 5]
    sad = [0, -100, -300, -320, -250, 0, -100]
    size = [10, 5, 3, 2, 4, 6, 1]
    basin_of = [0] * 10 + [1] * 5 + [2] * 3 + [3] * 2 + [4] * 4 + [5] * 6 + [6]
    edges = [(0, 1, -100), (1, 2, -300), (2, 3, -320), (0, 4, -250), (5, 6, -100), (1, 3, -280)]
    return BR.BarrierTree(rows, dcal, father, sad, size, basin_of, edges)


def test_barrier_tree_saddles_and_matrix_on_a_constructed_tree():
    t = constructed_tree()
    assert len(t) == 7 and [m.father for m in t.minima] == [-1, 0, 1, 2, 0, -1, 5]
    assert [m.barrier for m in t.minima] == [None, 3.0, 0.5, 0.2, 0.5, None, 0.5] and t.minima[1].energy == -4.0
    assert t.saddle(0, 1) == -1.0 and t.saddle(1, 0) == -1.0
    assert t.saddle(2, 3) == -3.2 and t.saddle(1, 3) == -3.0            # the highest link of 3 -> 2 -> 1
    assert t.saddle(3, 4) == -1.0                                       # 3 -> 2 -> 1 -> 0 <- 4: the link 1 -> 0 is the highest
    assert t.saddle(0, 4) == -2.5 and t.saddle(2, 2) == -3.5
    assert t.saddle(0, 5) is None and t.saddle(3, 6) is None and t.saddle(5, 6) == -1.0
    sm = t.saddle_matrix(5)
    m = sm["saddle_dcal"]
    assert m.shape == (5, 5) and (m == m.T).all() and m.diagonal().tolist() == [-500, -400, -350, -340, -300]
    assert m[0].tolist() == [-500, -100, -100, -100, -250] and m[1, 2] == -300 and m[1, 3] == -300 and m[2, 3] == -320 and m[3, 4] == -100
    assert [s.str_struct for s in sm["minima"]] == ["m0", "m1", "m2", "m3", "m4"]
    full = t.saddle_matrix()["saddle_dcal"]
    assert full.shape == (7, 7) and full[0, 5] == -200 and full[4, 6] == -150 and full[5, 6] == -100      # across roots: the higher energy
    text = t.format().splitlines()
    assert text[0].split() == ["1", "m0", "-5.00", "0", "0.00"] and text[3].split() == ["4", "m3", "-3.40", "3", "0.20"]


def test_prune_folds_shallow_minima_and_their_descendants():
    t = constructed_tree()
    p = t.prune(0.4)                    # only 3 (0.20) goes, into 2
    assert [m.str_struct for m in p.minima] == ["m0", "m1", "m2", "m4", "m5", "m6"]
    assert p.father.tolist() == [-1, 0, 1, 0, -1, 4] and p.basin_size.tolist() == [10, 5, 5, 4, 6, 1]
    assert p.basin_of.tolist() == [0] * 10 + [1] * 5 + [2] * 5 + [3] * 4 + [4] * 6 + [5]
    assert p.edges == [(0, 1, -100), (0, 3, -250), (1, 2, -300), (4, 5, -100)]        # (1, 3) became a second (1, 2): the lower saddle stays
    assert p.saddle(2, 3) == -1.0 and p.minima[2].barrier == 0.5
    q = t.prune(0.6)                    # 2, 4 and 6 go (0.50), and 3 with them
    assert [m.str_struct for m in q.minima] == ["m0", "m1", "m5"] and q.basin_size.tolist() == [14, 10, 7] and q.father.tolist() == [-1, 0, -1]
    # descendants of a pruned minimum are pruned: raise 3's own barrier artificially above the cut and it still goes
    deep = BR.BarrierTree(["m%d" % k for k in range(4)], [-500, -400, -350, -340], [-1, 0, 1, 2], [0, -100, -300, -200], [1, 1, 1, 1], [0, 1, 2, 3], [])
    r = deep.prune(0.6)                 # 2 has 0.50; 3 (1.40 as constructed, which no real tree gives) hangs under 2
    assert [m.str_struct for m in r.minima] == ["m0", "m1"] and r.basin_size.tolist() == [1, 3] and r.basin_of.tolist() == [0, 1, 1, 1]
    assert len(t.prune(0.0)) == 7 and len(t.prune(100.0)) == 2 and sum(t.prune(100.0).basin_size) == 31       # roots stay
