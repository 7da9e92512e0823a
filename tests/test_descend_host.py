"""rafft_descend_batch before any kernel runs: the tests' own restatement of the walk (`_descend_np.walk`,
whole-structure oracle energies, neighbours from a brute-force scan) equals a steepest descent done on the neighbour graph of the
full enumeration alone, under the built-in tables and an index-sensitive set, and the distinct ends are exactly the starts that do
not move; the host-pure part of the library (row parsing, sizes, chunk plans) in a stand-alone C++ program, plain and under
AddressSanitizer + UBSan; the records and limits against the header; bad arguments and all-erroneous batches without a device; the
grouping of ends into minima.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from rafft_amd import _native, params
from rafft_amd import descend as DSm
from conftest import ROOT
import _descend_np as DS
import _loops as LP
import _par_reader as PR


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def graph_descent(seq, rows):
    """per row of the enumeration the end of the steepest descent on the enumeration's own neighbour graph: rows are neighbours
    when their pair sets differ by one pair - (i, j) -, energies are looked up by row index"""
    sets = [frozenset(DS.pairs_of(r)) for r in rows]
    index = {s: k for k, s in enumerate(sets)}
    en = [oracle.eval_structure(seq, r) for r in rows]
    all_pairs = sorted({p for s in sets for p in s})
    nxt = []
    for k, s in enumerate(sets):
        best = None
        for p in all_pairs:
            o = index.get(s ^ {p})
            if o is not None and en[o] < en[k]:
                key = (en[o] - en[k], p[0], p[1], o)
                best = key if best is None or key < best else best
        nxt.append(k if best is None else best[3])
    ends, steps = [], []
    for k in range(len(rows)):
        n = 0
        while nxt[k] != k:
            k, n = nxt[k], n + 1
        ends.append(k)
        steps.append(n)
    return ends, steps, en


@pytest.mark.parametrize("which", ["builtin", "index"])
def test_the_restatement_is_the_steepest_descent_on_the_enumeration(which):
    if which == "index":
        oracle.set_tables(PR.tables_at(LP.index_sensitive_par(LP.builtin_par()), 37.0))
    walks = DS.mirror_walks(which)
    st = DS.stats(walks)
    print(f"\n{which}: {st}")
    if which == "builtin":
        DS.check_conditions(st)
    k = 0
    for seq, rows in DS.start_sequences():
        assert 16 <= len(seq) <= 22 and 8 <= len(rows) <= 1000
        ends, steps, en = graph_descent(seq, rows)
        mine = walks[k:k + len(rows)]
        k += len(rows)
        assert [w["end"] for w in mine] == [rows[e] for e in ends], (which, seq)
        assert [w["n_steps"] for w in mine] == steps and [w["start_dcal"] for w in mine] == en and [w["end_dcal"] for w in mine] == [en[e] for e in ends]
        # the distinct ends are exactly the starts that do not move
        assert {w["end"] for w in mine} == {w["end"] for w in mine if w["n_steps"] == 0}
        assert len({w["end"] for w in mine}) == sum(w["n_steps"] == 0 for w in mine)
        for w in mine:
            assert all(a > b for a, b in zip(w["dcal"], w["dcal"][1:])) and w["status"] == 0 and len(w["moves"]) == w["n_steps"]
    assert k == len(walks) == len(DS.starts())


def test_the_step_bound_of_the_restatement():
    seq, row = next((s, r) for (s, r), w in zip(DS.starts(), DS.mirror_walks()) if w["n_steps"] >= 4)
    full = DS.walk(seq, row)
    cut = DS.walk(seq, row, 2)
    assert cut["status"] == DS.ERR_CAPACITY and cut["n_steps"] == 2 and cut["moves"] == full["moves"][:2] and cut["end_dcal"] == full["dcal"][2]
    rest = DS.walk(seq, cut["end"])
    assert rest["end"] == full["end"] and rest["n_steps"] == full["n_steps"] - 2
    exact = DS.walk(seq, row, full["n_steps"])          # a bound of exactly the steps it needs is no error
    assert exact["status"] == 0 and exact["end"] == full["end"]


PARSE_CASES = [
    # (sequence, row, status): nested, unbalanced, a foreign character, the wrong length, a hairpin of 2, a non-canonical pair, N
    ("GGGGAAAACCCC", "((((....))))", 0), ("GGGGAAAACCCC", "(.(......).)", 0), ("GGGAAACCCGGGAAACCC", "(((...)))(((...)))", 0),
    ("GGGGAAAACCCC", "............", 0), ("G", ".", 0), ("GAAAC", "(...)", 0),
    ("GGGGAAAACCCC", "((((....))).", 8), ("GGGGAAAACCCC", ".(((....))))", 8), ("GGGGAAAACCCC", ")(((....)))(", 8),
    ("GGGGAAAACCCC", "(((([..]))))", 8), ("GGGGAAAACCCC", "<(((....)))>", 8), ("GGGGAAAACCCC", "((((....)))) ", 0),
    ("GGGGAAAACCCC", "((((....)))", 8), ("GGGGAAAACCCC", "", 8),
    ("GGGGAACCCC", "((((..))))", 8), ("GGGGACCCC", "((((.))))", 8), ("GGCC", "(())", 8), ("GAAC", "(..)", 8),
    ("GGGGAAAACCCA", "((((....))))", 8), ("AGGGAAAACCCA", "((((....))))", 8),
    ("NGGGAAAACCCN", "((((....))))", 8), ("NGGGAAAACCCN", ".(((....))).", 0), ("GGGNAAAANCCC", "(((......)))", 0), ("GGGNAAAANCCC", "((((....))))", 8),
]


def test_host_pure_part_against_the_tests_values_under_sanitizers(tmp_path):
    argv = []
    for seq, row, st in PARSE_CASES:
        # (a row longer than the sequence: the library reads the sequence's length of it - the one case the mirror does not speak of)
        want = DS.parse_status(seq, row[:len(seq)]) if len(row) > len(seq) else DS.parse_status(seq, row)
        assert want == st, (seq, row, want, st)
        argv += [seq, row, str(st), ",".join(f"{i}-{j}" for i, j in DS.pairs_of(row)) if st == 0 else ""]
    # ... and a slice of the list of starts, all valid
    for seq, row in DS.starts()[::40]:
        assert DS.parse_status(seq, row) == 0
        argv += [seq, row, "0", ",".join(f"{i}-{j}" for i, j in DS.pairs_of(row))]
    src = os.path.join(ROOT, "tests", "hostcheck", "descend_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("descend_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"{len(argv) // 4} cases, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr
    # the program does tell a wrong table from a right one
    r = subprocess.run([exe, "GGGGAAAACCCC", "((((....))))", "0", "0-11,1-10,2-9,3-7"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "1 failures" in r.stdout


def move_set_cases():
    """(sequence, row): the valid rows of PARSE_CASES, a slice of the starts, rows constructed for the edges of the walks, random rows
    at the lengths where the lanes' stride of 64 turns over"""
    cases = [(seq, row[:len(seq)]) for seq, row, st in PARSE_CASES if st == 0] + DS.starts()[::40]
    hp, two = "GGGGAAAACCCC", "A" + "GGGAAACCC" + "U" + "GGGAAACCC" + "U"
    cases += [("G", "."), ("GAAC", "...."), ("GAAAC", "....."), ("GAAAC", "(...)"),            # L = 1, 4 and 5, the shortest row with a possible pair
              (hp, "." * 12), ("AAAAAAAAAAAAUUUU" * 4, "." * 64),                               # open chains
              (two, "." + "(((...)))" + "." + "(((...)))" + "."),                                # an exterior loop of two helices, a partner directly behind each
              (two, "." + "(((...)))" + "." + "........." + "."), (two, "(" + "(((...)))" + ")" + "(((...)))" + "."),
              ("GAGAAACGAAACGAAACC", "(.(...)(...).....)"), ("GAGAAACGAAACGAAACC", "..(...)(...)......"),      # a multiloop, and before it closes
              ("GAAAAAAAAAAAAAAAAC", "(................)"), (hp, "(..........)"), (hp, "(.(......).)"),           # lonely pairs
              ("GGGNAAAANCCC", "(((......)))"), ("GGGNAAAANCCC", "." * 12), ("NNNNNNNNNNNN", "." * 12), ("NGGGAAAACCCN", ".(((....)))."), ("UNNNNAUNNNNA", "." * 12)]
    for L in DS.STRIDE_LENGTHS:
        seq, rows = DS.stride_rows(L)
        cases += [(seq, row) for row in rows]
    return cases


def test_move_set_positions_against_brute_force_on_the_host(tmp_path):
    """rafft_moves.h's enclosing_pair and next_partner, host-only: the moves they yield equal the program's own brute force, the
    restatement's brute-force scan (DS.neighbours) and the loops' members (DS.all_neighbours) - three statements against the one
    under test -, with next_partner bounded by the enclosing pair and by L"""
    argv = []
    for seq, row in move_set_cases():
        assert DS.parse_status(seq, row) == 0, (seq, row)
        want = sorted((i, j, rem) for i, j, rem, _ in DS.neighbours(seq, row))
        assert want == DS.all_neighbours(seq, row), (seq, row)
        argv += [seq, row, ",".join(f"{i}-{j}-{'r' if rem else 'a'}" for i, j, rem in want)]
    assert len(argv) // 3 >= 90 and any(len(a) > 5000 for a in argv[2::3]) and "" in argv[2::3]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "moves_check")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-missing-braces",
                           os.path.join(ROOT, "tests", "hostcheck", "moves_check.cpp"), "-o", exe])
    r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"{len(argv) // 3} cases, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr[-2000:]
    # the program does tell a wrong list from a right one: a move too few, a move too many, a removal called an addition
    for wrong in ("0-11-r,1-10-r,2-9-r", "0-11-r,1-10-r,2-9-r,3-8-r,4-8-a", "0-11-r,1-10-r,2-9-r,3-8-a"):
        r = subprocess.run([exe, "GGGGAAAACCCC", "((((....))))", wrong], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "1 cases, 2 failures" in r.stdout, (wrong, r.stdout + r.stderr)


def test_descend_records_and_limits_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    for name, cls, fields in (("rafft_descend_seq", _native.DescendSeq, ["status", "length", "n_rows", "row0"]),
                              ("rafft_descend_row", _native.DescendRow, ["status", "n_steps", "start_dcal", "end_dcal"])):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", hdr).group(1), flags=re.S)
        names = [n.strip() for n in re.findall(r"\bint32_t\s+(\w+);", body)]
        assert names == [n for n, _ in cls._fields_] == fields
        assert ctypes.sizeof(cls) == 16
    assert re.search(r"#define RAFFT_DESCEND_MAX_LEN\s+RAFFT_MFE_MAX_LEN", hdr) and _native.DESCEND_MAX_LEN == 4096
    assert {"rafft_descend_batch", "rafft_descend_counters"} <= set(_native.EXPORTS)
    proto = re.search(r"int rafft_descend_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_descend_batch.argtypes) == 13


def test_bad_arguments_and_erroneous_batches_need_no_device():
    L = _native.lib()
    seq = (ctypes.c_char_p * 1)(b"GGGAAAACCC")
    rowbuf = ctypes.create_string_buffer(b"(((....)))")
    rows = (ctypes.c_void_p * 1)(ctypes.addressof(rowbuf))
    out = ctypes.create_string_buffer(11)
    db = (ctypes.c_void_p * 1)(ctypes.addressof(out))
    i1 = lambda v: (ctypes.c_int * 1)(v)
    srec, rrec = (_native.DescendSeq * 1)(), (_native.DescendRow * 1)()
    rp = ctypes.addressof(rrec)
    E = _native.ERR_PARAM
    call = L.rafft_descend_batch
    assert call(-1, seq, i1(10), i1(1), rows, i1(10), 37.0, 0, 0, srec, rp, db, None) == E
    assert call(1, None, i1(10), i1(1), rows, i1(10), 37.0, 0, 0, srec, rp, db, None) == E
    assert call(1, seq, None, i1(1), rows, i1(10), 37.0, 0, 0, srec, rp, db, None) == E
    assert call(1, seq, i1(10), None, rows, i1(10), 37.0, 0, 0, srec, rp, db, None) == E
    assert call(1, seq, i1(10), i1(1), None, i1(10), 37.0, 0, 0, srec, rp, db, None) == E
    assert call(1, seq, i1(10), i1(1), rows, None, 37.0, 0, 0, srec, rp, db, None) == E
    assert call(1, seq, i1(10), i1(1), rows, i1(10), 37.0, 0, 0, None, rp, db, None) == E
    assert call(1, seq, i1(10), i1(1), rows, i1(10), 37.0, 0, 0, srec, None, db, None) == E
    assert call(1, seq, i1(10), i1(1), rows, i1(10), 37.0, 0, 0, srec, rp, None, None) == E
    assert call(1, seq, i1(10), i1(1), (ctypes.c_void_p * 1)(None), i1(10), 37.0, 0, 0, srec, rp, db, None) == E
    assert call(1, seq, i1(10), i1(1), rows, i1(10), 37.0, 0, 0, srec, rp, (ctypes.c_void_p * 1)(None), None) == E
    assert call(1, seq, i1(10), i1(-1), rows, i1(10), 37.0, 0, 0, srec, rp, db, None) == E          # a negative count
    assert call(1, seq, i1(10), i1(1), rows, i1(9), 37.0, 0, 0, srec, rp, db, None) == E            # a stride below the length
    assert call(1, seq, i1(10), i1(1), rows, i1(10), 37.0, -1, 0, srec, rp, db, None) == E          # max_steps
    assert call(1, seq, i1(10), i1(1), rows, i1(10), 37.0, 0, -1, srec, rp, db, None) == E          # workspace
    assert call(1, seq, i1(10), i1(1), rows, i1(10), 25.0, 0, 0, srec, rp, db, None) == _native.ERR_TEMP    # the built-in tables have no enthalpies
    assert call(0, None, None, None, None, None, 37.0, 0, 0, None, None, None, None) == 0
    # a sequence without rows needs neither rows nor an output
    assert call(1, seq, i1(10), i1(0), (ctypes.c_void_p * 1)(None), i1(10), 37.0, 0, 0, srec, None, (ctypes.c_void_p * 1)(None), None) == 0
    assert (srec[0].status, srec[0].length, srec[0].n_rows, srec[0].row0) == (0, 10, 0, 0)
    # a batch of nothing but erroneous items never reaches the device
    seqs = ["", "GGGTAAAACCC", "A" * 4097, "GGGAAAACCC", "GGGAAAACCA"]
    rows = [[""], ["(((.....)))", "..........."], ["." * 4097], ["(((....))", "(((....)).", "(((.[].)))", "(((..)..))"], ["(((....)))"]]
    srec, rrec, ends, moves = DSm.descend_batch_raw(seqs, rows)
    assert [q["status"] for q in srec] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG, 0, 0]
    assert [(q["length"], q["n_rows"], q["row0"]) for q in srec] == [(0, 1, 0), (11, 2, 1), (4097, 1, 3), (10, 4, 4), (10, 1, 8)]
    assert [r["status"].tolist() for r in rrec] == [[_native.ERR_EMPTY], [_native.ERR_BAD_CHAR] * 2, [_native.ERR_TOO_LONG], [_native.ERR_STRUCT] * 4, [_native.ERR_STRUCT]]
    assert all(not r["n_steps"].any() and not r["start_dcal"].any() and not r["end_dcal"].any() for r in rrec)
    # a sequence's error: rows of dots; a row's error: the row as it went in
    assert DSm.end_rows(ends[1], 11) == ["." * 11] * 2 and DSm.end_rows(ends[2], 4097) == ["." * 4097] and ends[0].tolist() == [[0]]
    assert ends[3].tobytes() == b"(((....))\0\0" + b"(((....)).\0" + b"(((.[].)))\0" + b"(((..)..))\0" and ends[4].tobytes() == b"(((....)))\0"
    assert all(len(m) == 0 for per in moves for m in per)
    assert L.rafft_last_error().decode().startswith("sequence 0: empty")
    srec, rrec, _, _ = DSm.descend_batch_raw(seqs[3:], rows[3:], moves=False)
    assert L.rafft_last_error().decode().startswith("sequence 0 row 0: malformed")
    cnt = (ctypes.c_longlong * 4)()
    assert L.rafft_descend_counters(ctypes.byref(cnt)) == 0 and list(cnt) == [0, 0, 0, 0]
    assert L.rafft_descend_counters(None) == E
    with pytest.raises(ValueError, match="sequence 0 row 0"):
        DSm.descend_batch(seqs[3:4], rows[3:4])
    with pytest.raises(KeyError):
        DSm.descend_batch(seqs[1:2], rows[1:2])
    with pytest.raises(ValueError, match="4096 nt"):
        DSm.descend_batch(seqs[2:3], rows[2:3])
    with pytest.raises(ValueError, match="longer than its sequence"):
        DSm.descend_batch_raw(["GGGAAAACCC"], [["(((....)))."]])
    assert DSm.descend_batch(seqs[1:2], rows[1:2], raise_errors=False) == [None]


def test_group_minima_on_constructed_ends():
    ends = ["b", "a", "b", "c", "a", "b", "d"]
    dcal = [-5, -7, -5, -5, -7, -5, 0]
    mins, counts, basin_of = DSm.group_minima(ends, dcal)
    # energy ascending; equal energies by first appearance (b at 0 before c at 3)
    assert mins == [("a", -7), ("b", -5), ("c", -5), ("d", 0)] and counts == [2, 3, 1, 1] and basin_of.tolist() == [1, 0, 1, 2, 0, 1, 3]
    assert DSm.group_minima([], [])[0] == [] and DSm.group_minima([], [])[2].tolist() == []
    one = DSm.group_minima(["x"] * 4, [3] * 4)
    assert one[0] == [("x", 3)] and one[1] == [4] and one[2].tolist() == [0] * 4
    # first appearance decides, not text order
    assert [m for m, _ in DSm.group_minima(["z", "y"], [1, 1])[0]] == ["z", "y"]


def test_row_blocks_of_the_python_call():
    a, stride = DSm._row_block(["((...))", "......."], 7)
    assert stride == 7 and a.shape == (2, 7) and a.tobytes() == b"((...))......."
    a, stride = DSm._row_block(["(...)"], 7)                   # shorter: padded with NULs
    assert a.tobytes() == b"(...)\0\0"
    arr = np.frombuffer(b"((...))\0.......\0", dtype=np.uint8).reshape(2, 8)
    a, stride = DSm._row_block(arr, 7)
    assert stride == 8 and a.tobytes() == arr.tobytes()
    a, stride = DSm._row_block([], 0)
    assert a.shape == (0, 1) and stride == 1
