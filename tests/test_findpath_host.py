"""rafft_findpath_batch before any kernel runs: the tests' own restatement of the search
(`_findpath_np.search`, whole-structure oracle energies) finds the exact lowest saddle of the short problems at width 256 - nothing is
dropped there - under the built-in tables and an index-sensitive set, and loses against it at width 1 on some; the host-pure part of
the library (moves, conflict masks of one, two and three words, sizes, chunk plans) in a stand-alone C++ program under AddressSanitizer + UBSan; the records and
limits against the header; bad arguments and erroneous problems without a device; barrier_rates on a constructed graph.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from rafft_amd import _native, params, rafft_kin
from rafft_amd import findpath as FPm
from conftest import ROOT
import _findpath_cases as FC
import _findpath_np as FP
import _loops as LP
import _par_reader as PR


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


@pytest.mark.parametrize("which", ["builtin", "index"])
def test_mirror_at_width_256_is_the_exact_search_and_width_1_loses(which):
    if which == "index":
        oracle.set_tables(PR.tables_at(LP.index_sensitive_par(LP.builtin_par()), 37.0))
    probs = FP.host_problems()
    assert len(probs) >= 100 and all(16 <= len(s) <= 22 for s, _, _ in probs)
    n_conflict = n_loss = 0
    for seq, a, b in probs:
        mv, n_rem = FP.move_list(a, b)
        assert 1 <= len(mv) <= 10
        n_conflict += any(FP.conflict_masks(mv, n_rem))
        exact = FP.exact_saddle(seq, a, b)
        wide, narrow = FP.search(seq, a, b, 256), FP.search(seq, a, b, 1)
        assert wide["saddle_dcal"] == exact, (which, seq, a, b)
        assert narrow["saddle_dcal"] >= exact, (which, seq, a, b)
        n_loss += narrow["saddle_dcal"] > exact
        for r in (wide, narrow):
            rows = FPm.path_rows(a, r["moves"])
            assert rows[-1] == b and [oracle.eval_structure(seq, x) for x in rows] == r["dcal"]
            assert r["saddle_dcal"] == max(r["dcal"]) and r["dcal"][r["saddle_step"]] == r["saddle_dcal"] and max(r["dcal"][:r["saddle_step"]], default=-10 ** 9) < r["saddle_dcal"]
    print(f"\n{which}: {len(probs)} problems, {n_conflict} with a conflict, width 1 loses on {n_loss}")
    assert 2 * n_conflict >= len(probs)
    if which == "builtin":
        assert n_loss >= 2


def describe(a, b):
    mv, n_rem = FP.move_list(a, b)
    conf = FP.conflict_masks(mv, n_rem)
    mw = max(1, (len(mv) + 63) // 64)
    words = lambda c: ":".join(format(c >> (64 * w) & (2 ** 64 - 1), "x") for w in range(mw))
    return f"{n_rem};" + ",".join(f"{i}-{j}" for i, j in mv) + ";" + ",".join(words(c) for c in conf[n_rem:])


def test_host_pure_part_against_the_tests_values_under_sanitizers(tmp_path):
    S, OKAY = str(_native.ERR_STRUCT), "0"
    hp = "GGGGAAAACCCC"
    cases = [
        # move order: removals ascending, then additions ascending; a crossing pair, shared bases, nested and disjoint pairs
        ("GGGGGAAAACCCCC", "((((.....)))).", ".((((....)))).", OKAY, None),
        ("GGGAAAACCCAAAGGC", "(((....)))......", "(..............)", OKAY, "3;0-9,1-8,2-7,0-15;1"),                # shares base 0 with (0,9) only
        ("GGGAAACCCGGGAAACCC", "(((...))).........", ".........(((...)))", OKAY, "3;0-8,1-7,2-6,9-17,10-16,11-15;0,0,0"),      # disjoint: no conflict
        ("GGGGAAAACCCC", "(..(....)..)", "((........))", OKAY, "1;3-8,1-10;0"),                                  # nested inside a kept pair and around a removal: none
        ("GGGAAAGGGAAACCCAAACCC", "(((...............)))", "......(((...)))......", OKAY, "3;0-20,1-19,2-18,6-14,7-13,8-12;0,0,0"),   # nested: none
        ("GGGAAAGGGCCCAAACCCAAA", "(((......)))........." , "......(((......)))...", OKAY, "3;0-11,1-10,2-9,6-17,7-16,8-15;7,7,7"),                 # crossing, from the mirror
        (hp, "((((....))))", "((((....))))", OKAY, "0;;"),                                                       # d = 0
        (hp, "............", "((((....))))", OKAY, "0;0-11,1-10,2-9,3-8;0,0,0,0"),
        (hp, "((((....)))", "............", S, ""), (hp, "((((....))))", "...........", S, ""),                  # another length
        (hp, "((((....))).", "............", S, ""), (hp, "............", ".(((....))))", S, ""),                # unbalanced
        (hp, "((((....))))", "....[..]....", S, ""), (hp, "<(((....)))>", "............", S, ""),                # foreign characters
        (hp, "............", "....(..)....", S, ""),                                                             # A-A
        ("NGGGAAAACCCN", "((((....))))", "............", S, ""),                                                 # N pairs with nothing
    ]
    argv = []
    for seq, a, b, st, desc in cases:
        if desc is None or st == OKAY:
            want = describe(a, b)
            assert desc is None or desc == want, (seq, a, b, desc, want)
            desc = want
        argv += [seq, a, b, st, desc]
    # ... and every problem of the list, as the mirror describes it
    n_cross = 0
    for seq, a, b in FP.host_problems():
        argv += [seq, a, b, OKAY, describe(a, b)]
        mv, n_rem = FP.move_list(a, b)
        n_cross += any(FP.conflict_masks(mv, n_rem))
    assert n_cross >= 50
    # ... and the problems of two and three mask words (_findpath_cases): removals and conflict words past bit 63
    wide = [prob for _, prob, *_ in FC.removal_cases() + FC.addition_cases() + FC.dedup_cases()]
    assert sorted({FC.mask_words(FC.dist(p)[0]) for p in wide}) == [1, 2, 3]
    for seq, a, b in wide:
        argv += [seq, a, b, OKAY, describe(a, b)]
    assert describe(*wide[7][1:]).split(";")[2].split(",")[:2] == ["8000000000000000:1:0", "0:3:0"]
    crossing =describe("(((......))).........", "......(((......)))...")
    assert crossing == "3;0-11,1-10,2-9,6-17,7-16,8-15;7,7,7"
    src = os.path.join(ROOT, "tests", "hostcheck", "findpath_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("findpath_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"{len(argv) // 5} cases, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr
    # the program does tell a wrong description from a right one
    r = subprocess.run([exe, hp, "............", "((((....))))", OKAY, "0;0-11,1-10,2-9,3-8;0,0,0,1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "1 failures" in r.stdout


def test_findpath_record_and_limits_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\}\s*rafft_findpath_rec;", hdr).group(1), flags=re.S)
    names = [n.strip() for n in re.findall(r"\bint32_t\s+(\w+);", body)]
    assert names == [n for n, _ in _native.FindpathRec._fields_] == ["status", "length", "dist", "start_dcal", "end_dcal", "saddle_dcal", "saddle_step", "_pad"]
    assert ctypes.sizeof(_native.FindpathRec) == 32
    assert re.search(r"#define RAFFT_FINDPATH_MAX_WIDTH\s+1024", hdr) and _native.FINDPATH_MAX_WIDTH == 1024
    assert re.search(r"#define RAFFT_FINDPATH_MAX_CANDIDATES \(1 << 20\)", hdr) and _native.FINDPATH_MAX_CANDIDATES == 1 << 20
    assert re.search(r"#define RAFFT_FINDPATH_MAX_LEN\s+RAFFT_MFE_MAX_LEN", hdr) and _native.FINDPATH_MAX_LEN == 4096
    assert {"rafft_findpath_batch", "rafft_findpath_counters"} <= set(_native.EXPORTS)
    proto = re.search(r"int rafft_findpath_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_findpath_batch.argtypes) == 11


def test_bad_arguments_and_erroneous_problems_need_no_device():
    L = _native.lib()
    seq, a, b = (ctypes.c_char_p * 1)(b"GGGAAAACCC"), (ctypes.c_char_p * 1)(b"(((....)))"), (ctypes.c_char_p * 1)(b"..........")
    ln, rec = (ctypes.c_int * 1)(10), (_native.FindpathRec * 1)()
    w = lambda v: (ctypes.c_int * 1)(v)
    E = _native.ERR_PARAM
    assert L.rafft_findpath_batch(-1, seq, ln, a, b, w(4), 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, None, ln, a, b, w(4), 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, None, a, b, w(4), 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, None, b, w(4), 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, a, None, w(4), 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, a, b, None, 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(4), 37.0, 0, None, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(0), 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(_native.FINDPATH_MAX_WIDTH + 1), 37.0, 0, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(4), 37.0, -1, rec, None, None) == E
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(4), 25.0, 0, rec, None, None) == _native.ERR_TEMP        # the built-in tables have no enthalpies
    assert L.rafft_findpath_batch(0, None, None, None, None, None, 37.0, 0, None, None, None) == 0
    # a batch of nothing but erroneous problems never reaches the device
    n = 1025
    probs = [("", "", ""), ("GGGTAAAACCC", "(((.....)))", "..........."), ("A" * 4097, "." * 4097, "." * 4097),
             ("GGGAAAACCC", "(((....))", ".........."), ("GGGAAAACCA", "(((....)))", ".........."),
             ("G" * n + "AAA" + "C" * n, "(" * n + "..." + ")" * n, "." * (2 * n + 3))]
    s, x, y = map(list, zip(*probs))
    recs, moves, dcal = FPm.findpath_batch_raw(s, x, y, [16] * 5 + [1024])
    assert [r["status"] for r in recs] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG, _native.ERR_STRUCT, _native.ERR_STRUCT, _native.ERR_CAPACITY]
    assert all(r["length"] == 0 for r in recs) and recs[5]["dist"] == n and all(len(m) == 0 for m in moves) and all(len(d) == 0 for d in dcal)
    assert L.rafft_last_error().decode().startswith("problem 0: empty")
    recs, _, _ = FPm.findpath_batch(s[3:5], x[3:5], y[3:5], raise_errors=False)
    assert [r["status"] for r in recs] == [_native.ERR_STRUCT] * 2 and L.rafft_last_error().decode().startswith("problem 0: a row")
    with pytest.raises(ValueError, match="problem 0"):
        FPm.findpath_batch(s[3:4], x[3:4], y[3:4])
    with pytest.raises(KeyError):
        FPm.findpath_batch(s[1:2], x[1:2], y[1:2])
    with pytest.raises(ValueError, match="4096 nt"):
        FPm.findpath_batch(s[2:3], x[2:3], y[2:3])
    with pytest.raises(_native.RafftError):
        FPm.findpath_batch(s[5:], x[5:], y[5:], width=1024)


def test_path_rows_and_reverse_path():
    mv = np.array([[-1, -7], [1, 5], [-2, -6]], dtype=np.int32)
    rows = FPm.path_rows("((...))", mv[:1])
    assert rows == ["((...))", ".(...)."]
    assert FPm.path_rows("(.....)", [(-1, -7), (1, 5)]) == ["(.....)", ".......", ".(...)."]
    back, en = FPm.reverse_path([(-1, -7), (1, 5)], [3, 9, 4])
    assert back.tolist() == [[-2, -6], [0, 6]] and en.tolist() == [4, 9, 3]
    assert FPm.path_rows(".(...).", back) == [".(...).", ".......", "(.....)"]
    assert FPm.path_rows("....", np.zeros((0, 2), dtype=np.int32)) == ["...."]


def test_barrier_rates_on_a_constructed_graph():
    kt = rafft_kin.KT
    en = np.array([0.0, -2.5, -1.0, -6.0, 3.0])
    edges = [(0, 1), (0, 2), (1, 3), (2, 3), (2, 4)]
    metro = np.zeros((5, 5))
    for i, j in edges:
        metro[i, j] = min(1.0, np.exp(-(en[j] - en[i]) / kt))
        metro[j, i] = min(1.0, np.exp(-(en[i] - en[j]) / kt))
    np.fill_diagonal(metro, -metro.sum(axis=1))
    top = np.maximum(en[:, None], en[None, :])
    # saddles equal to max(E_i, E_j) reproduce the Metropolis matrix - bit for bit off the diagonal
    same = rafft_kin.barrier_rates(metro, en, top, kt)
    assert np.array_equal(same - np.diag(np.diag(same)), metro - np.diag(np.diag(metro))) and np.allclose(np.diag(same), np.diag(metro), rtol=1e-15)
    # saddles below the endpoints are clamped
    assert np.array_equal(rafft_kin.barrier_rates(metro, en, top - 5.0, kt), same)
    # saddles above: both directions of an edge shrink by the same factor
    sad = top + np.array([[0, 1.5, 0.0, 9, 9], [1.5, 0, 9, 0.25, 9], [0.0, 9, 0, 4.0, 0.7], [9, 0.25, 4.0, 0, 9], [9, 9, 0.7, 9, 0]])
    got = rafft_kin.barrier_rates(metro, en, sad, kt)
    for i, j in edges:
        f = np.exp(-(sad[i, j] - top[i, j]) / kt)
        assert got[i, j] == metro[i, j] * f and got[j, i] == metro[j, i] * f
        assert got[i, j] <= metro[i, j] and (got[i, j] < metro[i, j]) == (sad[i, j] > top[i, j])
        # detailed balance with respect to the energies
        assert np.isclose(got[i, j] * np.exp(-en[i] / kt), got[j, i] * np.exp(-en[j] / kt), rtol=1e-12, atol=0.0)
    off = ~np.eye(5, dtype=bool)
    assert np.array_equal((got != 0) & off, (metro != 0) & off)
    assert np.abs(got.sum(axis=1)).max() <= 1e-12 * np.abs(got).max()
    # the lower triangle of `saddle` is not looked at, nor are entries without an edge
    junk = np.triu(sad) + np.tril(np.full((5, 5), -77.0), -1)
    assert np.array_equal(rafft_kin.barrier_rates(metro, en, junk, kt), got)
