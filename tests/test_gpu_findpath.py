"""rafft_findpath_batch on a real MI355X (`-m gpu`): on the short problems of tests/_findpath_np.py the saddle at width 256 is the
exact one (dynamic programming over all subsets of moves) and moves and energies are those of the tests' own restatement of the
search over whole-structure oracle energies, under the built-in tables and an index-sensitive set; the same restatement at 60-200 nt
and five widths; every row of every path evaluates back (eval_kernel) up to 1500 nt; the edges of the move set; same input - same
bits across batch position, order, duplicates, chunking and NULL paths; errors that stay with their problem; another temperature;
Python, the command line and the kinetics hook.  Integers and bytes: no tolerance."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import rafft_amd
from rafft_amd import _native as N, findpath as FPm, params, rafft as R, rafft_kin, zuker
from conftest import ROOT
import _findpath_np as FP
import _loops as LP
import _par_reader as PR

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 7, 16, 64)


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


def run(probs, widths, **kw):
    seqs, a, b = zip(*probs) if probs else ((), (), ())
    return FPm.findpath_batch_raw(list(seqs), list(a), list(b), widths, **kw)


def bits(recs, moves, dcal, k):
    return (tuple(recs[k].items()), moves[k].tobytes(), dcal[k].tobytes())


def same_as_mirror(prob, width, rec, moves, dcal, want=None):
    """`want`: what FP.search(*prob, width) returned, where the caller holds it already"""
    want = want or FP.search(*prob, width)
    assert rec["status"] == 0 and rec["length"] == rec["dist"] == want["dist"], (prob, width, rec)
    got = {k: rec[k] for k in ("start_dcal", "end_dcal", "saddle_dcal", "saddle_step")}
    assert got == {k: want[k] for k in got}, (prob, width, rec, want)
    assert [tuple(m) for m in moves.tolist()] == want["moves"], (prob, width)
    assert dcal.tolist() == want["dcal"], (prob, width)


def evaluate_back(probs, recs, moves, dcal, temp=37.0):
    """every row of every path has the path's energy at that step (eval_kernel, one call); consecutive rows differ by one pair; the
    first row is A and the last is B; the record's saddle is the maximum and saddle_step its first position"""
    flat_s, flat_r, want = [], [], []
    for (seq, a, b), rec, mv, en in zip(probs, recs, moves, dcal):
        assert rec["status"] == 0 and len(mv) == rec["length"] == rec["dist"] and len(en) == rec["dist"] + 1
        rows = FPm.path_rows(a, mv)
        assert rows[0] == a and rows[-1] == b
        for x, y in zip(rows, rows[1:]):
            assert len(FP.pairs_of(x) ^ FP.pairs_of(y)) == 1
        e = en.tolist()
        assert rec["start_dcal"] == e[0] and rec["end_dcal"] == e[-1] and rec["saddle_dcal"] == max(e) and rec["saddle_step"] == e.index(max(e))
        flat_s += [seq] * len(rows)
        flat_r += rows
        want += e
    got, st = R.eval_structures(flat_s, flat_r, temp=temp)
    assert not any(st) and list(got) == want
    return len(want)


_LONG = {}


def longer_problems():
    """60-200-nt sequences with A = the fast-folding end point at max_stack 1 and B = the best of max_stack 50 (the oracle's fold)"""
    if not _LONG:
        rng = np.random.default_rng(4242)
        probs = []
        for n in (60, 75, 90, 120, 200):
            for _ in range(2):
                s = rand(rng, n)
                a = oracle.fold(s, max_stack=1)[0].str_struct
                b = min(oracle.fold(s, max_stack=50), key=lambda x: x.dcal).str_struct
                probs.append((s, a, b))
        _LONG["p"] = probs
    return _LONG["p"]


@pytest.mark.parametrize("which", ["builtin", "index"])
def test_width_256_is_exact_on_the_short_problems_and_equals_the_mirror(sets, which):
    install(sets, which)
    probs = FP.host_problems()
    recs, moves, dcal = run(probs, 256)
    for k, prob in enumerate(probs):
        assert recs[k]["saddle_dcal"] == FP.exact_saddle(*prob), (which, prob)
        same_as_mirror(prob, 256, recs[k], moves[k], dcal[k])


def test_longer_problems_equal_the_mirror_at_five_widths():
    probs = longer_problems()
    ds = [len(FP.move_list(a, b)[0]) for _, a, b in probs]
    assert max(ds) >= 9 and sum(d > 0 for d in ds) >= 6, ds
    batch = [p for p in probs for _ in WIDTHS]
    widths = [w for _ in probs for w in WIDTHS]
    recs, moves, dcal = run(batch, widths)
    n_width_matters = 0
    for k, prob in enumerate(probs):
        for x, w in enumerate(WIDTHS):
            i = k * len(WIDTHS) + x
            same_as_mirror(prob, w, recs[i], moves[i], dcal[i])
        n_width_matters += len({recs[k * len(WIDTHS) + x]["saddle_dcal"] for x in range(len(WIDTHS))}) > 1
    print(f"\nd = {ds}; the width changes the saddle on {n_width_matters} of {len(probs)} problems")
    assert n_width_matters >= 1


def test_every_row_of_every_path_evaluates_back():
    rng = np.random.default_rng(99)
    long_seqs = [rand(rng, 300), rand(rng, 1500)]
    folds = rafft_amd.fold_batch(long_seqs, nb_mode=100, max_stack=20, max_branch=100)
    a = [min(f, key=lambda x: x.dcal).str_struct for f in folds]
    b = [m.str_struct for m in zuker.mfe_batch(long_seqs)]
    short = FP.host_problems()[:40] + longer_problems()
    probs = short[:25] + [(long_seqs[0], a[0], b[0])] + short[25:] + [(long_seqs[1], a[1], b[1])]
    widths = [256] * 25 + [64] + [256] * 15 + [16] * len(longer_problems()) + [8]
    recs, moves, dcal = run(probs, widths)
    print(f"\n300 nt: d = {recs[25]['dist']}, 1500 nt: d = {recs[-1]['dist']}")
    assert recs[25]["dist"] > 10 and recs[-1]["dist"] > 50
    evaluate_back(probs, recs, moves, dcal)


def test_edges_of_the_move_set(sets):
    hp = "GGGGAAAACCCC"
    long_loop = "GGG" + "A" * 34 + "CCC"
    probs = [
        (hp, "((((....))))", "((((....))))"),                                   # d = 0
        (hp, "............", "((((....))))"),                                   # open chain to a structure
        (hp, "((((....))))", "............"),                                   # ... and back
        # a hairpin shifted by one position: every addition conflicts with a removal, and a removal must come first
        ("GGGGGAAAACCCCC", "((((.....)))).", ".((((....))))."),
        # A and B share one base of a pair: (0,9) against (0,15)
        ("GGGAAAACCCAAAGGC", "(((....)))......", "(..............)"),
        ("NGGGAAAACCCN", ".(((....))).", "............"),                       # N bases
        ("GGGNAAAANCCC", "(((......)))", "((........))"),
        # a loop of more than 30 unpaired positions on the way: an interior loop of 34 + 1 and a hairpin of 36
        (long_loop, "(((" + "." * 34 + ")))", "." * 40),
        (long_loop, "." * 40, "(.(" + "." * 34 + ").)"),
    ]
    for s, a, b in probs:
        assert len(s) == len(a) == len(b), (s, a, b)
    recs, moves, dcal = run(probs, 16)
    assert [r["dist"] for r in recs[:3]] == [0, 4, 4] and recs[0]["saddle_dcal"] == recs[0]["start_dcal"] and len(dcal[0]) == 1 and len(moves[0]) == 0
    assert all(tuple(m)[0] < 0 for m in moves[2].tolist()) and all(tuple(m)[0] >= 0 for m in moves[1].tolist())
    mv, n_rem = FP.move_list(probs[3][1], probs[3][2])
    assert all(FP.conflict_masks(mv, n_rem)[n_rem:]) and moves[3][0][0] < 0
    for k, prob in enumerate(probs):
        same_as_mirror(prob, 16, recs[k], moves[k], dcal[k])
    evaluate_back(probs, recs, moves, dcal)
    # a multiloop closing and opening, under tables under which multiloops win
    install(sets, "multiloops_win")
    ml = "GAGAAACGAAACGAAACC"
    rows = ["(.(...)(...).....)", "." * 18, "..(...)(...)......"]
    ml_probs = [(ml, rows[2], rows[0]), (ml, rows[0], rows[2]), (ml, rows[1], rows[0]), (ml, rows[0], rows[1])]
    recs, moves, dcal = run(ml_probs, 16)
    for k, prob in enumerate(ml_probs):
        same_as_mirror(prob, 16, recs[k], moves[k], dcal[k])
        assert recs[k]["saddle_dcal"] == FP.exact_saddle(*prob)
    evaluate_back(ml_probs, recs, moves, dcal)


def test_same_input_same_bits():
    probs = FP.host_problems()[:30] + longer_problems()[:4]
    widths = [(1, 3, 16, 256)[k % 4] for k in range(len(probs))]
    recs, moves, dcal = run(probs, widths)
    want = [bits(recs, moves, dcal, k) for k in range(len(probs))]
    # reversed, with duplicates, one problem per chunk
    order = list(range(len(probs)))[::-1] + [3, 3, 17]
    r2, m2, d2 = run([probs[k] for k in order], [widths[k] for k in order], workspace_bytes=1)
    cnt = (ctypes.c_longlong * 4)()
    N.lib().rafft_findpath_counters(ctypes.byref(cnt))
    assert cnt[0] == len(order) == cnt[3]
    assert [bits(r2, m2, d2, x) for x in range(len(order))] == [want[k] for k in order]
    # alone
    for k in (0, 7, len(probs) - 1):
        r1, m1, d1 = run([probs[k]], [widths[k]])
        assert bits(r1, m1, d1, 0) == want[k]
    # without the paths
    r3, m3, d3 = run(probs, widths, paths=False)
    assert m3 is None and d3 is None and r3 == recs


def test_errors_stay_with_their_problem():
    L = N.lib()
    good = FP.host_problems()[:3]
    n_stack = 1024
    deep = lambda n: ("G" * n + "AAA" + "C" * n, "(" * n + "..." + ")" * n, "." * (2 * n + 3))
    bad = [
        ("", "", ""),                                                        # EMPTY
        ("GGGTAAAACCC", "(((.....)))", "..........."),                       # BAD_CHAR
        ("A" * (N.FINDPATH_MAX_LEN + 1), "." * (N.FINDPATH_MAX_LEN + 1), "." * (N.FINDPATH_MAX_LEN + 1)),      # TOO_LONG
        ("GGGAAAACCC", "(((....))", ".........."),                           # a row of another length
        ("GGGAAAACCC", "(((....)).", ".........."),                          # unbalanced
        ("GGGAAAACCC", "(((....)))", "....[]...."),                          # a foreign character
        ("GGGAAAACCA", "(((....)))", ".........."),                          # a non-canonical pair (G-A)
        deep(n_stack + 1),                                                   # width 1024 x 1025 moves
        ("GGGCCC", "((()))", "......"),                                      # a hairpin of no position: its energy leaves the key's range
    ]
    want_status = [N.ERR_EMPTY, N.ERR_BAD_CHAR, N.ERR_TOO_LONG, N.ERR_STRUCT, N.ERR_STRUCT, N.ERR_STRUCT, N.ERR_STRUCT, N.ERR_CAPACITY, N.ERR_CAPACITY]
    alone = run(good, 16)
    probs, widths = [], []
    for k, b in enumerate(bad):
        probs += [b, good[k % 3]]
        widths += [1024 if k == 7 else 16, 16]
    recs, moves, dcal = run(probs, widths)
    assert [r["status"] for r in recs[0::2]] == want_status
    assert all(r["length"] == 0 and len(m) == 0 and len(d) == 0 for r, m, d in zip(recs[0::2], moves[0::2], dcal[0::2]))
    assert recs[14]["dist"] == n_stack + 1
    assert L.rafft_last_error().decode().startswith("problem 0")
    for x in range(len(bad)):
        assert bits(recs, moves, dcal, 2 * x + 1) == bits(*alone, x % 3)
    # nothing but erroneous problems: the device is not touched (no allocation)
    before, after = (ctypes.c_ulonglong * 5)(), (ctypes.c_ulonglong * 5)()
    L.rafft_alloc_counters(ctypes.byref(before))
    recs, _, _ = run(bad[:8], [16] * 7 + [1024])
    assert [r["status"] for r in recs] == want_status[:8]
    # bad arguments return before a launch
    seq, a, b = (ctypes.c_char_p * 1)(b"GGGAAAACCC"), (ctypes.c_char_p * 1)(b"(((....)))"), (ctypes.c_char_p * 1)(b"..........")
    ln, rec = (ctypes.c_int * 1)(10), (N.FindpathRec * 1)()
    w = lambda v: (ctypes.c_int * 1)(v)
    assert L.rafft_findpath_batch(-1, seq, ln, a, b, w(4), 37.0, 0, rec, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, None, ln, a, b, w(4), 37.0, 0, rec, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, seq, ln, None, b, w(4), 37.0, 0, rec, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, seq, ln, a, b, None, 37.0, 0, rec, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(4), 37.0, 0, None, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(0), 37.0, 0, rec, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(N.FINDPATH_MAX_WIDTH + 1), 37.0, 0, rec, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(4), 37.0, -1, rec, None, None) == N.ERR_PARAM
    assert L.rafft_findpath_batch(1, seq, ln, a, b, w(4), 25.0, 0, rec, None, None) == N.ERR_TEMP          # the built-in tables have no enthalpies
    L.rafft_alloc_counters(ctypes.byref(after))
    assert list(before) == list(after)
    # width 1024 x 1024 moves is exactly the candidate cap: accepted
    recs, moves, dcal = run([deep(n_stack)], 1024)
    assert recs[0]["status"] == 0 and recs[0]["dist"] == n_stack and N.FINDPATH_MAX_CANDIDATES == 1024 * n_stack
    evaluate_back([deep(n_stack)], recs, moves, dcal)


def test_another_temperature_with_a_loaded_parameter_file(sets):
    params.load_params(sets["paths"]["synthetic"])
    probs = FP.host_problems()[:20] + longer_problems()[:4]
    for temp in (25.0, 60.0):
        recs, moves, dcal = run(probs, 16, temp=temp)
        evaluate_back(probs, recs, moves, dcal, temp=temp)
    r37, _, _ = run(probs, 16)
    assert [r["start_dcal"] for r in r37] != [r["start_dcal"] for r in recs]


def test_both_directions_returns_the_lower_saddle_from_a_to_b():
    probs = FP.host_problems() + longer_problems()
    seqs, a, b = map(list, zip(*probs))
    fw = FPm.findpath_batch(seqs, a, b, width=2)
    bw = FPm.findpath_batch(seqs, b, a, width=2)
    both = FPm.findpath_batch(seqs, a, b, width=2, both=True)
    n_back = 0
    for k, prob in enumerate(probs):
        f, r, x = fw[0][k], bw[0][k], both[0][k]
        take_back = r["saddle_dcal"] < f["saddle_dcal"]
        n_back += take_back
        assert x["saddle_dcal"] == min(f["saddle_dcal"], r["saddle_dcal"])
        if take_back:
            assert both[2][k].tolist() == bw[2][k].tolist()[::-1]
            assert FPm.path_rows(a[k], both[1][k]) == FPm.path_rows(b[k], bw[1][k])[::-1]
        else:
            assert both[1][k].tolist() == fw[1][k].tolist() and both[2][k].tolist() == fw[2][k].tolist()
    assert n_back >= 1
    evaluate_back(probs, *both)
    with pytest.raises(ValueError):
        FPm.findpath_batch(["GGGAAAACCC"], ["(((....))"], [".........."])
    with pytest.raises(KeyError):
        FPm.findpath_batch(["GGGTAAACCC"], ["(((....)))"], [".........."])


def test_command_line_as_a_process(tmp_path):
    probs = FP.host_problems()[:2] + longer_problems()[:1]
    f = tmp_path / "paths.txt"
    f.write_text(f">first\n{probs[0][0]}\n{probs[0][1]}\n{probs[0][2]}\n" + f"{probs[1][0]}\n{probs[1][1]}\n{probs[1][2]}\n\n" +
                 f">third\n{probs[2][0]}\n{probs[2][1]}\n{probs[2][2]}\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-sf", str(f), "--findpath", "--width", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    recs, moves, dcal = run(probs, 7)
    want = []
    for k, (name, prob) in enumerate(zip((">first", None, ">third"), probs)):
        if name:
            want.append(name)
        want.append(prob[0])
        want += [f"{row} {e / 100.0:7.2f}" for row, e in zip(FPm.path_rows(prob[1], moves[k]), dcal[k].tolist())]
        want.append(f"saddle {recs[k]['saddle_dcal'] / 100.0:.2f} barrier {(recs[k]['saddle_dcal'] - recs[k]['start_dcal']) / 100.0:.2f} kcal/mol")
    assert r.stdout.splitlines() == want
    rb = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-sf", str(f), "--findpath", "--width", "1", "--both"], capture_output=True, text=True, timeout=120)
    assert rb.returncode == 0 and len(rb.stdout.splitlines()) == len(want)


def test_kinetics_with_barriers_on_the_example_graph(capsys):
    """rafft_kin.main is what bin/rafft_kin runs"""
    from rafft_amd.utils import parse_rafft_output
    example = os.path.join(ROOT, "tests", "golden", "example_rafft_20.out")
    fast_paths, seq = parse_rafft_output(example)
    capsys.readouterr()
    short = ["-mt", "8", "-ns", "4"]            # (a short schedule: the integration is not what is tested here)
    rafft_kin.main([example, "--gpu"] + short)
    plain = capsys.readouterr().out
    rafft_kin.main([example, "--gpu", "--barriers", "16"] + short)
    barr = capsys.readouterr().out
    # without --barriers the command prints what kinetics_gpu gives without the new arguments
    _, _, _, equi = rafft_kin.kinetics_gpu(fast_paths, 8, 4)
    equi.sort(key=lambda el: el[2])
    assert plain == "".join("{} {:6.3f} {:5.1f} {:d}\n".format(st, fp, nrj, si) for st, nrj, fp, si in equi)
    table = [ln.split() for ln in barr.splitlines()]
    assert len(table) == len(equi) and abs(sum(float(t[1]) for t in table) - 1.0) <= 5e-4 * len(table)
    with pytest.raises(SystemExit):
        rafft_kin.main([example, "--barriers", "16"])
    # every off-diagonal rate is at most the Metropolis one, strictly below it where the saddle exceeds both ends
    g = rafft_kin.barrier_graph(fast_paths, seq, width=16)
    rate, brate, en, sad = g["rate"], g["barrier_rate"], g["energy"], g["saddle"]
    n = len(en)
    n_higher = 0
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            assert brate[i][j] <= rate[i][j] and (brate[i][j] > 0.0) == (rate[i][j] > 0.0)
            if rate[i][j] > 0.0 and sad[i][j] > max(en[i], en[j]):
                n_higher += 1
                assert brate[i][j] < rate[i][j]
    print(f"\n{n} structures, {int((rate > 0).sum())} directed edges, the saddle is above both ends on {n_higher}")
    assert n_higher >= 2
    assert np.abs(brate.sum(axis=1)).max() <= 1e-12 * np.abs(brate).max()
