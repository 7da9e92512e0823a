"""Accuracy scoring on the GPU (rafft_score_rows / rafft_score_result) against the independent restatement
tests/_scoring_np.py (pair sets, integer counts, the `>=` pick) and the host definition rafft_amd.scoring."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _scoring_np
import rafft_amd
from conftest import ROOT
from rafft_amd import _native as N
from rafft_amd import scoring

pytestmark = pytest.mark.gpu

ROW_KEYS = ("row_seq", "n_pred", "hit_pred", "hit_known", "n_exact", "status")
SEQ_KEYS = ("seq_status", "n_known", "n_rows", "row0", "pick_ppv", "pick_first")


def same_tables(got, want, keys=ROW_KEYS + SEQ_KEYS + ("ppv", "sens", "bp_distance")):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (k, bad[:10], a[bad[:10]], b[bad[:10]])


def test_published_structures_in_one_call(bench_rows):
    """the 6888 (structure, known) pairs of the reference's three published tables: all integers equal the restatement, and
    PPV / sensitivity agree with the published columns to 0.006 in exactly the rows where the host scoring.score does"""
    keys = ("best", "ppv", "ppv200")
    beams = [[r[k][0] for k in keys] for r in bench_rows]
    known = [r["known"] for r in bench_rows]
    got = scoring.score_rows_gpu(beams, known)
    assert len(got["n_pred"]) == 3 * len(bench_rows) == 6888
    same_tables(got, _scoring_np.table(beams, known), ROW_KEYS + ("n_known", "n_rows", "row0", "seq_status", "bp_distance"))
    i, differ = 0, 0
    for r in bench_rows:
        for k in keys:
            a, b = r[k + "_scores"]
            p, s = scoring.score(r[k][0], r["known"])
            host_ok = abs(p - a) <= 0.006 and abs(s - b) <= 0.006
            gpu_ok = abs(got["ppv"][i] - a) <= 0.006 and abs(got["sens"][i] - b) <= 0.006
            assert host_ok == gpu_ok, (r["name"], k, (p, s), (got["ppv"][i], got["sens"][i]), (a, b))
            assert (got["ppv"][i], got["sens"][i]) == (p, s)
            differ += not gpu_ok
            i += 1
    assert differ <= 3, differ          # the bound of tests/test_host.py::test_scoring_reproduces_reference_columns


def test_whole_beams_of_the_benchmark_set(bench_rows):
    """fold the 2296 benchmark sequences at n=100, ms=50 and score every row of every final beam with rafft_score_result: all rows
    against the restatement, both picks of every sequence against scoring.best_of and row 0, no row left out; score_batch_gpu
    and score_rows_gpu (rows handed over as text) give the same arrays"""
    seqs = [r["seq"] for r in bench_rows]
    known = [r["known"] for r in bench_rows]
    res = rafft_amd.fold_batch(seqs, 100, 50, 1000)
    beams = [[x.str_struct for x in beam] for beam in res]
    total = sum(len(b) for b in beams)
    assert total > 100000
    # the C entry point itself
    row_out, seq_out = np.zeros(total, scoring._row_dtype()), np.zeros(len(seqs), scoring._seq_dtype())
    N.check(N.lib().rafft_score_result(res._owner.res, (C.c_char_p * len(known))(*[k.encode() for k in known]),
                                       row_out.ctypes.data_as(C.c_void_p), seq_out.ctypes.data_as(C.c_void_p)))
    assert not row_out["status"].any() and not seq_out["status"].any()
    assert seq_out["n_rows"].tolist() == [len(b) for b in beams]                       # no row is left out
    assert seq_out["row0"].tolist() == np.concatenate([[0], np.cumsum([len(b) for b in beams])[:-1]]).tolist()
    got = scoring.score_batch_gpu(res, known)
    for k in ("n_pred", "hit_pred", "hit_known", "n_exact", "status"):
        assert np.array_equal(got[k], row_out[k]), k
    for k in ("n_known", "n_rows", "row0", "pick_ppv", "pick_first"):
        assert np.array_equal(got[k], seq_out[k]), k
    for k, pick in (("best", "pick_ppv"), ("first", "pick_first")):                   # the picked rows' records
        assert np.array_equal(seq_out[k], row_out[seq_out["row0"] + seq_out[pick]]), k
    same_tables(got, _scoring_np.table(beams, known))                                 # every row, both picks
    same_tables(scoring.score_rows_gpu(beams, known), got)
    for s, (beam, kn) in enumerate(zip(res, known)):
        p, sn, db = scoring.best_of(beam, kn)
        at = got["row0"][s] + got["pick_ppv"][s]
        assert beams[s][got["pick_ppv"][s]] == db and (got["ppv"][at], got["sens"][at]) == (p, sn), s
        assert got["pick_first"][s] == 0


def random_structure(L, rng, p_open=0.3, p_close=0.3, brackets=("()",), base=None):
    """a seeded random well-nested structure; with `base`, only on its unpaired positions (so the new pairs cross the old ones)"""
    out = list(base) if base is not None else ["."] * L
    stack = []
    for x in range(L):
        if out[x] != ".":
            continue
        u = rng.random()
        if u < p_open:
            stack.append((x, brackets[rng.integers(len(brackets))]))
        elif u < p_open + p_close and stack:
            y, b = stack.pop()
            out[y], out[x] = b[0], b[1]
    return "".join(out)


def test_edges_against_the_restatement():
    rng = np.random.default_rng(20)
    beams, known = [], []
    add = lambda b, k: (beams.append(b), known.append(k))
    add(["." * 30], random_structure(30, rng))                                        # a beam of one unfolded row
    add([random_structure(40, rng) for _ in range(5)], "." * 40)                      # a known structure without pairs
    for L in (50, 200, 700):                                                          # [ ] and < > crossing the nested pairs
        kn = random_structure(L, rng, brackets=("()", "<>"))
        kn = random_structure(L, rng, 0.2, 0.2, brackets=("[]",), base=kn)
        assert "[" in kn and "<" in kn and "(" in kn
        add([random_structure(L, rng) for _ in range(7)] + [kn.replace("<", "(").replace(">", ")").replace("[", ".").replace("]", ".")], kn)
    # slips at both sequence ends: i - 1 = -1 and j + 1 = L
    L = 12
    ends = ["(..........)", ".(.........)", "(.........).", ".(........).", "............", "((........))", "(.(......).)", "(....)(....)"]
    for kn in ends:
        add(ends, kn)
    add(["()", "..", "()"], "()")
    for L in (1, 63, 64, 65, 127, 128, 129, 512, 513):
        add([random_structure(L, rng, 0.45, 0.45) for _ in range(9)] + ["." * L], random_structure(L, rng, 0.45, 0.45))
    deep = lambda L, k: "(" * k + "." * (L - 2 * k) + ")" * k                          # opens carried across many chunks
    add([deep(300, 150), deep(300, 149), deep(300, 1), "." + deep(298, 140) + "."], deep(300, 148))
    for L in (4608, 4609, 5000):                                                      # around the end of the LDS plans
        add([random_structure(L, rng) for _ in range(6)], random_structure(L, rng))
    add([random_structure(32767, rng), deep(32767, 16383)], random_structure(32767, rng))     # through the caches
    want = _scoring_np.table(beams, known)
    got = scoring.score_rows_gpu(beams, known)
    same_tables(got, want)
    assert got["n_pred"].max() > 5000 and got["hit_pred"].sum() > 0 and (got["hit_pred"] != got["n_exact"]).any()


def test_bad_rows_and_bad_known_structures_stay_local():
    rng = np.random.default_rng(21)
    good = [random_structure(70, rng) for _ in range(4)]
    kn = random_structure(70, rng)
    bad_rows = ["(" + "." * 69, "." * 69 + ")", ")" + "." * 68 + "(", "(" * 36 + ")" * 34, good[0][:30] + "x" + good[0][31:], "<" + "." * 68 + ">"]
    beam = [good[0], bad_rows[0], good[1], bad_rows[1], bad_rows[2], good[2], bad_rows[3], bad_rows[4], bad_rows[5], good[3]]
    ok_at = [0, 2, 5, 9]
    beams = [good, beam, good, good, good]
    known = [kn, kn, kn[:-1], "(" + kn[1:-1] + "(", kn]                               # wrong length; malformed
    got = scoring.score_rows_gpu(beams, known, lengths=[70] * 5)
    err = N.lib().rafft_last_error().decode()
    assert "sequence 2" in err and "69" in err
    want = _scoring_np.table([good, good, good], [kn, kn, kn])
    assert got["seq_status"].tolist() == [0, 0, N.ERR_STRUCT, N.ERR_STRUCT, 0]
    assert got["pick_ppv"][2] == got["pick_ppv"][3] == -1 and got["pick_first"][2] == -1
    st = got["status"].reshape(-1)
    assert st[:4].tolist() == [0] * 4 and st[14:22].tolist() == [N.ERR_STRUCT] * 8 and st[22:].tolist() == [0] * 4
    assert st[4:14].tolist() == [0 if k in ok_at else N.ERR_STRUCT for k in range(10)]
    for k in ("n_pred", "hit_pred", "hit_known", "n_exact"):
        assert got[k][:4].tolist() == want[k][:4].tolist() == got[k][22:].tolist()
        assert got[k][4:14][ok_at].tolist() == want[k][:4].tolist()                    # the good rows between the bad ones
        assert not got[k][4:14][[1, 3, 4, 6, 7, 8]].any()
    assert got["pick_ppv"][1] == ok_at[want["pick_ppv"][0]] and got["pick_ppv"][0] == want["pick_ppv"][0] == got["pick_ppv"][4]
    assert got["n_known"].tolist() == [want["n_known"][0]] * 2 + [0, 0] + [want["n_known"][0]]
    # the host definition takes < > in a predicted row; the GPU rows hold ( ) . only: documented, status says so
    p, s, db = scoring.best_of_gpu(good, kn)
    assert (p, s, db) == scoring.best_of(good, kn)


def test_row_strides(bench_rows):
    """rows back to back (stride L) and NUL-terminated as in rafft_seq_result.db (stride L + 1)"""
    rows = bench_rows[:60]
    lib = N.lib()
    n = len(rows)
    outs = []
    for pad in (0, 1, 5):
        bufs = [b"".join(r[k][0].encode() + b"\0" * pad for k in ("best", "ppv", "ppv200")) for r in rows]
        I = lambda v: (C.c_int * n)(*v)
        row_out, seq_out = np.zeros(3 * n, scoring._row_dtype()), np.zeros(n, scoring._seq_dtype())
        N.check(lib.rafft_score_rows(n, I([len(r["seq"]) for r in rows]), I([3] * n), (C.c_char_p * n)(*bufs), I([len(r["seq"]) + pad for r in rows]),
                                     (C.c_char_p * n)(*[r["known"].encode() for r in rows]), row_out.ctypes.data_as(C.c_void_p),
                                     seq_out.ctypes.data_as(C.c_void_p)))
        outs.append((row_out.tobytes(), seq_out.tobytes()))
    assert outs[0] == outs[1] == outs[2]
    want = _scoring_np.table([[r[k][0] for k in ("best", "ppv", "ppv200")] for r in rows], [r["known"] for r in rows])
    for k in ("n_pred", "hit_pred", "hit_known", "n_exact", "status"):
        assert row_out[k].tolist() == want[k].tolist(), k
    for k in ("n_known", "n_rows", "row0", "pick_ppv", "pick_first"):
        assert seq_out[k].tolist() == want[k].tolist(), k
    assert seq_out["status"].tolist() == want["seq_status"].tolist()


def test_scores_command_as_a_process(tmp_path, bench_rows):
    """bin/rafft -sf FILE --batch --scores on 40 benchmark sequences = fold_batch + restatement, line by line"""
    rows = [r for r in bench_rows if len(r["seq"]) <= 400][::37][:40]
    assert len(rows) == 40
    f = tmp_path / "benchmark_cleaned.csv"
    f.write_text("".join(f"{r['seq']},{r['known']},{r['name']}\n" for r in rows))
    res = rafft_amd.fold_batch([r["seq"] for r in rows], 100, 50, 1000)
    beams = [[(x.str_struct, x.dcal) for x in beam] for beam in res]
    records = [(r["seq"], r["known"], r["name"]) for r in rows]
    for select in ("ppv", "energy"):
        out = tmp_path / f"{select}.csv"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-sf", str(f), "--batch", "-n", "100", "-ms", "50", "--max_branch", "1000",
                            "--scores", str(out), "--select", select], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert out.read_text().splitlines() == _scoring_np.table_lines(records, beams, select), select
