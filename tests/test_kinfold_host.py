"""rafft_kinfold_batch before any kernel runs: the weight table against its formula; the tests' restatement
of the process (`_kinfold_np.Mirror`: whole-structure oracle energies, brute-force neighbours, its own Philox) against the exact
master equation on full enumerations - occupancies and survival, judged by `_sample_stats.misses` -, which validates restatement
and definition alike; the host-pure part of the library in a stand-alone C++ program, plain and under AddressSanitizer + UBSan;
the records and limits against the header; bad arguments and all-erroneous batches without a device; the bookkeeping of
first_passage and occupancy on constructed records.  No GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from rafft_amd import _native, params
from rafft_amd import kinfold as KFm
from conftest import ROOT
import _descend_np as DS
import _kinfold_np as KF
import _sample_stats as SS

KT37 = KF.GAS * 310.15


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def test_philox_restatement_equals_the_librarys(tmp_path):
    assert KF.philox((0, 0), (0, 0, 0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)      # Random123's known answer
    exe = str(tmp_path / "rng_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "hostcheck", "rng_check.cpp"), "-o", exe])
    cases = [(77, k, t) for k in range(6) for t in range(6)] + [((1 << 64) - 1, KF.MASK, KF.MASK), (1 << 32, 3, 1 << 20)]
    r = subprocess.run([exe], input="".join(f"{key} {k} {t}\n" for key, k, t in cases), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    for (key, k, t), line in zip(cases, r.stdout.split("\n")):
        assert tuple(int(x, 16) for x in line.split()[:4]) == KF.philox((key & KF.MASK, key >> 32), (k, t, 0, 0))


@pytest.mark.parametrize("temp,kt", [(37.0, 0.0), (37.0, 2.5), (60.0, 0.0)])
def test_weight_table_against_the_formula(temp, kt):
    W = KFm.kinfold_weights(temp, kt)
    kT = kt if kt else KF.GAS * (temp + 273.15)
    want = KF.formula_weights(kT)
    assert W.dtype == np.uint64 and len(W) == KF.NW == _native.KINFOLD_NW
    assert int(W[0]) == 1 << 32
    assert max(abs(int(a) - b) for a, b in zip(W, want)) <= 1
    assert all(int(a) >= int(b) for a, b in zip(W, W[1:]))
    zeros = np.flatnonzero(W == 0)
    first = math.floor(100.0 * kT * 33.0 * math.log(2.0)) + 1       # 2^32 exp(-d / (100 kT)) < 1/2
    assert (zeros[0] == first and (W[first:] == 0).all()) if first < KF.NW else len(zeros) == 0
    assert (first < KF.NW) == (kt == 0.0)                           # (both kinds of table are among the cases)


def test_weight_table_refuses_what_it_cannot_hold():
    out = (ctypes.c_uint64 * KF.NW)()
    f = _native.lib().rafft_kinfold_weights
    assert f(37.0, 0.0, out) == 0 and out[0] == 1 << 32
    for temp, kt in ((37.0, -1.0), (37.0, float("nan")), (37.0, float("inf")), (-273.15, 0.0), (float("nan"), 0.0)):
        assert f(temp, kt, out) == _native.ERR_PARAM
    assert f(37.0, 0.0, None) == _native.ERR_PARAM
    with pytest.raises(ValueError):
        KFm.kinfold_weights(37.0, -0.5)


# ---- the restatement against the exact master equation

GRID = [3.7, 17.3, 61.9, 171.3, 433.7]
N_MIRROR = 1000


def short_sequences():
    return [(seq, rows) for seq, rows in DS.start_sequences() if len(rows) <= 300][:2]


def test_the_restatement_follows_the_master_equation_on_full_enumerations():
    W = KFm.kinfold_weights()
    M = KF.Mirror(W)
    cases = short_sequences()
    assert len(cases) == 2
    for s, (seq, rows) in enumerate(cases):
        Q, en = KF.generator(seq, rows, W)
        open_chain = "." * len(seq)
        p0 = np.zeros(len(rows))
        p0[rows.index(open_chain)] = 1.0
        # occupancy of every state of the enumeration at five times
        P = KF.propagate(Q, p0, GRID)
        assert np.abs(P.sum(axis=1) - 1.0).max() < 1e-9 and P.min() > -1e-12
        P = np.clip(P, 0.0, 1.0)
        index = {r: k for k, r in enumerate(rows)}
        counts = np.zeros((len(GRID), len(rows)))
        steps = 0
        for k in range(N_MIRROR):
            t = M.trajectory(seq, open_chain, k, 1000 + s, GRID[-1], grid=GRID)
            assert t["near"] == 0 and t["flags"] == KF.KF_TIME and t["time"] == GRID[-1] and len(t["samples"]) == len(GRID)
            assert t["end"] in index and t["dcal"][-1] == en[index[t["end"]]] == t["end_dcal"]
            steps += t["n_steps"]
            # the state at a time is the row after the last jump at or before it
            for ti, tau in enumerate(GRID):
                n = sum(1 for T in t["times"] if T <= tau)
                assert t["samples"][ti][0] == t["dcal"][n]
            at, ti = [], 0
            pairs = set()
            for (i, j), T in zip(t["moves"], t["times"]):
                while ti < len(GRID) and GRID[ti] < T:
                    at.append(_row_of(pairs, len(seq)))
                    ti += 1
                pairs ^= {(i, j) if i >= 0 else (-i - 1, -j - 1)}
            while ti < len(GRID):
                at.append(_row_of(pairs, len(seq)))
                ti += 1
            assert _row_of(pairs, len(seq)) == t["end"]
            for ti, r in enumerate(at):
                counts[ti, index[r]] += 1
        print(f"\n{seq}: {len(rows)} structures, {steps / N_MIRROR:.1f} steps a trajectory")
        assert steps > 10 * N_MIRROR
        bad = SS.misses(counts, N_MIRROR, P)
        assert len(bad) == 0, (seq, bad, counts.ravel()[bad], (N_MIRROR * P).ravel()[bad])
        # survival: the MFE row absorbing
        mfe = int(np.argmin(en))
        Qa = Q.copy()
        Qa[:, mfe] = 0.0
        arrived = np.clip(KF.propagate(Qa, p0, GRID)[:, mfe], 0.0, 1.0)
        got = np.zeros(len(GRID))
        for k in range(N_MIRROR):
            t = M.trajectory(seq, open_chain, k, 2000 + s, GRID[-1], watch=[rows[mfe]], n_stop=1, grid=GRID)
            if t["flags"] & KF.KF_STOP:
                assert t["end"] == rows[mfe] and t["stop_index"] == 0 and t["time"] == t["times"][-1] <= GRID[-1]
                got += np.array(GRID) >= t["time"]
                # after its arrival the trajectory holds the stop row
                assert all(smp == (en[mfe], 0) for smp, tau in zip(t["samples"], GRID) if tau >= t["time"])
            else:
                assert t["flags"] == KF.KF_TIME and t["stop_index"] == -1 and all(w == -1 for _, w in t["samples"])
        assert 0 < got[-1] < N_MIRROR or arrived[-1] in (0.0, 1.0)
        assert len(SS.misses(got, N_MIRROR, arrived)) == 0, (seq, got, N_MIRROR * arrived)


def _row_of(pairs, L):
    row = ["."] * L
    for i, j in pairs:
        row[i], row[j] = "(", ")"
    return "".join(row)


def test_the_step_bound_and_the_ends_of_the_restatement():
    M = KF.Mirror(KFm.kinfold_weights())
    seq = short_sequences()[0][0]
    grid = [0.0, 2.1, 1e6]
    full = M.trajectory(seq, "." * len(seq), 3, 9, 1e6, max_steps=40, grid=grid)
    assert full["flags"] == KF.KF_MORE and full["status"] == KF.ERR_CAPACITY and full["n_steps"] == 40 and full["time"] == full["times"][-1]
    assert full["samples"][0] == (0, -1) and full["samples"][-1] == KF.INVALID
    cut = M.trajectory(seq, "." * len(seq), 3, 9, 1e6, max_steps=3, grid=grid)
    assert cut["moves"] == full["moves"][:3] and cut["times"] == full["times"][:3] and cut["n_steps"] == 3
    timed = M.trajectory(seq, "." * len(seq), 3, 9, full["times"][5], max_steps=40)       # t_max at a jump: the jump is taken
    assert timed["flags"] == KF.KF_TIME and timed["n_steps"] == 6 and timed["time"] == full["times"][5]
    zero = M.trajectory(seq, "." * len(seq), 3, 9, 0.0, grid=[0.0])
    assert zero["flags"] == KF.KF_TIME and zero["n_steps"] == 0 and zero["time"] == 0.0 and zero["samples"] == [(0, -1)]
    here = M.trajectory(seq, "." * len(seq), 3, 9, 5.0, watch=["." * len(seq)], n_stop=1, grid=[1.0])
    assert here["flags"] == KF.KF_STOP and here["n_steps"] == 0 and here["time"] == 0.0 and here["stop_index"] == 0 and here["samples"] == [(0, 0)]
    stuck = M.trajectory("AAAAAAAA", "........", 0, 0, 7.5, grid=[1.0])
    assert stuck["flags"] == KF.KF_ABSORBED and stuck["n_steps"] == 0 and stuck["time"] == 7.5 and stuck["samples"] == [(0, -1)]


# ---- the host-pure part, the header, the arguments

def test_host_pure_part_against_the_tests_values_under_sanitizers(tmp_path):
    argv = []
    for temp, kt in ((37.0, 0.0), (37.0, 0.8), (25.0, 0.0)):
        want = KF.formula_weights(kt if kt else KF.GAS * (temp + 273.15))
        for d in (0, 1, 2, 99, 100, 500, 1409, 1410, 1411, 4095):
            argv += [repr(temp), repr(kt), str(d), str(want[d])]
    src = os.path.join(ROOT, "tests", "hostcheck", "kinfold_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("kinfold_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"{len(argv) // 4} cases, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr
    # the program does tell a wrong entry from a right one
    r = subprocess.run([exe, "37.0", "0.0", "1", "4225842395"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "1 failures" in r.stdout


def test_kinfold_records_and_limits_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    for name, cls, size in (("rafft_kinfold_seq", _native.KinfoldSeq, 16), ("rafft_kinfold_traj", _native.KinfoldTraj, 32)):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", hdr).group(1), flags=re.S)
        names = [n.strip() for n in re.findall(r"\b(?:int32_t|double)\s+(\w+);", body)]
        assert names == [n for n, _ in cls._fields_] and ctypes.sizeof(cls) == size
    assert [n for n, _ in _native.KinfoldTraj._fields_] == list(KFm.TRAJ_DTYPE.names) and KFm.TRAJ_DTYPE.itemsize == 32
    assert [KFm.TRAJ_DTYPE.fields[n][1] for n in KFm.TRAJ_DTYPE.names] == [getattr(_native.KinfoldTraj, n).offset for n in KFm.TRAJ_DTYPE.names]
    assert re.search(r"#define RAFFT_KINFOLD_MAX_LEN\s+RAFFT_DESCEND_MAX_LEN", hdr) and _native.KINFOLD_MAX_LEN == 4096
    for name, val in (("NW", _native.KINFOLD_NW), ("MAX_WATCH", _native.KINFOLD_MAX_WATCH), ("TIME", _native.KF_TIME), ("STOP", _native.KF_STOP),
                      ("ABSORBED", _native.KF_ABSORBED), ("MORE", _native.KF_MORE)):
        assert int(re.search(r"#define RAFFT_KINFOLD_" + name + r"\s+(\d+)", hdr).group(1)) == val
    assert re.search(r"#define RAFFT_KINFOLD_DEFAULT_STEPS\s+\(1 << 20\)", hdr) and _native.KINFOLD_DEFAULT_STEPS == 1 << 20 == KF.DEFAULT_STEPS
    assert (KF.KF_TIME, KF.KF_STOP, KF.KF_ABSORBED, KF.KF_MORE) == (_native.KF_TIME, _native.KF_STOP, _native.KF_ABSORBED, _native.KF_MORE)
    assert {"rafft_kinfold_batch", "rafft_kinfold_weights", "rafft_kinfold_counters"} <= set(_native.EXPORTS)
    proto = re.search(r"int rafft_kinfold_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_kinfold_batch.argtypes) == 25


def test_bad_arguments_and_erroneous_batches_need_no_device():
    L = _native.lib()
    E = _native.ERR_PARAM
    seq = (ctypes.c_char_p * 1)(b"GGGAAAACCC")
    rowbuf = ctypes.create_string_buffer(b"(((....)))")
    rows = (ctypes.c_void_p * 1)(ctypes.addressof(rowbuf))
    wbuf = ctypes.create_string_buffer(b"(((....)))" * 65)
    watch = (ctypes.c_void_p * 1)(ctypes.addressof(wbuf))
    out = ctypes.create_string_buffer(11)
    db = (ctypes.c_void_p * 1)(ctypes.addressof(out))
    sbuf = (ctypes.c_int32 * 8)()
    smp = (ctypes.c_void_p * 1)(ctypes.addressof(sbuf))
    i1 = lambda v: (ctypes.c_int * 1)(v)
    grid = lambda *v: (ctypes.c_double * len(v))(*v)
    srec, trec = (_native.KinfoldSeq * 1)(), (_native.KinfoldTraj * 1)()
    good = dict(n_seq=1, seqs=seq, lens=i1(10), n_rows=i1(1), rows=rows, stride=i1(10), n_rep=1, n_watch=i1(1), n_stop=i1(1), watch=watch,
                wstride=i1(10), seeds=None, temp=37.0, kt=0.0, t_max=5.0, max_steps=0, n_times=2, times=grid(1.0, 5.0), ws=0, srec=srec,
                trec=ctypes.addressof(trec), db=db, smp=smp, moves=None, jt=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.rafft_kinfold_batch(*[a[k] for k in good])
    for k in ("seqs", "lens", "n_rows", "rows", "stride", "srec", "trec", "db", "smp", "times", "n_stop", "watch", "wstride"):
        assert call(**{k: None}) == E, k
    none1 = (ctypes.c_void_p * 1)(None)
    for kw in (dict(n_seq=-1), dict(n_rows=i1(-1)), dict(stride=i1(9)), dict(wstride=i1(9)), dict(rows=none1), dict(db=none1), dict(smp=none1),
               dict(watch=none1), dict(n_rep=0), dict(n_rep=-3), dict(n_watch=i1(65)), dict(n_watch=i1(-1)), dict(n_stop=i1(2)), dict(n_stop=i1(-1)),
               dict(t_max=-1.0), dict(t_max=float("inf")), dict(t_max=float("nan")), dict(times=grid(2.0, 1.0)), dict(times=grid(1.0, 5.5)),
               dict(times=grid(-1.0, 5.0)), dict(times=grid(1.0, float("nan"))), dict(kt=-0.1), dict(kt=float("nan")), dict(kt=float("inf")),
               dict(max_steps=-1), dict(ws=-1), dict(n_times=-1), dict(moves=none1), dict(jt=none1),
               dict(moves=(ctypes.c_void_p * 1)(ctypes.addressof(sbuf)), jt=none1), dict(n_rep=1 << 30, n_rows=i1(4))):
        assert call(**kw) == E, kw
    assert call(temp=25.0) == _native.ERR_TEMP          # the built-in tables have no enthalpies
    assert call(n_seq=0) == 0 and L.rafft_kinfold_batch(*([0] + [None] * 5 + [1] + [None] * 5 + [37.0, 0.0, 1.0, 0, 0, None, 0] + [None] * 6)) == 0
    # a sequence without rows needs neither rows nor outputs; n_watch may be NULL
    assert call(n_rows=i1(0), rows=none1, db=none1, smp=none1, trec=None, n_watch=None, n_stop=None, watch=None, wstride=None) == 0
    assert (srec[0].status, srec[0].length, srec[0].n_traj, srec[0].traj0) == (0, 10, 0, 0)
    # a batch of nothing but erroneous items never reaches the device
    seqs = ["", "GGGTAAAACCC", "A" * 4097, "GGGAAAACCC", "GGGAAAACCA", "GGGAAAACCC"]
    rows = [[None], ["(((.....)))", None], [None], ["(((....))", "(((..)..))"], ["(((....)))"], [None, "(((....)))"]]
    watch = [[], [], [], [], [], ["(((....)))", "(((..)..))"]]
    srec, trec, ends, samples, mv, tm = KFm.kinfold_batch_raw(seqs, rows, 5.0, n_rep=2, watch=watch, n_stop=[0, 0, 0, 0, 0, 1], sample_times=[1.0, 2.0],
                                                              max_steps=4, log=True)
    S = _native.ERR_STRUCT
    assert [q["status"] for q in srec] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG, 0, 0, S]
    assert [(q["length"], q["n_traj"], q["traj0"]) for q in srec] == [(0, 2, 0), (11, 4, 2), (4097, 2, 6), (10, 4, 8), (10, 2, 12), (10, 4, 14)]
    assert [t["status"].tolist() for t in trec] == [[_native.ERR_EMPTY] * 2, [_native.ERR_BAD_CHAR] * 4, [_native.ERR_TOO_LONG] * 2, [S] * 4, [S] * 2, [S] * 4]
    for t in trec:
        assert not t["n_steps"].any() and not t["flags"].any() and not t["start_dcal"].any() and (t["stop_index"] == -1).all() and not t["time"].any()
    assert all((x == KFm.INVALID_SAMPLE).all() for x in samples) and samples[3].shape == (4, 2, 2)
    # a sequence's error: rows of dots; a row's error: the row as it went in, once per replicate
    assert KFm.end_rows(ends[1], 11) == ["." * 11] * 4 and KFm.end_rows(ends[5], 10) == ["." * 10] * 4 and ends[0].tolist() == [[0], [0]]
    assert ends[3].tobytes() == b"(((....))\0\0" * 2 + b"(((..)..))\0" * 2 and ends[4].tobytes() == b"(((....)))\0" * 2
    assert all(len(m) == 0 for per in mv for m in per) and all(len(m) == 0 for per in tm for m in per)
    assert L.rafft_last_error().decode().startswith("sequence 0: empty")
    KFm.kinfold_batch_raw(seqs[3:], rows[3:], 5.0, watch=watch[3:], n_stop=[0, 0, 1])
    assert L.rafft_last_error().decode().startswith("sequence 0 row 0: malformed")
    KFm.kinfold_batch_raw(seqs[5:], rows[5:], 5.0, watch=watch[5:], n_stop=1)
    assert L.rafft_last_error().decode().startswith("sequence 0 watched row 1: malformed")
    cnt = (ctypes.c_longlong * 4)()
    assert L.rafft_kinfold_counters(ctypes.byref(cnt)) == 0 and list(cnt) == [0, 0, 0, 0]
    assert L.rafft_kinfold_counters(None) == E
    with pytest.raises(ValueError, match="sequence 0 row 0"):
        KFm.kinfold_batch(seqs[3:4], rows[3:4], 5.0)
    with pytest.raises(ValueError, match="watched row"):
        KFm.kinfold_batch(seqs[5:], rows[5:], 5.0, watch=watch[5:])
    with pytest.raises(KeyError):
        KFm.kinfold_batch(seqs[1:2], rows[1:2], 5.0)
    with pytest.raises(ValueError, match="4096 nt"):
        KFm.kinfold_batch(seqs[2:3], rows[2:3], 5.0)
    assert KFm.kinfold_batch(seqs[1:2], rows[1:2], 5.0, raise_errors=False) == [None]


def test_first_passage_and_occupancy_bookkeeping_on_constructed_records():
    flags = np.array([_native.KF_STOP, _native.KF_TIME, _native.KF_STOP, _native.KF_ABSORBED, _native.KF_MORE, _native.KF_STOP])
    time = np.array([2.5, 9.0, 0.0, 9.0, 4.0, 8.75])
    times, missing = KFm.passage_times(flags, time)
    assert times.tolist() == [2.5, 0.0, 8.75] and missing == 0.5
    assert KFm.passage_times([], [])[0].size == 0 and KFm.passage_times([], [])[1] == 0.0
    assert KFm.passage_times([_native.KF_TIME] * 3, [1.0] * 3)[1] == 1.0
    # four trajectories, three times, two watched rows: the last column counts the states that are neither
    smp = np.array([[[0, -1], [-100, 0], [-300, 1]],
                    [[0, -1], [-50, -1], [-300, 1]],
                    [[-100, 0], [-100, 0], [-100, 0]],
                    [[0, -1], [-2 ** 31, -2], [-2 ** 31, -2]]], dtype=np.int32)
    assert KFm.occupancy_counts(smp, 2).tolist() == [[1, 0, 3], [2, 0, 1], [1, 2, 0]]       # (what was not reached is not counted)
    assert KFm.occupancy_counts(smp[:, :0], 2).shape == (0, 3)
    assert KFm.occupancy_counts(smp[:3], 64).shape == (3, 65) and KFm.occupancy_counts(smp[:3], 64)[:, 64].tolist() == [2, 1, 0]
    assert KFm._rows_of(None, 4) == ["...."] and KFm._rows_of([None, "(..)"[:4]], 4) == ["....", "(..)"]
