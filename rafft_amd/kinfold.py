"""Stochastic folding trajectories on the GPU (rafft_kinfold_batch): what a user of the reference gets from
ViennaRNA's Kinfold - continuous-time Monte Carlo over insertion and deletion of single pairs with Metropolis rates, from the open
chain or any structure, with first-passage times to stop structures and the state at given times.  The unreduced dynamics that
rafft_kin's master equation on a fast-folding graph, a basin_graph or a BarrierTree coarse-grains."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .descend import _row_block, end_rows
from .mccaskill import _seeds_of
from .rafft import raise_for_status

TRAJ_DTYPE = np.dtype([("status", "<i4"), ("flags", "<i4"), ("n_steps", "<i4"), ("start_dcal", "<i4"), ("end_dcal", "<i4"),
                       ("stop_index", "<i4"), ("time", "<f8")])
INVALID_SAMPLE = (-2 ** 31, -2)     # what a sample record holds that a trajectory did not reach (KF_MORE) or that had an error


def kinfold_weights(temp=37.0, kt=0.0):
    """the uint64 weight table of a call at (temp, kt): W[0] = 2^32, W[d] = floor(2^32 exp(-d / (100 kT)) + 0.5); needs no device"""
    out = np.zeros(N.KINFOLD_NW, dtype=np.uint64)
    if N.lib().rafft_kinfold_weights(float(temp), float(kt), out.ctypes.data):
        raise ValueError("kt is negative or not finite, or kT is not above 0")
    return out


def _rows_of(rows, length):
    """the start rows of one sequence with None as the open chain (rows itself None: one open chain)"""
    if rows is None:
        rows = [None]
    if isinstance(rows, np.ndarray):
        return rows
    return ["." * length if r is None else r for r in rows]


def kinfold_batch_raw(sequences, rows, t_max, n_rep=1, watch=None, n_stop=None, seeds=None, sample_times=(), temp=37.0, kt=0.0, max_steps=0,
                      workspace_bytes=0, log=False):
    """(seq_records, traj_records, ends, samples, moves, times) of rafft_kinfold_batch.  rows[s]: the start rows of sequence s as
    descend_batch_raw takes them, None for the open chain; watch[s]: its watched rows (None: none anywhere), the first n_stop[s] of
    them absorbing (an int: the same for every sequence; None: 0).  seq_records: one dict per sequence (status, length, n_traj,
    traj0); traj_records: per sequence an array of TRAJ_DTYPE, trajectory k = r * n_rep + rep; ends: per sequence an (n_traj, L + 1)
    uint8 array; samples: per sequence an (n_traj, n_times, 2) int32 array of (dcal, watch index); moves, times: per sequence lists
    of (n_steps, 2) int32 and (n_steps,) float64 arrays, or None without log=True - which allocates max_steps (or
    KINFOLD_DEFAULT_STEPS) entries per trajectory, so give max_steps with it.  Nothing is raised for an item's own error."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    if len(rows) != n or (watch is not None and len(watch) != n):
        raise ValueError("one list of rows per sequence")
    enc, arr, lens = N.seq_arrays(sequences)
    blocks, strides = [], []
    for s in range(n):
        a, stride = _row_block(_rows_of(rows[s], len(enc[s])), len(enc[s]))
        blocks.append(a)
        strides.append(stride)
    n_rep = int(n_rep)
    n_traj = [b.shape[0] * max(n_rep, 0) for b in blocks]
    grid = np.ascontiguousarray(sample_times, dtype=np.float64)
    n_times = grid.size
    ptr = lambda a: a.ctypes.data if a.size else None
    ints = lambda v: (C.c_int * n)(*v)
    voids = lambda v: (C.c_void_p * n)(*[ptr(a) for a in v])
    if watch is None:
        wargs = (None, None, None, None)
        wblocks = []
    else:
        wb = [_row_block(w if w is not None else [], len(enc[s])) for s, w in enumerate(watch)]
        wblocks = [a for a, _ in wb]
        stops = [0] * n if n_stop is None else [int(n_stop)] * n if isinstance(n_stop, (int, np.integer)) else [int(x) for x in n_stop]
        wargs = (ints([a.shape[0] for a in wblocks]), ints(stops), voids(wblocks), ints([st for _, st in wb]))
    seeds = _seeds_of(seeds, n)
    bound = int(max_steps) if max_steps > 0 else N.KINFOLD_DEFAULT_STEPS
    ends = [np.zeros((n_traj[s], len(enc[s]) + 1), dtype=np.uint8) for s in range(n)]
    samples = [np.zeros((n_traj[s], n_times, 2), dtype=np.int32) for s in range(n)]
    mv = [np.zeros((n_traj[s], bound, 2), dtype=np.int32) for s in range(n)] if log else None
    tm = [np.zeros((n_traj[s], bound), dtype=np.float64) for s in range(n)] if log else None
    srec = (N.KinfoldSeq * n)()
    total = sum(n_traj)
    trec = np.zeros(total, dtype=TRAJ_DTYPE)
    N.check(L.rafft_kinfold_batch(n, arr, lens, ints([b.shape[0] for b in blocks]), voids(blocks), ints(strides), n_rep, *wargs,
                                  (C.c_ulonglong * n)(*seeds) if seeds is not None else None, float(temp), float(kt), float(t_max), int(max_steps),
                                  n_times, grid.ctypes.data_as(C.POINTER(C.c_double)) if n_times else None, int(workspace_bytes), srec,
                                  trec.ctypes.data if total else None, voids(ends), voids(samples) if n_times else None,
                                  voids(mv) if log else None, voids(tm) if log else None))
    seq_recs = [dict(status=r.status, length=r.length, n_traj=r.n_traj, traj0=r.traj0) for r in srec]
    traj_recs, out_mv, out_tm = [], [] if log else None, [] if log else None
    for s, q in enumerate(seq_recs):
        part = trec[q["traj0"]:q["traj0"] + q["n_traj"]].copy()
        traj_recs.append(part)
        if log:
            out_mv.append([mv[s][k, :part["n_steps"][k]].copy() for k in range(q["n_traj"])])
            out_tm.append([tm[s][k, :part["n_steps"][k]].copy() for k in range(q["n_traj"])])
    return seq_recs, traj_recs, ends, samples, out_mv, out_tm


def kinfold_batch(seqs, rows, t_max, n_rep=1, watch=None, n_stop=None, seeds=None, sample_times=(), temp=37.0, kt=0.0, max_steps=0,
                  log=False, raise_errors=True):
    """Per sequence a dict(rows, dcal, start_dcal, n_steps, flags, stop_index, time, status, samples[, moves, times]) over its
    n_rows * n_rep trajectories (k = r * n_rep + rep): the row each ended in, its energy, why it ended (flags: N.KF_TIME, KF_STOP,
    KF_ABSORBED, KF_MORE) and when.  A sequence with an error raises what fold_batch raises for it, a malformed row or watched row
    a ValueError, a trajectory that max_steps ended a RafftError (raise_errors=False: the statuses say it, the entry of a sequence
    with an error is None)."""
    srec, trec, ends, samples, mv, tm = kinfold_batch_raw(seqs, rows, t_max, n_rep, watch, n_stop, seeds, sample_times, temp, kt, max_steps, 0, log)
    out = []
    for s, q in enumerate(srec):
        if q["status"] != N.OK:
            if raise_errors:
                if q["status"] == N.ERR_STRUCT:
                    raise ValueError(f"sequence {s}: a watched row is malformed, has a non-canonical pair, or a hairpin of fewer than 3")
                raise_for_status(q["status"], seqs[s], s, "kinfold_batch", "RAFFT_KINFOLD_MAX_LEN")
            out.append(None)
            continue
        t = trec[s]
        st = t["status"]
        if raise_errors and st.any():
            k = int(np.flatnonzero(st)[0])
            if st[k] == N.ERR_STRUCT:
                raise ValueError(f"sequence {s} row {k // n_rep}: malformed, a non-canonical pair, or a hairpin of fewer than 3")
            raise N.RafftError(int(st[k]), f"sequence {s} trajectory {k}: not ended after {int(t['n_steps'][k])} steps (max_steps)")
        d = dict(rows=end_rows(ends[s], q["length"]), dcal=t["end_dcal"], start_dcal=t["start_dcal"], n_steps=t["n_steps"], flags=t["flags"],
                 stop_index=t["stop_index"], time=t["time"], status=st, samples=samples[s])
        if log:
            d["moves"], d["times"] = mv[s], tm[s]
        out.append(d)
    return out


def passage_times(flags, time):
    """(times, missing) of the trajectories of one sequence: the arrival times of those that reached a stop row, in their order, and
    the share of all that did not"""
    flags, time = np.asarray(flags, dtype=np.int64), np.asarray(time, dtype=np.float64)
    hit = (flags & N.KF_STOP) != 0
    return time[hit].copy(), (1.0 - hit.sum() / len(flags)) if len(flags) else 0.0


def first_passage(seq, start, stop, n, t_max, seed=0, temp=37.0, kt=0.0, max_steps=0):
    """(times, missing): n trajectories of `seq` from `start` (None: the open chain) with the row `stop` (or a list of rows)
    absorbing: the first-passage times of those that arrived by t_max and the share that did not"""
    stops = [stop] if isinstance(stop, str) else list(stop)
    d = kinfold_batch([seq], [[start]], t_max, n_rep=n, watch=[stops], n_stop=len(stops), seeds=seed, temp=temp, kt=kt, max_steps=max_steps)[0]
    return passage_times(d["flags"], d["time"])


def occupancy_counts(samples, n_watch):
    """the (n_times, n_watch + 1) matrix of one sequence's sample records ((n_traj, n_times, 2) int32): how many trajectories are in
    watched row w at each time, the last column those in none; records that were not reached (watch index -2) are not counted"""
    samples = np.asarray(samples)
    n_times = samples.shape[1]
    out = np.zeros((n_times, n_watch + 1), dtype=np.int64)
    for t in range(n_times):
        w = samples[:, t, 1]
        w = w[w >= -1]
        out[t] = np.bincount(np.where(w < 0, n_watch, w), minlength=n_watch + 1)
    return out


def occupancy(seqs, starts, watch, n, sample_times, t_max=None, n_stop=0, seeds=0, temp=37.0, kt=0.0, max_steps=0):
    """Per sequence the (n_times, n_watch + 1) count matrix of n trajectories from starts[s] (None: the open chain): column w
    counts those in watch[s][w] at sample_times[t], the last column those elsewhere - divided by n, the columns line up with the
    populations rafft_kin.solve_master_equation returns for the same states in the same order.  t_max: the last sample time."""
    grid = np.asarray(sample_times, dtype=np.float64)
    t_max = float(grid[-1]) if t_max is None else t_max
    res = kinfold_batch(seqs, [[st] for st in starts], t_max, n_rep=n, watch=watch, n_stop=n_stop, seeds=seeds, sample_times=grid, temp=temp,
                        kt=kt, max_steps=max_steps)
    return [occupancy_counts(d["samples"], len(watch[s])) for s, d in enumerate(res)]
