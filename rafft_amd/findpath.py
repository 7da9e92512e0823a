"""Folding barriers between pairs of structures on the GPU (rafft_findpath_batch): what a user of the
reference gets from ViennaRNA's findpath (RNA.fold_compound(seq).path_findpath(A, B, width); Flamm et al. 2001) - a direct path from
A to B whose highest point is low, for a whole batch of (sequence, A, B) problems in one call."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .rafft import raise_for_status


def findpath_batch_raw(sequences, starts, ends, widths, temp=37.0, workspace_bytes=0, paths=True):
    """(records, moves, dcal) of rafft_findpath_batch: one dict per problem with the numbers of rafft_findpath_rec; per problem an
    (length, 2) int32 array of moves - (i, j) for an added pair, (-i-1, -j-1) for a removed one - and an int32 array of its length + 1
    energies in dcal/mol (both empty for a problem with an error; None with paths=False, which passes NULL for both).  Nothing is
    raised for a problem's own error.  widths: one int, or one per problem."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    if not (len(starts) == len(ends) == n):
        raise ValueError("one start row and one end row per sequence")
    widths = [int(widths)] * n if np.isscalar(widths) else [int(w) for w in widths]
    if len(widths) != n:
        raise ValueError("one width per problem")
    enc, arr, lens = N.seq_arrays(sequences)
    rows = lambda v: (C.c_char_p * n)(*[r.encode("ascii", "replace") for r in v])
    a, b = rows(starts), rows(ends)
    rec = (N.FindpathRec * n)()
    mv = [np.zeros((len(e), 2), dtype=np.int32) for e in enc] if paths else None
    en = [np.zeros(len(e) + 1, dtype=np.int32) for e in enc] if paths else None
    mp = (C.c_void_p * n)(*[x.ctypes.data for x in mv]) if paths else None
    ep = (C.c_void_p * n)(*[x.ctypes.data for x in en]) if paths else None
    N.check(L.rafft_findpath_batch(n, arr, lens, a, b, (C.c_int * n)(*widths), float(temp), int(workspace_bytes), rec, mp, ep))
    recs = [dict(status=r.status, length=r.length, dist=r.dist, start_dcal=r.start_dcal, end_dcal=r.end_dcal, saddle_dcal=r.saddle_dcal,
                 saddle_step=r.saddle_step) for r in rec]
    if not paths:
        return recs, None, None
    moves = [mv[k][:r["length"]].copy() for k, r in enumerate(recs)]
    dcal = [en[k][:r["length"] + 1].copy() if r["status"] == N.OK else np.zeros(0, dtype=np.int32) for k, r in enumerate(recs)]
    return recs, moves, dcal


def reverse_path(moves, dcal):
    """the same structures walked the other way: moves in reverse order, added and removed exchanged, energies reversed"""
    return (-np.asarray(moves, dtype=np.int32)[::-1] - 1).copy(), np.asarray(dcal, dtype=np.int32)[::-1].copy()


def findpath_batch(seqs, starts, ends, width=16, both=False, temp=37.0, workspace_bytes=0, raise_errors=True):
    """(records, moves, dcal) per problem p of a path from starts[p] to ends[p] whose saddle is low.  both=True also searches from
    ends[p] to starts[p] in the same call and returns the path with the lower saddle (the forward one on a tie), walked from
    starts[p] to ends[p].  A problem with an error raises (raise_errors=False: its record keeps the status, its path is empty)."""
    n = len(seqs)
    if both:
        recs, moves, dcal = findpath_batch_raw(list(seqs) * 2, list(starts) + list(ends), list(ends) + list(starts), width, temp, workspace_bytes)
        for p in range(n):
            f, r = recs[p], recs[n + p]
            if f["status"] == N.OK and r["status"] == N.OK and r["saddle_dcal"] < f["saddle_dcal"]:
                moves[p], dcal[p] = reverse_path(moves[n + p], dcal[n + p])
                recs[p] = dict(f, saddle_dcal=r["saddle_dcal"], saddle_step=int(np.argmax(dcal[p])))
        recs, moves, dcal = recs[:n], moves[:n], dcal[:n]
    else:
        recs, moves, dcal = findpath_batch_raw(seqs, starts, ends, width, temp, workspace_bytes)
    if raise_errors:
        for p, r in enumerate(recs):
            if r["status"] == N.ERR_STRUCT:
                raise ValueError(f"problem {p}: a row is malformed, of another length than the sequence, or holds a non-canonical pair")
            if r["status"] != N.OK:
                raise_for_status(r["status"], seqs[p], p, "findpath_batch", "RAFFT_FINDPATH_MAX_LEN",
                                 f"width {width} x {r['dist']} moves is above {N.FINDPATH_MAX_CANDIDATES} candidates, or an energy outside the sort key")
    return recs, moves, dcal


def findpath(seq, start, end, width=16, both=False, temp=37.0):
    recs, moves, dcal = findpath_batch([seq], [start], [end], width, both, temp)
    return recs[0], moves[0], dcal[0]


def path_rows(start, moves):
    """the len(moves) + 1 dot-bracket rows of a path that starts at `start`"""
    row = list(start)
    out = [start]
    for i, j in np.asarray(moves, dtype=np.int64).reshape(-1, 2).tolist():
        if i < 0:
            row[-i - 1] = row[-j - 1] = "."
        else:
            row[i], row[j] = "(", ")"
        out.append("".join(row))
    return out
