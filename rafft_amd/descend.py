"""Gradient walks to local minima on the GPU (rafft_descend_batch): what a user of the reference gets from
ViennaRNA's fold_compound.path_gradient (vrna_path_gradient), RNAlocmin or the flooding of `barriers` - the local minimum every
structure of a batch walks down to under insertion and deletion of single pairs, and with it the basins of a sample."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .findpath import findpath_batch
from .rafft import raise_for_status
from .utils import Structure, energies_from_dcal


def _row_block(rows, length):
    """(uint8 array of shape (n, stride), stride) of the start rows of one sequence: a list of strings (a row shorter than
    the sequence is padded with NULs, which the library reports as malformed; a longer one is refused here), or a uint8 array of shape
    (n, stride) as sample_batch_raw and subopt_batch_raw return them"""
    if isinstance(rows, np.ndarray):
        a = np.ascontiguousarray(rows, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("a row array has the shape (n_rows, stride)")
        return a, a.shape[1]
    enc = [r.encode("ascii", "replace") for r in rows]
    if any(len(e) > length for e in enc):
        raise ValueError("a row is longer than its sequence")
    stride = max(length, 1)
    a = np.zeros((len(enc), stride), dtype=np.uint8)
    for k, e in enumerate(enc):
        a[k, :len(e)] = np.frombuffer(e, dtype=np.uint8)
    return a, stride


def descend_batch_raw(sequences, rows, temp=37.0, max_steps=0, workspace_bytes=0, moves=True):
    """(seq_records, row_records, ends, moves) of rafft_descend_batch.  rows[s]: the start rows of sequence s (see _row_block).  seq_records: one dict per sequence (status, length, n_rows, row0); row_records:
    per sequence a dict of int32 arrays status, n_steps, start_dcal, end_dcal; ends: per sequence an (n_rows, L + 1) uint8 array - a
    row is the dot-bracket text and its NUL; moves: per sequence a list of (n_steps, 2) int32 arrays - (i, j) for an added pair,
    (-i-1, -j-1) for a removed one - or None with moves=False, which passes NULL.  Nothing is raised for an item's own error."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    if len(rows) != n:
        raise ValueError("one list of rows per sequence")
    enc, arr, lens = N.seq_arrays(sequences)
    blocks, strides = [], []
    for s in range(n):
        a, stride = _row_block(rows[s], len(enc[s]))
        blocks.append(a)
        strides.append(stride)
    n_rows = [b.shape[0] for b in blocks]
    bound = [int(max_steps) if max_steps > 0 else 2 * len(e) + 16 for e in enc]
    ends = [np.zeros((n_rows[s], len(enc[s]) + 1), dtype=np.uint8) for s in range(n)]
    mv = [np.zeros((n_rows[s], bound[s], 2), dtype=np.int32) for s in range(n)] if moves else None
    ptr = lambda a: a.ctypes.data if a.size else None
    srec = (N.DescendSeq * n)()
    total = sum(n_rows)
    rrec = np.zeros((total, 4), dtype=np.int32)
    N.check(L.rafft_descend_batch(n, arr, lens, (C.c_int * n)(*n_rows), (C.c_void_p * n)(*[ptr(b) for b in blocks]), (C.c_int * n)(*strides),
                                  float(temp), int(max_steps), int(workspace_bytes), srec, rrec.ctypes.data if total else None,
                                  (C.c_void_p * n)(*[ptr(e) for e in ends]), (C.c_void_p * n)(*[ptr(m) for m in mv]) if moves else None))
    seq_recs = [dict(status=r.status, length=r.length, n_rows=r.n_rows, row0=r.row0) for r in srec]
    row_recs, out_moves = [], [] if moves else None
    for s, q in enumerate(seq_recs):
        part = rrec[q["row0"]:q["row0"] + q["n_rows"]]
        row_recs.append(dict(status=part[:, 0].copy(), n_steps=part[:, 1].copy(), start_dcal=part[:, 2].copy(), end_dcal=part[:, 3].copy()))
        if moves:
            out_moves.append([mv[s][r, :part[r, 1]].copy() for r in range(q["n_rows"])])
    return seq_recs, row_recs, ends, out_moves


def end_rows(ends, length):
    """the end rows of one sequence as strings, from its (n_rows, L + 1) uint8 array"""
    text = ends[:, :-1].tobytes().decode("ascii", "replace")
    return [text[r * length:(r + 1) * length] for r in range(ends.shape[0])]


def descend_batch(seqs, rows, temp=37.0, max_steps=0, moves=False, raise_errors=True):
    """Per sequence a dict(rows, dcal, start_dcal, n_steps, status[, moves]): the local minimum every start row walks down to (as a
    string), its energy, the start's energy and the steps taken.  A sequence with an error raises what fold_batch raises for it, a
    malformed row a ValueError, a walk that max_steps stopped a RafftError (raise_errors=False: the statuses say it, the entry of
    a sequence with an error is None)."""
    srec, rrec, ends, mv = descend_batch_raw(seqs, rows, temp, max_steps, 0, moves)
    out = []
    for s, q in enumerate(srec):
        if q["status"] != N.OK:
            if raise_errors:
                raise_for_status(q["status"], seqs[s], s, "descend_batch", "RAFFT_DESCEND_MAX_LEN")
            out.append(None)
            continue
        st = rrec[s]["status"]
        if raise_errors and st.any():
            r = int(np.flatnonzero(st)[0])
            if st[r] == N.ERR_STRUCT:
                raise ValueError(f"sequence {s} row {r}: malformed, a non-canonical pair, or a hairpin of fewer than 3")
            raise N.RafftError(int(st[r]), f"sequence {s} row {r}: not at a minimum after {int(rrec[s]['n_steps'][r])} steps (max_steps)")
        d = dict(rows=end_rows(ends[s], q["length"]), dcal=rrec[s]["end_dcal"], start_dcal=rrec[s]["start_dcal"], n_steps=rrec[s]["n_steps"], status=st)
        if moves:
            d["moves"] = mv[s]
        out.append(d)
    return out


def group_minima(ends, dcal):
    """(minima, counts, basin_of) of the end rows of one sequence: the distinct rows as (row, dcal) sorted by (energy, first
    appearance), how many walks ended in each, and per walk the index of its minimum in that order"""
    first, energy, count = {}, {}, {}
    for r, (row, e) in enumerate(zip(ends, dcal)):
        if row not in first:
            first[row], energy[row], count[row] = r, int(e), 0
        count[row] += 1
    order = sorted(first, key=lambda row: (energy[row], first[row]))
    index = {row: k for k, row in enumerate(order)}
    return [(row, energy[row]) for row in order], [count[row] for row in order], np.array([index[row] for row in ends], dtype=np.int64)


def minima_batch(seqs, rows, temp=37.0, max_steps=0):
    """Per sequence (minima, counts, basin_of): the distinct local minima its rows walk down to as utils.Structure, sorted by
    (energy, first appearance), the number of rows in each basin, and basin_of[r], the index of row r's minimum."""
    out = []
    for s, d in enumerate(descend_batch(seqs, rows, temp, max_steps)):
        mins, counts, basin_of = group_minima(d["rows"], d["dcal"].tolist())
        en = energies_from_dcal(np.array([e for _, e in mins], dtype=np.int32)).tolist()
        out.append(([Structure(row, e, en[k]) for k, (row, e) in enumerate(mins)], counts, basin_of))
    return out


def basin_graph(seq, rows, width=16, max_minima=32, temp=37.0):
    """The basins of one sequence's rows and the barriers between them: dict(minima, counts, basin_of, saddle_dcal) with the lowest
    max_minima minima (basin_of is -1 for a row whose minimum is not among them) and the symmetric matrix of the saddles between them
    (the diagonal holds the minima's own energies), from one findpath_batch(both=True) call over all pairs."""
    minima, counts, basin_of = minima_batch([seq], [rows], temp)[0]
    m = min(len(minima), int(max_minima))
    minima, counts = minima[:m], counts[:m]
    basin_of = np.where(basin_of < m, basin_of, -1)
    sad = np.zeros((m, m), dtype=np.int64)
    for k in range(m):
        sad[k, k] = minima[k].dcal
    pairs = [(a, b) for a in range(m) for b in range(a + 1, m)]
    if pairs:
        recs, _, _ = findpath_batch([seq] * len(pairs), [minima[a].str_struct for a, _ in pairs], [minima[b].str_struct for _, b in pairs],
                                    width=width, both=True, temp=temp)
        for (a, b), r in zip(pairs, recs):
            sad[a, b] = sad[b, a] = r["saddle_dcal"]
    return dict(minima=minima, counts=counts, basin_of=basin_of, saddle_dcal=sad)
