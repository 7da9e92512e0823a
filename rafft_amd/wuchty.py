"""Every structure within an energy band above the minimum free energy, on the GPU (rafft_subopt_batch): what
a user of the reference gets from `RNAsubopt -e delta -s`, the file its landscape tool reads with --sub (utility/surface.py:54-63).
The ensemble is the one mfe_batch minimises over; the enumeration is that of Wuchty, Fontana, Hofacker and Schuster (1999)."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .rafft import raise_for_status
from .utils import structures_from_rows


def subopt_batch_raw(sequences, delta_dcal, max_structs=100000, temp=37.0, workspace_bytes=0):
    """(records, rows, dcal) of rafft_subopt_batch: one dict per sequence with the numbers of rafft_subopt_seq, per sequence an
    (n_structs, L + 1) uint8 array - a row is the dot-bracket text and its NUL - and an int32 array of the rows' energies in
    dcal/mol, ascending, equal energies in enumeration order.  Nothing is raised for a sequence's own error (it has no rows; with
    RAFFT_ERR_CAPACITY its record holds n_reached).  delta_dcal / max_structs / workspace_bytes as in include/rafft_hip.h."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    enc, arr, lens = N.seq_arrays(sequences)
    res = C.POINTER(N.SuboptResult)()
    N.check(L.rafft_subopt_batch(n, arr, lens, float(temp), int(delta_dcal), int(max_structs), int(workspace_bytes), C.byref(res)))
    try:
        recs, rows, dcal = [], [], []
        for k in range(n):
            r = res.contents.seq[k]
            recs.append(dict(status=r.status, length=r.length, mfe_dcal=r.mfe_dcal, n_structs=r.n_structs, n_reached=r.n_reached))
            ns, w = r.n_structs, r.length + 1
            if ns:
                rows.append(np.frombuffer(C.string_at(r.db, ns * w), dtype=np.uint8).reshape(ns, w).copy())
                dcal.append(np.ctypeslib.as_array(r.dcal, shape=(ns,)).astype(np.int32, copy=True))
            else:
                rows.append(np.zeros((0, w), dtype=np.uint8))
                dcal.append(np.zeros(0, dtype=np.int32))
    finally:
        L.rafft_subopt_free(res)
    return recs, rows, dcal


def subopt_batch(sequences, delta=1.0, max_structs=100000, temp=37.0, raise_errors=True):
    """Every structure of each sequence within `delta` kcal/mol of its minimum free energy (as `RNAsubopt -e delta -s`), as a list
    of lists of utils.Structure, energies ascending.  A sequence with an error raises what fold_batch raises for it, one with more
    than max_structs structures in the band a RafftError (raise_errors=False: its entry is None)."""
    delta_dcal = int(round(float(delta) * 100.0))
    if not 0 <= delta_dcal <= N.SUBOPT_MAX_DELTA:
        raise ValueError(f"delta is 0 .. {N.SUBOPT_MAX_DELTA // 100} kcal/mol")
    recs, rows, dcal = subopt_batch_raw(sequences, delta_dcal, max_structs, temp)
    out = []
    for k, s in enumerate(sequences):
        st = recs[k]["status"]
        if st != N.OK:
            if raise_errors:
                raise_for_status(st, s, k, "subopt_batch", "RAFFT_SUBOPT_MAX_LEN",
                                 f"at least {recs[k]['n_reached']} structures within {delta} kcal/mol, max_structs is {max_structs}")
            out.append(None)
        else:
            out.append(structures_from_rows(rows[k], dcal[k], len(s)))
    return out


def subopt(sequence, delta=1.0, max_structs=100000, temp=37.0):
    return subopt_batch([sequence], delta, max_structs, temp)[0]
