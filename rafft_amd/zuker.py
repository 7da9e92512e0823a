"""Minimum-free-energy structures on the GPU (rafft_mfe_batch): what the reference gets from ViennaRNA's
RNA.fold for the comparison column of its benchmark (benchmark_results/src/vrna_mfe.py:25, bench_mfe.py:11-15); the same under a
base-pair span (section 18) and under hard constraints and soft terms such as SHAPE data (section 20)."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .rafft import _per_sequence
from .utils import Structure, energies_from_dcal


def _mfe_raw(call, sequences, temp, knob, workspace_bytes):
    """(rows, dcal, n_pairs, status) of the C call `call`, whose one argument of its own (`knob`) lies between temp and workspace_bytes"""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    _, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    rec = (N.MfeSeq * n)()
    N.check(getattr(L, call)(n, arr, lens, float(temp), int(knob), int(workspace_bytes), rec, out))
    return ([b.value.decode("ascii") for b in bufs], [r.dcal for r in rec], [r.n_pairs for r in rec], [r.status for r in rec])


def _structures(raw, sequences, raise_errors, call, limit):
    """What a `_raw` call returned, as a list of utils.Structure; a sequence with an error as _per_sequence treats it"""
    rows, dcal, _, status = raw
    en = energies_from_dcal(np.asarray(dcal, dtype=np.int32)).tolist() if rows else []
    return _per_sequence(sequences, status, raise_errors, lambda k: Structure(rows[k], dcal[k], en[k]), call, limit)


def mfe_batch_raw(sequences, temp=37.0, max_lds_len=0, workspace_bytes=0):
    """(rows, dcal, n_pairs, status) of rafft_mfe_batch: dot-bracket strings and three int lists, one entry per sequence; nothing is
    raised for a sequence's own error (its row is all dots).  max_lds_len / workspace_bytes as in include/rafft_hip.h."""
    return _mfe_raw("rafft_mfe_batch", sequences, temp, max_lds_len, workspace_bytes)


def mfe_batch(sequences, temp=37.0, raise_errors=True):
    """The MFE structure of every sequence, as a list of utils.Structure.  A sequence with an error raises what fold_batch raises
    for it (raise_errors=False: its entry is None)."""
    return _structures(mfe_batch_raw(sequences, temp), sequences, raise_errors, "mfe_batch", "RAFFT_MFE_MAX_LEN")


def mfe(sequence, temp=37.0):
    return mfe_batch([sequence], temp)[0]


def mfe_span_batch_raw(sequences, max_span, temp=37.0, workspace_bytes=0):
    """(rows, dcal, n_pairs, status) of rafft_mfe_span_batch: the MFE structures whose pairs (i, j) all
    have j - i + 1 <= max_span, of sequences of up to N.MFE_SPAN_MAX_LEN nt.  As mfe_batch_raw otherwise."""
    return _mfe_raw("rafft_mfe_span_batch", sequences, temp, max_span, workspace_bytes)


def mfe_span_batch(sequences, max_span, temp=37.0, raise_errors=True):
    """The MFE structure under a maximum base-pair span of every sequence, as a list of utils.Structure; errors as mfe_batch."""
    return _structures(mfe_span_batch_raw(sequences, max_span, temp), sequences, raise_errors, "mfe_span_batch", "RAFFT_MFE_SPAN_MAX_LEN")


def mfe_span(sequence, max_span, temp=37.0):
    return mfe_span_batch([sequence], max_span, temp)[0]


class ConstrainedStructure(Structure):
    """A Structure of mfe_constrained_batch: `.dcal` / `.energy` are the objective (loop energies plus soft terms), `.pseudo_dcal`
    the soft terms of the row in dcal, so rafft_eval_structure of the row gives dcal - pseudo_dcal."""
    __slots__ = ("pseudo_dcal",)

    def __init__(self, str_struct, dcal, energy, pseudo_dcal):
        super().__init__(str_struct, dcal, energy)
        self.pseudo_dcal = int(pseudo_dcal)


def _soft_arrays(values, sequences, name):
    """(keep, arr): the array of pointers to one int32 array per sequence (a null pointer for None), or None for no argument"""
    if values is None:
        return None, None
    if len(values) != len(sequences):
        raise ValueError(f"{name}: {len(values)} entries for {len(sequences)} sequences")
    keep, ptrs = [], []
    for k, v in enumerate(values):
        if v is None:
            ptrs.append(None)
            continue
        a = np.ascontiguousarray(v, dtype=np.int32)
        if a.shape != (len(sequences[k]),):
            raise ValueError(f"{name}[{k}]: {a.shape} values for a sequence of {len(sequences[k])} nt")
        keep.append(a)
        ptrs.append(a.ctypes.data)
    return keep, (C.c_void_p * len(ptrs))(*ptrs)


def mfe_constrained_batch_raw(sequences, constraints=None, soft_unpaired=None, soft_stack=None, temp=37.0, max_lds_len=0, workspace_bytes=0):
    """(rows, dcal, n_pairs, pseudo_dcal, status) of rafft_mfe_constrained_batch.  constraints: per sequence a
    string of . x | < > ( ) or None; soft_unpaired / soft_stack: per sequence the dcal values u[k] / b[k] (array-like of its length) or
    None; each of the three may be None as a whole.  Nothing is raised for a sequence's own error (its row is all dots): a malformed
    constraint is ERR_STRUCT, constraints no structure satisfies ERR_INFEASIBLE."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    _, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    con = None
    if constraints is not None:
        if len(constraints) != n:
            raise ValueError(f"constraints: {len(constraints)} entries for {n} sequences")
        con = (C.c_char_p * n)(*[None if c is None else c.encode("ascii", "replace") for c in constraints])
    keep_u, u = _soft_arrays(soft_unpaired, sequences, "soft_unpaired")
    keep_b, b = _soft_arrays(soft_stack, sequences, "soft_stack")
    rec = (N.MfeConSeq * n)()
    N.check(L.rafft_mfe_constrained_batch(n, arr, lens, float(temp), con, u, b, int(max_lds_len), int(workspace_bytes), rec, out))
    del keep_u, keep_b
    return ([x.value.decode("ascii") for x in bufs], [r.dcal for r in rec], [r.n_pairs for r in rec], [r.pseudo_dcal for r in rec],
            [r.status for r in rec])


def mfe_constrained_batch(sequences, constraints=None, soft_unpaired=None, soft_stack=None, temp=37.0, raise_errors=True):
    """The constrained MFE structure of every sequence, as a list of ConstrainedStructure.  A sequence with an error raises what
    mfe_batch raises for it, a malformed constraint a ValueError, constraints no structure satisfies a RafftError
    (raise_errors=False: its entry is None)."""
    rows, dcal, _, pseudo, status = mfe_constrained_batch_raw(sequences, constraints, soft_unpaired, soft_stack, temp)
    if raise_errors:
        for k, st in enumerate(status):
            if st == N.ERR_STRUCT:
                raise ValueError(f"sequence {k}: malformed constraint {constraints[k]!r} (length, characters . x | < > ( ), balance, "
                                 "canonical forced pairs that enclose at least 3 positions)")
            if st == N.ERR_INFEASIBLE:
                raise N.RafftError(st, f"sequence {k}: no structure satisfies its constraints")
    en = energies_from_dcal(np.asarray(dcal, dtype=np.int32)).tolist() if rows else []
    return _per_sequence(sequences, status, raise_errors, lambda k: ConstrainedStructure(rows[k], dcal[k], en[k], pseudo[k]), "mfe_constrained_batch",
                         "RAFFT_MFE_MAX_LEN")


def mfe_constrained(sequence, constraint=None, soft_unpaired=None, soft_stack=None, temp=37.0):
    one = lambda x: None if x is None else [x]
    return mfe_constrained_batch([sequence], one(constraint), one(soft_unpaired), one(soft_stack), temp)[0]


def shape_deigan(reactivities, m=1.8, b=-0.6):
    """The Deigan pseudo-energies of SHAPE reactivities, in dcal, as soft_stack takes them (`RNAfold --shape`, method D):
    b[k] = rint(100 (m ln(r + 1) + b)) for r >= 0, 0 for missing data (r < 0 or NaN), clipped to +-RAFFT_MFE_SOFT_MAX."""
    r = np.asarray(reactivities, dtype=np.float64)
    have = ~np.isnan(r) & (r >= 0)
    e = np.rint(100.0 * (m * np.log(np.where(have, r, 0.0) + 1.0) + b))
    return np.where(have, np.clip(e, -N.MFE_SOFT_MAX, N.MFE_SOFT_MAX), 0).astype(np.int32)
