"""Minimum-free-energy structures on the GPU (rafft_mfe_batch): what the reference gets from ViennaRNA's
RNA.fold for the comparison column of its benchmark (benchmark_results/src/vrna_mfe.py:25, bench_mfe.py:11-15)."""
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
