"""Partition function, base-pair probabilities and centroid structures on the GPU (rafft_pf_batch): what a
user of the reference gets from ViennaRNA's RNA.fold_compound(seq, md).pf() / bpp(), the calls beside the RNA.fold of
benchmark_results/src/vrna_mfe.py:25.  The ensemble is the one mfe_batch minimises over."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .rafft import _raise_like_reference


class PfResult:
    """energy: ensemble free energy -kT ln Z in kcal/mol; centroid: the dot-bracket row of the pairs with P > 0.5; mfe_frequency:
    the share of the MFE structure in the ensemble; mfe_energy: that structure's energy in kcal/mol; probs: L x L numpy array,
    P(i pairs j) at [i][j] for i < j (None when not asked for).  str_struct: the centroid, so that the scorers take it as a row."""
    __slots__ = ("energy", "centroid", "mfe_frequency", "mfe_energy", "probs")

    def __init__(self, energy, centroid, mfe_frequency, mfe_energy, probs=None):
        self.energy, self.centroid, self.mfe_frequency, self.mfe_energy, self.probs = energy, centroid, mfe_frequency, mfe_energy, probs

    @property
    def str_struct(self):
        return self.centroid

    def __repr__(self):
        return f"PfResult({self.centroid!r}, energy={self.energy:.2f}, mfe_frequency={self.mfe_frequency:.4g})"


def pf_batch_raw(sequences, temp=37.0, scale_factor=0.0, workspace_bytes=0, probs=True):
    """(rows, records, probs) of rafft_pf_batch: the centroid rows, one dict per sequence with the fields of rafft_pf_seq, and -
    with probs=True - one L x L numpy array per sequence (None for a sequence longer than RAFFT_PF_MAX_LEN); nothing is raised
    for a sequence's own error (its row is all dots, its numbers are 0).  scale_factor / workspace_bytes as in include/rafft_hip.h."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    enc, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    rec = (N.PfSeq * n)()
    pr, ptrs = None, None
    if probs:
        pr = [np.zeros((len(e), len(e)), dtype=np.float64) if len(e) <= N.PF_MAX_LEN else None for e in enc]
        ptrs = (C.c_void_p * n)(*[p.ctypes.data if p is not None and p.size else None for p in pr])
    N.check(L.rafft_pf_batch(n, arr, lens, float(temp), float(scale_factor), int(workspace_bytes), rec, out, ptrs))
    recs = [{k: getattr(r, k) for k, _ in N.PfSeq._fields_} for r in rec]
    return [b.value.decode("ascii") for b in bufs], recs, pr


def pf_batch(sequences, temp=37.0, probs=True, raise_errors=True):
    """The ensemble of every sequence, as a list of PfResult.  A sequence with an error raises what fold_batch raises for it
    (raise_errors=False: its entry is None)."""
    rows, recs, pr = pf_batch_raw(sequences, temp, probs=probs)
    out = []
    for k, s in enumerate(sequences):
        st = recs[k]["status"]
        if st != N.OK:
            if raise_errors:
                if st == N.ERR_TOO_LONG:
                    raise ValueError(f"sequence of {len(s)} nt: pf_batch takes up to {N.PF_MAX_LEN} nt (RAFFT_PF_MAX_LEN)")
                if st == N.ERR_CAPACITY:
                    raise N.RafftError(st, f"sequence {k}: the scaled partition function left the fp64 range")
                _raise_like_reference(st, s)
            out.append(None)
        else:
            out.append(PfResult(recs[k]["energy"], rows[k], recs[k]["mfe_frequency"], recs[k]["mfe_dcal"] / 100.0, pr[k] if pr is not None else None))
    return out


def pf(sequence, temp=37.0, probs=True):
    return pf_batch([sequence], temp, probs)[0]
