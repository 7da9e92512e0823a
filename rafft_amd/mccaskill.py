"""Partition function, base-pair probabilities and centroid structures on the GPU (rafft_pf_batch): what a
user of the reference gets from ViennaRNA's RNA.fold_compound(seq, md).pf() / bpp(), the calls beside the RNA.fold of
benchmark_results/src/vrna_mfe.py:25.  The ensemble is the one mfe_batch minimises over.  Structures drawn from that ensemble
(rafft_sample_batch): what ViennaRNA's pbacktrack / `RNAsubopt -p` give.  Maximum-expected-accuracy structures
and the ensemble diversity from the pair probabilities, or from pair frequencies of any rows (rafft_mea_batch /
rafft_mea_probs_batch): what `RNAfold -p --MEA` gives.  The ensemble under hard constraints and SHAPE
pseudo-energies (rafft_pf_constrained_batch): what `RNAfold -p -C --enforceConstraint` and `RNAfold -p --shape`
give."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .rafft import _per_sequence
from .utils import structures_from_rows
from .zuker import _soft_arrays


class PfResult:
    """energy: ensemble free energy -kT ln Z in kcal/mol; centroid: the dot-bracket row of the pairs with P > 0.5; mfe_frequency:
    the share of the MFE structure in the ensemble; mfe_energy: that structure's energy in kcal/mol; probs: L x L numpy array,
    P(i pairs j) at [i][j] for i < j (None when not asked for; from pf_span_batch it is banded, shape (L, W), P(i, i+d) at [i][d]);
    unpaired: numpy array of the L unpaired probabilities (pf_span_batch, pf_constrained_batch; else None).  str_struct: the centroid, so that the scorers
    take it as a row."""
    __slots__ = ("energy", "centroid", "mfe_frequency", "mfe_energy", "probs", "unpaired")

    def __init__(self, energy, centroid, mfe_frequency, mfe_energy, probs=None, unpaired=None):
        self.energy, self.centroid, self.mfe_frequency, self.mfe_energy, self.probs = energy, centroid, mfe_frequency, mfe_energy, probs
        self.unpaired = unpaired

    @property
    def str_struct(self):
        return self.centroid

    def __repr__(self):
        return f"PfResult({self.centroid!r}, energy={self.energy:.2f}, mfe_frequency={self.mfe_frequency:.4g})"


_LEFT_RANGE = "the scaled partition function left the fp64 range"      # what RAFFT_ERR_CAPACITY of a sequence says in the calls below


def _fp64_buffers(shapes):
    """One zeroed fp64 numpy array per shape (None: no array for that sequence) and the array of pointers a call takes for them
    (null where there is no array or an empty one)"""
    bufs = [np.zeros(sh, dtype=np.float64) if sh is not None else None for sh in shapes]
    return bufs, (C.c_void_p * len(bufs))(*[b.ctypes.data if b is not None and b.size else None for b in bufs])


def pf_batch_raw(sequences, temp=37.0, scale_factor=0.0, workspace_bytes=0, probs=True):
    """(rows, records, probs) of rafft_pf_batch: the centroid rows, one dict per sequence with the fields of rafft_pf_seq, and -
    with probs=True - one L x L numpy array per sequence (None for a sequence longer than RAFFT_PF_MAX_LEN); nothing is raised
    for a sequence's own error (its row is all dots, its numbers are 0).  scale_factor / workspace_bytes as in include/rafft_hip.h."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    enc, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    rec = (N.PfSeq * n)()
    pr, ptrs = _fp64_buffers([(len(e), len(e)) if len(e) <= N.PF_MAX_LEN else None for e in enc]) if probs else (None, None)
    N.check(L.rafft_pf_batch(n, arr, lens, float(temp), float(scale_factor), int(workspace_bytes), rec, out, ptrs))
    recs = [{k: getattr(r, k) for k, _ in N.PfSeq._fields_} for r in rec]
    return [b.value.decode("ascii") for b in bufs], recs, pr


def pf_batch(sequences, temp=37.0, probs=True, raise_errors=True):
    """The ensemble of every sequence, as a list of PfResult.  A sequence with an error raises what fold_batch raises for it
    (raise_errors=False: its entry is None)."""
    rows, recs, pr = pf_batch_raw(sequences, temp, probs=probs)

    def make(k):
        return PfResult(recs[k]["energy"], rows[k], recs[k]["mfe_frequency"], recs[k]["mfe_dcal"] / 100.0, pr[k] if pr is not None else None)
    return _per_sequence(sequences, [r["status"] for r in recs], raise_errors, make, "pf_batch", "RAFFT_PF_MAX_LEN", _LEFT_RANGE)


def pf(sequence, temp=37.0, probs=True):
    return pf_batch([sequence], temp, probs)[0]


# ---- under a base-pair span (rafft_pf_span_batch)

def pf_span_batch_raw(sequences, max_span, temp=37.0, scale_factor=0.0, workspace_bytes=0, probs=True, unpaired=True):
    """(rows, records, probs, unpaired) of rafft_pf_span_batch: the centroid rows, one dict per sequence with the fields of
    rafft_pf_seq (mfe_dcal: the span MFE), with probs=True one BANDED (L, W) numpy array per sequence, W = min(max_span, L), P(i, i+d)
    at [i][d] (None for a sequence longer than RAFFT_MFE_SPAN_MAX_LEN), and with unpaired=True one array of L unpaired
    probabilities per sequence (None likewise); nothing is raised for a sequence's own error (its row is all dots, its numbers are
    0)."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n, max_span = len(sequences), int(max_span)
    enc, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    rec = (N.PfSeq * n)()
    fits = [len(e) <= N.MFE_SPAN_MAX_LEN for e in enc]
    width = max(1, min(max_span, N.MFE_MAX_LEN))       # (an argument the library refuses gets buffers of a legal shape)
    pr, ptrs = _fp64_buffers([(len(e), min(width, len(e))) if ok else None for e, ok in zip(enc, fits)]) if probs else (None, None)
    un, uptrs = _fp64_buffers([len(e) if ok else None for e, ok in zip(enc, fits)]) if unpaired else (None, None)
    N.check(L.rafft_pf_span_batch(n, arr, lens, float(temp), float(scale_factor), max_span, int(workspace_bytes), rec, out, ptrs, uptrs))
    recs = [{k: getattr(r, k) for k, _ in N.PfSeq._fields_} for r in rec]
    return [b.value.decode("ascii") for b in bufs], recs, pr, un


def pf_span_batch(sequences, max_span, temp=37.0, probs=True, raise_errors=True):
    """The ensemble of every sequence under `max_span`, as a list of PfResult whose probs are banded, shape (L, W), and which
    hold `unpaired`.  A sequence with an error raises what fold_batch raises for it (raise_errors=False: its entry is None)."""
    rows, recs, pr, un = pf_span_batch_raw(sequences, max_span, temp, probs=probs)

    def make(k):
        return PfResult(recs[k]["energy"], rows[k], recs[k]["mfe_frequency"], recs[k]["mfe_dcal"] / 100.0, pr[k] if pr is not None else None, un[k])
    return _per_sequence(sequences, [r["status"] for r in recs], raise_errors, make, "pf_span_batch", "RAFFT_MFE_SPAN_MAX_LEN", _LEFT_RANGE)


def pf_span(sequence, max_span, temp=37.0, probs=True):
    return pf_span_batch([sequence], max_span, temp, probs)[0]


# ---- under hard constraints and soft terms (rafft_pf_constrained_batch)

def pf_constrained_batch_raw(sequences, constraints=None, soft_unpaired=None, soft_stack=None, temp=37.0, scale_factor=0.0, workspace_bytes=0,
                             probs=True, unpaired=True):
    """(rows, records, probs, unpaired) of rafft_pf_constrained_batch: the centroid rows, one dict per sequence with the fields of
    rafft_pf_seq (mfe_dcal: the constrained objective), with probs=True one L x L numpy array per sequence (None beyond
    RAFFT_PF_MAX_LEN) and with unpaired=True one array of L unpaired probabilities (None likewise).  constraints, soft_unpaired and
    soft_stack as zuker.mfe_constrained_batch_raw takes them (shape_deigan makes soft_stack from reactivities).  Nothing is raised for
    a sequence's own error (its row is all dots, its numbers are 0): a malformed constraint is ERR_STRUCT, constraints no structure
    satisfies ERR_INFEASIBLE."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    enc, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    con = None
    if constraints is not None:
        if len(constraints) != n:
            raise ValueError(f"constraints: {len(constraints)} entries for {n} sequences")
        con = (C.c_char_p * n)(*[None if c is None else c.encode("ascii", "replace") for c in constraints])
    keep_u, u = _soft_arrays(soft_unpaired, sequences, "soft_unpaired")
    keep_b, b = _soft_arrays(soft_stack, sequences, "soft_stack")
    rec = (N.PfSeq * n)()
    fits = [len(e) <= N.PF_MAX_LEN for e in enc]
    pr, ptrs = _fp64_buffers([(len(e), len(e)) if ok else None for e, ok in zip(enc, fits)]) if probs else (None, None)
    un, uptrs = _fp64_buffers([len(e) if ok else None for e, ok in zip(enc, fits)]) if unpaired else (None, None)
    N.check(L.rafft_pf_constrained_batch(n, arr, lens, float(temp), con, u, b, float(scale_factor), int(workspace_bytes), rec, out, ptrs, uptrs))
    del keep_u, keep_b
    recs = [{k: getattr(r, k) for k, _ in N.PfSeq._fields_} for r in rec]
    return [x.value.decode("ascii") for x in bufs], recs, pr, un


def pf_constrained_batch(sequences, constraints=None, soft_unpaired=None, soft_stack=None, temp=37.0, probs=True, raise_errors=True):
    """The ensemble of every sequence under its constraints and soft terms, as a list of PfResult that hold `unpaired` - the
    modelled accessibility to set beside a probe; mfe_energy is the constrained objective in kcal/mol.  The centroid need not satisfy
    a `|`.  mea_from_probs over the `probs` of these results is the MEA row under the data.  A sequence with an error raises what
    pf_batch raises for it, a malformed constraint a ValueError, constraints no structure satisfies a RafftError (raise_errors=False:
    its entry is None)."""
    rows, recs, pr, un = pf_constrained_batch_raw(sequences, constraints, soft_unpaired, soft_stack, temp, probs=probs)
    status = [r["status"] for r in recs]
    if raise_errors:
        for k, st in enumerate(status):
            if st == N.ERR_STRUCT:
                raise ValueError(f"sequence {k}: malformed constraint {constraints[k]!r} (length, characters . x | < > ( ), balance, "
                                 "canonical forced pairs that enclose at least 3 positions)")
            if st == N.ERR_INFEASIBLE:
                raise N.RafftError(st, f"sequence {k}: no structure satisfies its constraints")

    def make(k):
        return PfResult(recs[k]["energy"], rows[k], recs[k]["mfe_frequency"], recs[k]["mfe_dcal"] / 100.0, pr[k] if pr is not None else None, un[k])
    return _per_sequence(sequences, status, raise_errors, make, "pf_constrained_batch", "RAFFT_PF_MAX_LEN", _LEFT_RANGE)


def pf_constrained(sequence, constraint=None, soft_unpaired=None, soft_stack=None, temp=37.0, probs=True):
    one = lambda x: None if x is None else [x]
    return pf_constrained_batch([sequence], one(constraint), one(soft_unpaired), one(soft_stack), temp, probs)[0]


def band_to_dense(band):
    """The L x L matrix of a banded (L, W) array: band[i][d] at [i][i + d] (for short sequences: L x L doubles)"""
    band = np.asarray(band)
    L, W = band.shape
    dense = np.zeros((L, L), dtype=band.dtype)
    for d in range(min(W, L)):
        dense[np.arange(L - d), np.arange(d, L)] = band[:L - d, d]
    return dense


def band_pairs(band, cutoff=1e-5):
    """[(i, j, p)] of the pairs with p >= cutoff in a banded (L, W) array, 0-based, i ascending then j"""
    band = np.asarray(band)
    L = band.shape[0]
    i, d = np.nonzero(band >= cutoff)                  # row-major: i ascending, then d
    keep = i + d < L
    return [(int(a), int(a + b), float(band[a, b])) for a, b in zip(i[keep], d[keep])]


def dense_pairs(dense, cutoff=1e-5):
    """band_pairs for an L x L matrix (P at [i][j], i < j)"""
    i, j = np.nonzero(np.triu(np.asarray(dense), 1) >= cutoff)
    return [(int(a), int(b), float(dense[a, b])) for a, b in zip(i, j)]


def _seeds_of(seeds, n):
    """None, one int for every sequence, or one int per sequence -> a list of n ints below 2^64, or None"""
    if seeds is None:
        return None
    if isinstance(seeds, (int, np.integer)):
        seeds = [int(seeds)] * n
    seeds = [int(x) for x in seeds]
    if len(seeds) != n:
        raise ValueError(f"{len(seeds)} seeds for {n} sequences")
    if any(not 0 <= x < 1 << 64 for x in seeds):
        raise ValueError("a seed is an integer in 0 .. 2^64 - 1")
    return seeds


def sample_batch_raw(sequences, n_samples, seeds=None, temp=37.0, scale_factor=0.0, workspace_bytes=0):
    """(records, rows, dcal) of rafft_sample_batch: one dict per sequence with the fields of rafft_sample_seq, per sequence an
    (n_samples, L + 1) uint8 array - a row is the dot-bracket text and its NUL - and an int32 array of the rows' energies in
    dcal/mol.  Nothing is raised for a sequence's own error (its rows are all dots, its record has n_samples 0).  seeds: None (all
    0), one int used for every sequence, or one int per sequence; row k of a sequence depends on its seed and k, not on n_samples
    or the batch.  scale_factor / workspace_bytes as in include/rafft_hip.h."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n, n_samples = len(sequences), int(n_samples)
    enc, arr, lens = N.seq_arrays(sequences)
    seeds = _seeds_of(seeds, n)
    sd = (C.c_ulonglong * n)(*seeds) if seeds is not None else None
    rec = (N.SampleSeq * n)()
    if not 0 <= n_samples <= N.SAMPLE_MAX:       # (no buffers for a call the library refuses)
        N.check(L.rafft_sample_batch(n, arr, lens, float(temp), float(scale_factor), int(workspace_bytes), n_samples, sd, rec, None, None))
    rows = [np.zeros((n_samples, len(e) + 1), dtype=np.uint8) for e in enc]
    dcal = [np.zeros(n_samples, dtype=np.int32) for _ in enc]
    out = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
    dc = (C.c_void_p * n)(*[d.ctypes.data for d in dcal])
    N.check(L.rafft_sample_batch(n, arr, lens, float(temp), float(scale_factor), int(workspace_bytes), n_samples, sd, rec, out, dc))
    recs = [{k: getattr(r, k) for k, _ in N.SampleSeq._fields_} for r in rec]
    return recs, rows, dcal


def sample_batch(sequences, n_samples, seeds=None, temp=37.0, raise_errors=True):
    """n_samples structures drawn from the Boltzmann ensemble of every sequence, as a list of lists of utils.Structure (in the
    order drawn, repeats included).  A sequence with an error raises what fold_batch raises for it (raise_errors=False: None)."""
    recs, rows, dcal = sample_batch_raw(sequences, n_samples, seeds, temp)
    return _per_sequence(sequences, [r["status"] for r in recs], raise_errors, lambda k: structures_from_rows(rows[k], dcal[k], len(sequences[k])),
                         "sample_batch", "RAFFT_PF_MAX_LEN", _LEFT_RANGE)


def sample(sequence, n_samples, seed=None, temp=37.0):
    return sample_batch([sequence], n_samples, seed, temp)[0]


# ---- maximum-expected-accuracy structures (rafft_mea_batch / rafft_mea_probs_batch)

class MeaResult:
    """structure: the MEA row; mea: its expected accuracy, the sum of 2 gamma P over its pairs and of the unpaired probabilities
    over its unpaired positions; energy_of_structure: the row's energy in kcal/mol (None for a row made from a matrix alone);
    energy: the ensemble free energy in kcal/mol (None likewise); diversity: the mean base-pair distance of the ensemble, sum of
    2 P (1 - P); unpaired: numpy array of q; probs: L x L numpy array or None.  str_struct: the row, so that the scorers take it."""
    __slots__ = ("structure", "mea", "energy_of_structure", "energy", "diversity", "unpaired", "probs")

    def __init__(self, structure, mea, energy_of_structure, energy, diversity, unpaired, probs=None):
        self.structure, self.mea, self.energy_of_structure, self.energy = structure, mea, energy_of_structure, energy
        self.diversity, self.unpaired, self.probs = diversity, unpaired, probs

    @property
    def str_struct(self):
        return self.structure

    def __repr__(self):
        return f"MeaResult({self.structure!r}, mea={self.mea:.2f}, diversity={self.diversity:.2f})"


def mea_batch_raw(sequences, gamma=1.0, temp=37.0, scale_factor=0.0, workspace_bytes=0, probs=True):
    """(rows, records, probs, unpaired) of rafft_mea_batch: the MEA rows, one dict per sequence with the fields of rafft_mea_seq,
    with probs=True one L x L numpy array per sequence (None beyond RAFFT_PF_MAX_LEN), and one array of L unpaired probabilities
    per sequence; nothing is raised for a sequence's own error (its row is all dots, its numbers are 0)."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    enc, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    rec = (N.MeaSeq * n)()
    pr, ptrs = _fp64_buffers([(len(e), len(e)) if len(e) <= N.PF_MAX_LEN else None for e in enc]) if probs else (None, None)
    un, uptrs = _fp64_buffers([len(e) for e in enc])
    N.check(L.rafft_mea_batch(n, arr, lens, float(temp), float(scale_factor), int(workspace_bytes), float(gamma), rec, out, ptrs, uptrs))
    recs = [{k: getattr(r, k) for k, _ in N.MeaSeq._fields_} for r in rec]
    return [b.value.decode("ascii") for b in bufs], recs, pr, un


def mea_batch(sequences, gamma=1.0, temp=37.0, probs=False, raise_errors=True):
    """The MEA structure of every sequence, as a list of MeaResult.  A sequence with an error raises what fold_batch raises for it
    (raise_errors=False: its entry is None)."""
    rows, recs, pr, un = mea_batch_raw(sequences, gamma, temp, probs=probs)

    def make(k):
        return MeaResult(rows[k], recs[k]["mea"], recs[k]["dcal"] / 100.0, recs[k]["energy"], recs[k]["diversity"], un[k], pr[k] if pr is not None else None)
    return _per_sequence(sequences, [r["status"] for r in recs], raise_errors, make, "mea_batch", "RAFFT_PF_MAX_LEN", _LEFT_RANGE)


def mea(sequence, gamma=1.0, temp=37.0):
    return mea_batch([sequence], gamma, temp)[0]


def mea_from_probs_raw(matrices, gamma=1.0, workspace_bytes=0):
    """(rows, records, unpaired) of rafft_mea_probs_batch for a list of square fp64 matrices (only [i][j], i < j, is read)"""
    L = N.lib()
    mats = [np.ascontiguousarray(m, dtype=np.float64) for m in matrices]
    for k, m in enumerate(mats):
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise ValueError(f"matrix {k}: shape {m.shape} is not square")
    n = len(mats)
    lens = (C.c_int * n)(*[m.shape[0] for m in mats])
    ptrs = (C.c_void_p * n)(*[m.ctypes.data if m.size else None for m in mats])
    bufs = [C.create_string_buffer(m.shape[0] + 1) for m in mats]
    out = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    un, uptrs = _fp64_buffers([m.shape[0] for m in mats])
    rec = (N.MeaProbsSeq * n)()
    N.check(L.rafft_mea_probs_batch(n, lens, ptrs, float(gamma), int(workspace_bytes), rec, out, uptrs))
    recs = [{k: getattr(r, k) for k, _ in N.MeaProbsSeq._fields_} for r in rec]
    return [b.value.decode("ascii") for b in bufs], recs, un


def mea_from_probs(matrices, gamma=1.0):
    """The MEA row of every matrix of pair probabilities or pair frequencies (pair_frequencies), as a list of MeaResult without
    energies.  An empty matrix or one beyond RAFFT_PF_MAX_LEN raises ValueError."""
    rows, recs, un = mea_from_probs_raw(matrices, gamma)
    out = []
    for k, r in enumerate(recs):
        if r["status"] != N.OK:
            raise ValueError(f"matrix {k}: " + ("empty" if r["status"] == N.ERR_EMPTY else "longer than RAFFT_PF_MAX_LEN"))
        out.append(MeaResult(rows[k], r["mea"], None, None, r["diversity"], un[k], None))
    return out


def pair_frequencies(rows, weights=None):
    """The L x L matrix mea_from_probs takes, from dot-bracket rows of one length (text, bytes, or objects with str_struct): at
    [i][j], i < j, the weighted share of the rows that hold the pair (i,j).  weights: one non-negative number per row (None: all
    equal); they are normalised to sum 1."""
    texts = [r if isinstance(r, str) else r.decode("ascii") if isinstance(r, (bytes, bytearray)) else r.str_struct for r in rows]
    if not texts:
        raise ValueError("no rows")
    L = len(texts[0])
    w = np.ones(len(texts)) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (len(texts),) or (w < 0).any() or not w.sum() > 0:
        raise ValueError("weights: one non-negative number per row, not all zero")
    counts = {}
    for t, x in zip(texts, w):
        if len(t) != L:
            raise ValueError("rows of different lengths")
        stack = []
        for j, ch in enumerate(t):
            if ch == "(":
                stack.append(j)
            elif ch == ")":
                if not stack:
                    raise ValueError(f"unbalanced row {t!r}")
                key = (stack.pop(), j)
                counts[key] = counts.get(key, 0.0) + x
            elif ch != ".":
                raise ValueError(f"row {t!r} holds {ch!r}")
        if stack:
            raise ValueError(f"unbalanced row {t!r}")
    F = np.zeros((L, L), dtype=np.float64)
    total = float(w.sum())
    for (i, j), x in counts.items():
        F[i, j] = min(1.0, x / total)
    return F
