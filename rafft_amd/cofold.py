"""Minimum-free-energy structures of two-strand dimers on the GPU (rafft_cofold_batch): what RNAcofold's MFE
answers for a miRNA and its target, an antisense oligo, a probe or a primer dimer.  A dimer is written "A&B" or given as (A, B)."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .rafft import _per_sequence
from .utils import Structure, energies_from_dcal, paired_positions
from .zuker import mfe_batch_raw


def split_dimer(text):
    """(A, B) of "A&B"; a ValueError for a text without `&` or with more than one"""
    parts = text.split("&")
    if len(parts) != 2:
        raise ValueError(f"{text!r}: a dimer is written A&B, with one '&'")
    return parts[0], parts[1]


def _as_pairs(dimers):
    return [split_dimer(d) if isinstance(d, str) else (d[0], d[1]) for d in dimers]


def cofold_duplex_init(temp=37.0):
    """duplex_init in force at `temp`, in dcal: the loaded parameter file's DuplexInit scaled with its enthalpy, 410 with the built-in tables"""
    _params_mod.ensure_default_params()
    v = C.c_int()
    N.check(N.lib().rafft_cofold_duplex_init(float(temp), C.byref(v)))
    return v.value


def cofold_batch_raw(sequences, cuts=None, temp=37.0, max_lds_len=0, workspace_bytes=0):
    """(rows, dcal, n_pairs, n_inter, cut, status) of rafft_cofold_batch: sequences[s] is A followed by B without a separator,
    cuts[s] = len(A) (0, or cuts=None: a single strand); the rows have no separator either.  Nothing is raised for a sequence's
    own error (its row is all dots); a cut outside 0 .. len - 1 is ERR_STRUCT.  max_lds_len / workspace_bytes as mfe_batch_raw."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    if cuts is not None and len(cuts) != n:
        raise ValueError(f"cuts: {len(cuts)} entries for {n} sequences")
    _, arr, lens, bufs, out = N.seq_arrays(sequences, rows=True)
    cut = None if cuts is None else (C.c_int * n)(*[int(c) for c in cuts])
    rec = (N.CofoldSeq * n)()
    N.check(L.rafft_cofold_batch(n, arr, lens, cut, float(temp), int(max_lds_len), int(workspace_bytes), rec, out))
    return ([b.value.decode("ascii") for b in bufs], [r.dcal for r in rec], [r.n_pairs for r in rec], [r.n_inter for r in rec],
            [r.cut for r in rec], [r.status for r in rec])


class CofoldResult(Structure):
    """A Structure of cofold_batch: `.row` (and `.str_struct`) is rowA&rowB, `.dcal` / `.energy` the dimer's minimum free energy,
    `.n_inter` the pairs between the strands; with monomers=True `.energy_a`, `.energy_b` (the mfe_batch energies of the strands)
    and `.binding` = E(AB) - E(A) - E(B), in kcal/mol, with `.binding_dcal` the exact integer."""
    __slots__ = ("n_inter", "energy_a", "energy_b", "binding", "binding_dcal")

    def __init__(self, row, dcal, energy, n_inter):
        super().__init__(row, dcal, energy)
        self.n_inter = int(n_inter)
        self.energy_a = self.energy_b = self.binding = self.binding_dcal = None

    @property
    def row(self):
        return self.str_struct

    @property
    def pair_list(self):
        """the pairs, as positions of the concatenation A B"""
        return paired_positions(self.str_struct.replace("&", ""))


def cofold_batch(dimers, temp=37.0, monomers=False, raise_errors=True):
    """The MFE structure of every dimer, as a list of CofoldResult.  dimers: "A&B" strings or (A, B) pairs; both strands must hold
    a base.  monomers=True: one more mfe_batch call over all strands gives energy_a, energy_b and binding.  A dimer with an error
    raises what mfe_batch raises for the concatenation (raise_errors=False: its entry is None)."""
    pairs = _as_pairs(dimers)
    for k, (a, b) in enumerate(pairs):
        if not a or not b:
            raise ValueError(f"dimer {k}: an empty strand")
    seqs = [a + b for a, b in pairs]
    rows, dcal, _, n_inter, _, status = cofold_batch_raw(seqs, [len(a) for a, _ in pairs], temp)
    en = energies_from_dcal(np.asarray(dcal, dtype=np.int32)).tolist() if rows else []
    cut_row = lambda k: rows[k][:len(pairs[k][0])] + "&" + rows[k][len(pairs[k][0]):]
    out = _per_sequence(seqs, status, raise_errors, lambda k: CofoldResult(cut_row(k), dcal[k], en[k], n_inter[k]), "cofold_batch", "RAFFT_MFE_MAX_LEN")
    if monomers and out:
        mono = mfe_batch_raw([s for p in pairs for s in p], temp)
        md = mono[1]
        me = energies_from_dcal(np.asarray(md, dtype=np.int32)).tolist()
        for k, r in enumerate(out):
            if r is None or mono[3][2 * k] or mono[3][2 * k + 1]:
                continue
            r.energy_a, r.energy_b = me[2 * k], me[2 * k + 1]
            r.binding_dcal = r.dcal - md[2 * k] - md[2 * k + 1]
            r.binding = float(energies_from_dcal(np.asarray([r.binding_dcal], dtype=np.int32))[0])
    return out


def cofold(a, b, temp=37.0, monomers=False):
    return cofold_batch([(a, b)], temp, monomers)[0]
