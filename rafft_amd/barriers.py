"""Exact barrier trees of energy bands on the GPU (rafft_barriers_batch): what a user of the reference gets
from `RNAsubopt -e D -s | barriers` - the local minima of a band, the exact saddle that joins each to a deeper one, the basin of
every structure and the tree coarse-grained kinetics starts from.  The landscape is the list of rows handed over, in its order."""
import ctypes as C

import numpy as np

from . import _native as N
from . import params as _params_mod
from .descend import _row_block
from .rafft import raise_for_status
from .utils import Structure, energies_from_dcal
from .wuchty import subopt_batch_raw


def barriers_batch_raw(sequences, rows, dcal, max_edges=0, workspace_bytes=0):
    """Per sequence a dict of rafft_barriers_batch's result: status, length, n_rows and the int32 arrays rank, father, saddle_rank,
    dcal, saddle_dcal, basin_size (one entry per minimum), basin ([n_rows]: minimum index) and edges ((n_edges, 3): a, b,
    saddle_rank).  rows[s]: the rows of sequence s as subopt_batch_raw / sample_batch_raw return them or a list of strings
    (descend._row_block); dcal[s]: their energies, non-decreasing.  Nothing is raised for a sequence's own error (its arrays are
    empty)."""
    L = N.lib()
    _params_mod.ensure_default_params()
    n = len(sequences)
    if len(rows) != n or len(dcal) != n:
        raise ValueError("one list of rows and one of energies per sequence")
    enc, arr, lens = N.seq_arrays(sequences)
    blocks, strides, dc = [], [], []
    for s in range(n):
        a, stride = _row_block(rows[s], len(enc[s]))
        d = np.ascontiguousarray(dcal[s], dtype=np.int32).reshape(-1)
        if d.shape[0] != a.shape[0]:
            raise ValueError(f"sequence {s}: {a.shape[0]} rows and {d.shape[0]} energies")
        blocks.append(a); strides.append(stride); dc.append(d)
    n_rows = [b.shape[0] for b in blocks]
    ptr = lambda a: a.ctypes.data if a.size else None
    res = C.POINTER(N.BarriersResult)()
    N.check(L.rafft_barriers_batch(n, arr, lens, (C.c_int * n)(*n_rows), (C.c_void_p * n)(*[ptr(b) for b in blocks]), (C.c_int * n)(*strides),
                                   (C.c_void_p * n)(*[ptr(d) for d in dc]), int(max_edges), int(workspace_bytes), C.byref(res)))
    out = []
    try:
        for k in range(n):
            r = res.contents.seq[k]
            mins = np.ctypeslib.as_array(C.cast(r.minima, C.POINTER(C.c_int32)), shape=(r.n_minima, 6)).copy() if r.n_minima else np.zeros((0, 6), np.int32)
            edges = np.ctypeslib.as_array(C.cast(r.edges, C.POINTER(C.c_int32)), shape=(r.n_edges, 3)).copy() if r.n_edges else np.zeros((0, 3), np.int32)
            basin = np.ctypeslib.as_array(r.basin, shape=(r.n_rows,)).copy() if r.n_minima else np.zeros(0, np.int32)
            out.append(dict(status=r.status, length=r.length, n_rows=r.n_rows, rank=mins[:, 0].copy(), father=mins[:, 1].copy(), saddle_rank=mins[:, 2].copy(),
                            dcal=mins[:, 3].copy(), saddle_dcal=mins[:, 4].copy(), basin_size=mins[:, 5].copy(), basin=basin, edges=edges))
    finally:
        L.rafft_barriers_free(res)
    return out


def barriers_counters():
    """of the last barriers_batch_raw: dict(chunks, launches, rows, hits, minima, edges)"""
    cnt = (C.c_longlong * 6)()
    N.check(N.lib().rafft_barriers_counters(C.byref(cnt)))
    return dict(zip(("chunks", "launches", "rows", "hits", "minima", "edges"), list(cnt)))


class Minimum(Structure):
    """a local minimum of a BarrierTree: a utils.Structure with father (minimum index, -1 for a root), barrier (kcal/mol, None for
    a root) and basin_size"""
    __slots__ = ("father", "barrier", "basin_size")


class BarrierTree:
    """The barrier tree of one landscape.  minima: a Minimum per local minimum (energy ascending by the list's order), each
    with father (minimum index, -1 for a root), barrier (kcal/mol, None for a root) and basin_size; dcal / saddle_dcal / father as
    int arrays; basin_of[row]: the minimum index of every row handed over; edges: (a, b, saddle_dcal) of adjacent basins."""

    def __init__(self, structures, dcal, father, saddle_dcal, basin_size, basin_of=None, edges=()):
        self.dcal = np.asarray(dcal, dtype=np.int64)
        self.father = np.asarray(father, dtype=np.int64)
        self.saddle_dcal = np.asarray(saddle_dcal, dtype=np.int64)
        self.basin_size = np.asarray(basin_size, dtype=np.int64)
        self.basin_of = np.zeros(0, dtype=np.int64) if basin_of is None else np.asarray(basin_of, dtype=np.int64)
        self.edges = [tuple(int(v) for v in e) for e in edges]
        en = energies_from_dcal(self.dcal).tolist()
        self.minima = []
        for k, row in enumerate(structures):
            st = Minimum(row, int(self.dcal[k]), en[k])
            st.father = int(self.father[k])
            st.barrier = None if st.father < 0 else (int(self.saddle_dcal[k]) - int(self.dcal[k])) / 100.0
            st.basin_size = int(self.basin_size[k])
            self.minima.append(st)

    def __len__(self):
        return len(self.minima)

    def _way_up(self, m):
        """[(minimum, the saddle of the link that leaves it)] from m to its root"""
        way = []
        while m >= 0:
            way.append((m, int(self.saddle_dcal[m])))
            m = int(self.father[m])
        return way

    def saddle_dcal_between(self, a, b):
        """the maximum saddle_dcal along the tree path between minima a and b; the minimum's own energy for a == b; None when they
        hang under different roots"""
        if a == b:
            return int(self.dcal[a])
        wa, wb = self._way_up(a), self._way_up(b)
        if wa[-1][0] != wb[-1][0]:
            return None
        # fathers have lower indices, so the two ways up meet where their tails agree
        while len(wa) > 1 and len(wb) > 1 and wa[-2][0] == wb[-2][0]:
            wa.pop(); wb.pop()
        return max(s for _, s in wa[:-1] + wb[:-1])

    def saddle(self, a, b):
        """the exact lowest saddle between minima a and b within the landscape, kcal/mol (None across roots)"""
        s = self.saddle_dcal_between(a, b)
        return None if s is None else s / 100.0

    def saddle_matrix(self, k=None):
        """dict(minima, saddle_dcal) for the k lowest minima, in the shape descend.basin_graph gives and rafft_kin.barrier_rates
        takes (saddle_dcal / 100): a symmetric int64 matrix, the diagonal the minima's energies; minima under different roots keep
        the higher of their energies (no saddle is known: barrier_rates then leaves the rate as it is)"""
        k = len(self) if k is None else min(int(k), len(self))
        sad = np.zeros((k, k), dtype=np.int64)
        for a in range(k):
            sad[a, a] = self.dcal[a]
            for b in range(a + 1, k):
                s = self.saddle_dcal_between(a, b)
                sad[a, b] = sad[b, a] = max(self.dcal[a], self.dcal[b]) if s is None else s
        return dict(minima=self.minima[:k], saddle_dcal=sad)

    def prune(self, minh):
        """A tree without the minima whose barrier is below minh kcal/mol; the basin of each is folded into its father's.  A dropped
        minimum's descendants go with it: they joined the tree through it, so their saddles are no higher than its saddle and
        their energies no lower than its energy - their barriers are no higher.  Roots stay."""
        h = int(round(float(minh) * 100.0))
        keep, into = [], np.arange(len(self), dtype=np.int64)
        for m in range(len(self)):
            f = int(self.father[m])
            if f >= 0 and (into[f] != f or int(self.saddle_dcal[m]) - int(self.dcal[m]) < h):
                into[m] = into[f]          # (fathers come first: into[f] is final)
            else:
                keep.append(m)
        new = {m: k for k, m in enumerate(keep)}
        size = np.zeros(len(keep), dtype=np.int64)
        for m in range(len(self)):
            size[new[int(into[m])]] += self.basin_size[m]
        basin_of = np.array([new[int(into[b])] for b in self.basin_of], dtype=np.int64)
        edges = {}
        for a, b, s in self.edges:
            a, b = sorted((new[int(into[a])], new[int(into[b])]))
            if a != b:
                edges[(a, b)] = min(s, edges.get((a, b), s))
        return BarrierTree([self.minima[m].str_struct for m in keep], self.dcal[keep], [new[int(self.father[m])] if self.father[m] >= 0 else -1 for m in keep],
                           self.saddle_dcal[keep], size, basin_of, sorted((a, b, s) for (a, b), s in edges.items()))

    def format(self):
        """the lines of `barriers`' listing: index (from 1) structure energy father (0 for a root) barrier, kcal/mol as the rest of
        the command line prints them"""
        lines = []
        for k, m in enumerate(self.minima):
            lines.append(f"{k + 1:4d} {m.str_struct} {m.dcal / 100.0:7.2f} {m.father + 1:4d} {0.0 if m.barrier is None else m.barrier:7.2f}\n")
        return "".join(lines)


def tree_from_record(rec, rows, dcal):
    """the BarrierTree of one record of barriers_batch_raw over the rows ((n, stride) uint8 array or list of strings) and energies"""
    L = rec["length"]
    text = (lambda r: rows[r][:L].tobytes().decode("ascii")) if isinstance(rows, np.ndarray) else (lambda r: rows[r])
    d = np.asarray(dcal, dtype=np.int64)
    edges = [(int(a), int(b), int(d[t])) for a, b, t in rec["edges"]]
    return BarrierTree([text(int(r)) for r in rec["rank"]], rec["dcal"], rec["father"], rec["saddle_dcal"], rec["basin_size"], rec["basin"], edges)


def barrier_trees(seqs, delta=1.0, max_structs=100000, temp=37.0, max_edges=0, raise_errors=True):
    """The barrier tree of every sequence's band of `delta` kcal/mol above its minimum free energy: one subopt call, one barriers
    call.  A sequence with an error raises what subopt_batch raises for it, one whose edges exceed max_edges a RafftError
    (raise_errors=False: its entry is None)."""
    delta_dcal = int(round(float(delta) * 100.0))
    if not 0 <= delta_dcal <= N.SUBOPT_MAX_DELTA:
        raise ValueError(f"delta is 0 .. {N.SUBOPT_MAX_DELTA // 100} kcal/mol")
    recs, rows, dcal = subopt_batch_raw(seqs, delta_dcal, max_structs, temp)
    for k, s in enumerate(seqs):
        if recs[k]["status"] != N.OK and raise_errors:
            raise_for_status(recs[k]["status"], s, k, "barrier_trees", "RAFFT_BARRIERS_MAX_LEN",
                             f"at least {recs[k]['n_reached']} structures within {delta} kcal/mol, max_structs is {max_structs}")
    ok = [k for k in range(len(seqs)) if recs[k]["status"] == N.OK]
    out = [None] * len(seqs)
    if ok:
        res = barriers_batch_raw([seqs[k] for k in ok], [rows[k] for k in ok], [dcal[k] for k in ok], max_edges)
        msg = N.lib().rafft_last_error().decode()
        for k, r in zip(ok, res):
            if r["status"] != N.OK:
                if raise_errors:
                    raise N.RafftError(int(r["status"]), msg)
                continue
            out[k] = tree_from_record(r, rows[k], dcal[k])
    return out


def barrier_tree(seq, delta=1.0, max_structs=100000, temp=37.0, max_edges=0):
    return barrier_trees([seq], delta, max_structs, temp, max_edges)[0]
