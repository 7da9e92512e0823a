"""Prediction accuracy against a known structure: PPV and sensitivity as the reference obtains them
from RNAstructure's `scorer` (benchmark_results/scoring.py:76-94; SURVEY.md 8f-4, a "next" row).
`scorer`'s default rule: a pair (i,j) counts as found when the other structure holds (i,j), (i+-1,j)
or (i,j+-1).  Reproduces the pvv/sens columns of the reference's *_scores.csv (checked in tests)."""
from .utils import paired_positions


def _found(pair, others):
    i, j = pair
    return (i, j) in others or (i - 1, j) in others or (i + 1, j) in others or (i, j - 1) in others or (i, j + 1) in others


def score(predicted, known):
    """(ppv, sensitivity) in percent; the reference maps an undefined value (no pairs) to 0."""
    P, K = set(paired_positions(predicted)), set(paired_positions(known))
    ppv = 100.0 * sum(1 for p in P if _found(p, K)) / len(P) if P else 0.0
    sens = 100.0 * sum(1 for k in K if _found(k, P)) / len(K) if K else 0.0
    return ppv, sens


def best_of(structures, known):
    """The reference's selection in test_one_seq (scoring.py:83-94): last structure reaching the
    highest PPV (`>=`)."""
    best = (0.0, 0.0, None)
    for st in structures:
        db = st if isinstance(st, str) else st.str_struct
        p, s = score(db, known)
        if p >= best[0]:
            best = (p, s, db)
    return best


# ---- the same on the GPU, for whole beams of many sequences (include/rafft_hip.h: rafft_score_rows,
# rafft_score_result).  No CPU fallback: without the library or a GPU these raise.

def _row_dtype():
    import numpy as np
    return np.dtype([(k, "<i4") for k in ("n_pred", "hit_pred", "hit_known", "n_exact", "status")])


def _seq_dtype():
    import numpy as np
    return np.dtype([(k, "<i4") for k in ("status", "n_known", "n_rows", "row0", "pick_ppv", "pick_first")]
                    + [("best", _row_dtype()), ("first", _row_dtype())])


def _table(rows, seqs):
    """the score table: per row the counts, the index of its sequence and ppv / sens / bp_distance from them (fp64, the host
    formula); per sequence status, n_known, n_rows, row0 and the two picks (row indices within the sequence, -1 = none)"""
    import numpy as np
    row_seq = np.repeat(np.arange(len(seqs)), seqs["n_rows"])
    n_known = seqs["n_known"][row_seq].astype(np.int64)
    n_pred, hit_pred, hit_known = (rows[k].astype(np.int64) for k in ("n_pred", "hit_pred", "hit_known"))
    ppv = np.divide(100.0 * hit_pred, n_pred, out=np.zeros(len(rows)), where=n_pred > 0)
    sens = np.divide(100.0 * hit_known, n_known, out=np.zeros(len(rows)), where=n_known > 0)
    return dict(row_seq=row_seq, n_pred=rows["n_pred"], hit_pred=rows["hit_pred"], hit_known=rows["hit_known"], n_exact=rows["n_exact"],
                status=rows["status"], ppv=ppv, sens=sens, bp_distance=n_pred + n_known - 2 * rows["n_exact"],
                seq_status=seqs["status"], n_known=seqs["n_known"], n_rows=seqs["n_rows"], row0=seqs["row0"],
                pick_ppv=seqs["pick_ppv"], pick_first=seqs["pick_first"])


def _known_array(known):
    import ctypes as C
    return (C.c_char_p * len(known))(*[k.encode("ascii", "replace") for k in known])


def score_rows_gpu(rows_per_sequence, known, lengths=None):
    """Score every structure of every sequence against that sequence's known structure in one GPU call.
    rows_per_sequence[s]: the dot-bracket strings (or Structure objects) of sequence s, all of one length; known[s]: its known
    structure (( ) < > [ ] .).  lengths[s]: the sequence length when it cannot be read off the rows (default: the first row's
    length, or the known structure's for a sequence without rows).  Returns the score table (see _table): numpy arrays."""
    import ctypes as C
    import numpy as np
    from . import _native as N
    lib = N.lib()
    n = len(known)
    assert len(rows_per_sequence) == n
    bufs, lens = [], []
    for s, beam in enumerate(rows_per_sequence):
        dbs = [st if isinstance(st, str) else st.str_struct for st in beam]
        L = int(lengths[s]) if lengths is not None else len(dbs[0]) if dbs else len(known[s])
        if any(len(d) != L for d in dbs):
            raise ValueError(f"sequence {s}: rows of different lengths")
        bufs.append("".join(dbs).encode("ascii", "replace"))
        lens.append(L)
    counts = [len(b) for b in rows_per_sequence]
    row_out, seq_out = np.zeros(sum(counts), _row_dtype()), np.zeros(n, _seq_dtype())
    I = lambda v: (C.c_int * n)(*v)
    N.check(lib.rafft_score_rows(n, I(lens), I(counts), (C.c_char_p * n)(*bufs), I(lens), _known_array(known),
                                 row_out.ctypes.data_as(C.c_void_p), seq_out.ctypes.data_as(C.c_void_p)))
    return _table(row_out, seq_out)


def score_batch_gpu(batch_result, known):
    """The final beam of every sequence of a fold_batch result against known[s], scored where the fold left the rows (the
    library's pinned result memory goes to the device as it lies).  Returns the score table (see _table)."""
    import ctypes as C
    import numpy as np
    from . import _native as N
    lib = N.lib()
    res = batch_result._owner.res
    n = res.contents.n_seq
    assert len(known) == n
    total = 0
    for s in range(n):
        sr = res.contents.seq[s]
        if sr.status == N.OK and sr.n_steps > 0:
            total += sr.step_size[sr.n_steps - 1]
    row_out, seq_out = np.zeros(total, _row_dtype()), np.zeros(n, _seq_dtype())
    N.check(lib.rafft_score_result(res, _known_array(known), row_out.ctypes.data_as(C.c_void_p), seq_out.ctypes.data_as(C.c_void_p)))
    return _table(row_out, seq_out)


def best_of_gpu(structures, known):
    """best_of on the GPU: (ppv, sensitivity, dot-bracket) of the last structure reaching the highest PPV."""
    dbs = [st if isinstance(st, str) else st.str_struct for st in structures]
    t = score_rows_gpu([dbs], [known], lengths=[len(known)])
    k = int(t["pick_ppv"][0])
    if k < 0:
        return (0.0, 0.0, None)
    return (float(t["ppv"][k]), float(t["sens"][k]), dbs[k])
