"""Independent restatement of the reference's accuracy scoring (benchmark_results/scoring.py:12-28,76-94) on pair SETS, for the
tests of the GPU scoring: integer counts, the `>=` pick.  Imports nothing from rafft_amd."""
import numpy as np


def pairs(db):
    """scoring.py:12-28: ( and < share a stack, [ has its own"""
    reg, pk, out = [], [], set()
    for i, c in enumerate(db):
        if c in "(<":
            reg.append(i)
        elif c == "[":
            pk.append(i)
        elif c in ")>":
            out.add((reg.pop(), i))
        elif c == "]":
            out.add((pk.pop(), i))
    return out


def counts(pred, known):
    """(n_pred, hit_pred, hit_known, n_exact, n_known): `scorer`'s rule - a pair (i, j) is found when the other structure holds
    (i, j), (i +- 1, j) or (i, j +- 1)"""
    P, K = pairs(pred), pairs(known)
    found = lambda p, S: any(q in S for q in ((p[0], p[1]), (p[0] - 1, p[1]), (p[0] + 1, p[1]), (p[0], p[1] - 1), (p[0], p[1] + 1)))
    return len(P), sum(found(p, K) for p in P), sum(found(k, P) for k in K), len(P & K), len(K)


def table(rows_per_sequence, known):
    """the score table of rafft_amd.scoring.score_rows_gpu, same keys, for well-formed input"""
    rows, seqs = [], []
    for s, (beam, kn) in enumerate(zip(rows_per_sequence, known)):
        best, best_ppv, n_known = -1, 0.0, len(pairs(kn))
        for r, db in enumerate(beam):
            n_pred, hit_pred, hit_known, n_exact, _ = counts(db, kn)
            ppv = 100.0 * hit_pred / n_pred if n_pred else 0.0
            if ppv >= best_ppv:                         # scoring.py:90-91
                best, best_ppv = r, ppv
            rows.append((s, n_pred, hit_pred, hit_known, n_exact))
        seqs.append((n_known, len(beam), len(rows) - len(beam), best, 0 if beam else -1))
    rows = np.array(rows, dtype=np.int64).reshape(-1, 5)
    seqs = np.array(seqs, dtype=np.int64).reshape(-1, 5)
    n_known = seqs[rows[:, 0], 0]
    ppv = np.array([100.0 * h / n if n else 0.0 for h, n in zip(rows[:, 2], rows[:, 1])])
    sens = np.array([100.0 * h / n if n else 0.0 for h, n in zip(rows[:, 3], n_known)])
    return dict(row_seq=rows[:, 0], n_pred=rows[:, 1], hit_pred=rows[:, 2], hit_known=rows[:, 3], n_exact=rows[:, 4],
                status=np.zeros(len(rows), np.int64), ppv=ppv, sens=sens, bp_distance=rows[:, 1] + n_known - 2 * rows[:, 4],
                seq_status=np.zeros(len(seqs), np.int64), n_known=seqs[:, 0], n_rows=seqs[:, 1], row0=seqs[:, 2],
                pick_ppv=seqs[:, 3], pick_first=seqs[:, 4])


def table_lines(records, beams, select):
    """the lines of the reference's score table (scoring.py:120-128) for records (seq, known, name) and their beams of
    (dot-bracket, dcal) in beam order; select "ppv": last `>=` (scoring.py:90-91), "energy": the first structure (--one)"""
    out = ["seq,len_seq,struct,nrj,nbp,pvv,sens,name"]
    for (seq, known, name), beam in zip(records, beams):
        scored = [counts(db, known) for db, _ in beam]
        ppv = [100.0 * c[1] / c[0] if c[0] else 0.0 for c in scored]
        k, best = 0, 0.0
        if select == "ppv":
            for i, p in enumerate(ppv):
                if p >= best:
                    best, k = p, i
        (db, dcal), c = beam[k], scored[k]
        sens = 100.0 * c[2] / c[4] if c[4] else 0.0
        nrj = float(np.float32(np.float64(np.float32(dcal)) / 100.0))         # ViennaRNA's (float)en / 100. through a float
        out.append(f"{seq},{len(seq)},{db},{nrj!r},{db.count('(')},{round(ppv[k], 2)!r},{round(sens, 2)!r},{name}")
    return out
