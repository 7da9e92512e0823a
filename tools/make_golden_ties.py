"""Golden vectors for tie-heavy, low-complexity sequences (repeats): on those almost every decision of the fold is a
tie-break, which the reference defines only implicitly - lag ranking by value descending, then lag descending
(`sorted` followed by `[::-1]`), the best stem of a lag by a `>=` arg-max, the beam as a children-before-parents
stable merge.  Container only, like tools/make_golden.py: the reference's own Python runs with that tool's stand-in
`RNA` module (energies from the KAT-pinned oracle evaluator, everything else REFERENCE code) and its `create_childs`
recording hook; the reference is imported when this script runs and nothing of its text is copied.

Outputs (tests/golden/):
  fold_traj_ties.json.gz    full trajectories, layout of fold_traj.json.gz           (reference Python)
  node_expand_ties.json.gz  per-region records, layout of node_expand.json.gz        (reference Python)
  fold_ties_long.json.gz    trajectories of repeats of 1100-4200 nt, where the reference's Python is too slow: by the
                            CPU oracle (oracle/rafft_oracle.c), which the two files above pin on ties

Usage: python tools/make_golden_ties.py [--jobs N] [--only-long]
"""
import gzip
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GOLD = os.path.join(ROOT, "tests", "golden")
FAMILIES = ("GC", "AU", "GU", "CUG", "GGGAAACCC", "GGGGCCCC", "GC+A", "GC+N5")
LENGTHS = (33, 130, 257, 600)
# region records per fold: non-contiguous regions are always taken (up to NONCONTIG of them), the root and every
# third contiguous region up to CONTIG
NONCONTIG, CONTIG = 5, 4


def family(name, L):
    """the unit repeated and cut to L nt; `GC+A`: one A at L//2 (a defect makes the ties partial), `GC+N5`: five N from L//3"""
    unit = name.split("+")[0]
    s = (unit * (L // len(unit) + 1))[:L]
    if name == "GC+A":
        s = s[:L // 2] + "A" + s[L // 2 + 1:]
    if name == "GC+N5":
        s = s[:L // 3] + "NNNNN" + s[L // 3 + 5:]
    assert len(s) == L
    return s


def fold_cases():
    """(family, L, reference fold() keywords, whether regions are recorded)"""
    base = dict(nb_mode=100, max_stack=20, max_branch=1000)
    todo = [(f, L, dict(base), True) for f in FAMILIES for L in LENGTHS]
    # few children per step: the cut of the beam falls inside groups of equal energy
    for f in ("CUG", "GGGAAACCC"):
        for ms, mb in ((1, 1000), (7, 7), (50, 3)):
            todo.append((f, 130, dict(nb_mode=100, max_stack=ms, max_branch=mb), ms == 7))
    todo.append(("CUG", 130, dict(base, gc_wei=1.0, au_wei=1.0, gu_wei=1.0), True))      # every pair type counts the same
    # min_hp=1: on the GC repeat the `>=` arg-max then ends on a hairpin too tight to be kept - nothing forms
    todo.append(("GC", 130, dict(base, min_hp=1), True))
    todo.append(("GGGAAACCC", 130, dict(base, min_hp=1), True))
    return todo


def long_cases():
    """(family, L, max_stack) of the oracle-made fixture: beyond what the reference's Python folds in minutes"""
    return [(f, L, 4) for f in ("GC", "CUG", "GGGGCCCC") for L in (1100, 1500)] + [("GC", 4200, 2)]


def one_case(args):
    fam, L, kw, record = args
    import make_golden as MG       # installs the stand-in RNA module, imports the reference
    R, U = MG.R, MG.U
    recs, left, calls = [], [NONCONTIG if record else 0, CONTIG if record else 0], [0]

    def rec_create_childs(upair, cur_str, gp):
        n = len(upair.pos_list)
        noncontig = any(upair.pos_list[i + 1] - upair.pos_list[i] != 1 for i in range(n - 1))
        take = n >= 2 and ((noncontig and left[0] > 0) or (not noncontig and left[1] > 0 and calls[0] % 3 == 0))
        calls[0] += 1
        if take:
            left[0 if noncontig else 1] -= 1
            cor_l = U.auto_cor(upair.forward, upair.backward)
            cs = sorted(cor_l, key=lambda el: el[1])
            ranked = cs[::-1][:gp.nb_mode]
            ws = [R.window_slide(upair.forward, upair.backward, pos, upair.pos_list, gp.min_hp) for pos, _ in ranked]
            sol = R.find_best_consecutives(cs, upair, cur_str, gp)
            recs.append(dict(
                family=fam, seq=gp.sequence, db=cur_str.str_struct, pos=list(map(int, upair.pos_list)),
                nb_mode=gp.nb_mode, min_hp=gp.min_hp, min_nrj=gp.min_nrj, gc=gp.gc_wei, au=gp.au_wei, gu=gp.gu_wei,
                cor=[float(c) for _, c in cor_l], lags=[int(p) for p, _ in ranked],
                ws=[[int(a), int(b), int(c), float(d)] for a, b, c, d in ws],
                sol=[[int(s[0]), float(s[1]), int(s[2]), int(s[3]), int(round(s[4] * 100))] for s in sol]))
        return MG._orig_create(upair, cur_str, gp)

    R.create_childs = rec_create_childs
    seq = family(fam, L)
    t0 = time.time()
    fin, traj = R.fold(seq, traj=True, **kw)
    print(f"[ties golden] {fam} L={L} {kw}: {len(traj)} steps, {len(recs)} records, {time.time() - t0:.0f} s", flush=True)
    case = dict(family=fam, seq=seq, params=kw,
                traj=[[[s.str_struct, int(round(float(s.energy) * 100))] for s in st] for st in traj])
    return case, recs


def one_long_case(args):
    fam, L, ms = args
    import oracle
    seq = family(fam, L)
    t0 = time.time()
    _, traj = oracle.fold(seq, 100, ms, 1000, traj=True)
    print(f"[ties golden] oracle {fam} L={L} max_stack={ms}: {len(traj)} steps, {time.time() - t0:.0f} s", flush=True)
    return dict(family=fam, seq=seq, params=dict(nb_mode=100, max_stack=ms, max_branch=1000),
                traj=[[[s.str_struct, s.dcal] for s in st] for st in traj])


def write(name, obj):
    p = os.path.join(GOLD, name)
    with gzip.GzipFile(p, "wb", mtime=0) as fh:
        fh.write(json.dumps(obj, separators=(",", ":")).encode())
    print(name, os.path.getsize(p), "bytes")


def main():
    import multiprocessing as mp
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(8, len(os.sched_getaffinity(0)))
    import oracle
    oracle.oracle.build()                  # once, before the workers race to build it
    with mp.get_context("fork").Pool(jobs) as pool:
        # (slowest first; the results come back in the order of the list whatever the order they finish in)
        longs = pool.map_async(one_long_case, long_cases(), chunksize=1)
        res = [] if "--only-long" in sys.argv else pool.map(one_case, fold_cases(), chunksize=1)
        longs = longs.get()
    write("fold_ties_long.json.gz", longs)
    if res:
        write("fold_traj_ties.json.gz", [c for c, _ in res])
        write("node_expand_ties.json.gz", [r for _, rr in res for r in rr])
        print(len(res), "fold cases;", sum(len(rr) for _, rr in res), "node records;", len(longs), "long oracle folds")


if __name__ == "__main__":
    main()
