"""Time rafft_amd's folding barriers (rafft_findpath_batch) on the benchmark set.  DESIGN.md section 13.  Needs the MI355X.
    python tools/findpath_measure.py [--reps R] [--graphs G] [--no-profile] [OUT.json]      (default profiles/findpath_headline.json)
Workload: the 2296 benchmark sequences, A = the best structure of the final beam of the fold (n = 100, ms = 50), B = the row of
mfe_batch, at widths 16 and 64.  Every timed call ends with its paths on the host (the C call synchronises its stream and copies
them before it returns), so a host clock around it is a call time: one warm-up call, then R warm calls, all kept, the median
reported.  Per-kernel times come from ONE run of this script's own child (`--child W`: one warm-up call and one call at width W)
under `rocprofv3 --kernel-trace --stats`; they are a profile of that run, not of the timed calls.  Beside the times: the
distribution of d and of the barrier heights, the share of problems whose saddle differs between the two widths, the time of the
tests' Python mirror on a 50-problem sample on the CPU (context only), and - on the edges of the fast-folding graphs of the first G
sequences of the same fold (width 16, both directions) - the excess of the saddle over max(E_i, E_j), which says whether
`rafft_kin --barriers` matters."""
import argparse
import csv
import glob
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
WIDTHS = (16, 64)


def workload():
    import rafft_amd
    from rafft_amd import zuker
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    folds = rafft_amd.fold_batch(seqs, nb_mode=100, max_stack=50, max_branch=1000, traj=True)
    starts = [min(final, key=lambda x: x.dcal).str_struct for final, _ in folds]
    ends = [m.str_struct for m in zuker.mfe_batch(seqs)]
    return seqs, starts, ends, folds


def quantiles(v):
    import numpy as np
    v = np.asarray(v, dtype=np.float64)
    return dict(min=float(v.min()), q25=float(np.percentile(v, 25)), median=float(np.median(v)), q75=float(np.percentile(v, 75)),
                q99=float(np.percentile(v, 99)), max=float(v.max()), mean=float(v.mean()))


def graph_edges(traj):
    """(parent row, child row) of a fast-folding graph: a structure of step k - 1 whose pairs are all pairs of a structure of step k"""
    import numpy as np
    from rafft_amd.rafft_kin import _pair_table
    edges = set()
    tabs = [np.stack([_pair_table(s.str_struct) for s in step]) for step in traj]
    for k in range(1, len(traj)):
        for ci, st in enumerate(traj[k]):
            for pi in np.nonzero(((tabs[k - 1] == -1) | (tabs[k - 1] == tabs[k][ci][None, :])).all(axis=1))[0]:
                a, b = traj[k - 1][int(pi)].str_struct, st.str_struct
                if a != b:
                    edges.add((a, b))
    return sorted(edges)


def kernel_profile(width):
    """per-kernel totals of one child run under rocprofv3 --kernel-trace --stats (None when rocprofv3 is not there)"""
    exe = next((p for p in ("/opt/rocm/bin/rocprofv3",) if os.path.exists(p)), None)
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__), "--child", str(width)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(error=(r.stderr or r.stdout)[-400:])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "findpath" in name:
                    rows.append(dict(kernel=name.split("(")[0].replace("void ", ""), calls=int(row.get("Calls") or 0),
                                     total_ms=float(row["TotalDurationNs"]) / 1e6, average_us=float(row.get("AverageNs") or 0.0) / 1e3))
        return dict(width=width, note="one warm-up call and one call, both counted", kernels=sorted(rows, key=lambda x: -x["total_ms"]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "findpath_headline.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--graphs", type=int, default=100)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import _native as N, findpath as F
    seqs, starts, ends, folds = workload()
    if args.child:
        for _ in range(2):
            F.findpath_batch_raw(seqs, starts, ends, args.child)
        return
    lens = np.array([len(s) for s in seqs])
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), n_problems=len(seqs), reps=args.reps,
               workload="benchmark set; A = best of the final beam (n = 100, ms = 50), B = the mfe_batch row",
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())),
               clock="time.perf_counter around calls that end with their paths on the host; one warm-up call per width", widths={})
    saddles = {}
    for w in WIDTHS:
        F.findpath_batch_raw(seqs, starts, ends, w)
        secs = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            recs, moves, dcal = F.findpath_batch_raw(seqs, starts, ends, w)
            secs.append(time.perf_counter() - t0)
        import ctypes
        c = (ctypes.c_longlong * 4)()
        N.check(N.lib().rafft_findpath_counters(ctypes.byref(c)))
        status = np.array([r["status"] for r in recs])
        ok = status == 0
        d = np.array([r["dist"] for r in recs])[ok]
        barrier = np.array([(r["saddle_dcal"] - r["start_dcal"]) / 100.0 for r in recs])[ok]
        saddles[w] = np.where(ok, np.array([r["saddle_dcal"] for r in recs]), -10 ** 9)
        out["widths"][str(w)] = dict(seconds_median=float(np.median(secs)), seconds_all=[float(v) for v in secs],
                                     problems_per_second_median=len(seqs) / float(np.median(secs)),
                                     counters=dict(zip(("chunks", "levels", "launches", "problems_run"), (int(v) for v in c))),
                                     problems_ok=int(ok.sum()), problems_over_capacity=int((status == N.ERR_CAPACITY).sum()),
                                     d=quantiles(d), problems_with_d_0=int((d == 0).sum()), barrier_kcal=quantiles(barrier),
                                     problems_with_a_barrier=int((barrier > 0).sum()))
    both_ok = (saddles[16] > -10 ** 9) & (saddles[64] > -10 ** 9)
    out["share_of_problems_whose_saddle_differs_between_widths"] = float((saddles[16] != saddles[64])[both_ok].mean())
    out["share_of_problems_where_width_64_is_lower"] = float((saddles[64] < saddles[16])[both_ok].mean())
    # the tests' mirror on the CPU, as context
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _findpath_np as FP
    rng = np.random.default_rng(5)
    recs16, _, _ = F.findpath_batch_raw(seqs, starts, ends, 16)
    small = [k for k, r in enumerate(recs16) if r["status"] == 0 and 1 <= r["dist"] <= 40]
    sample = [int(k) for k in rng.choice(small, min(50, len(small)), replace=False)]
    t0 = time.perf_counter()
    agree = sum(FP.search(seqs[k], starts[k], ends[k], 16)["saddle_dcal"] == recs16[k]["saddle_dcal"] for k in sample)
    out["cpu_mirror"] = dict(problems=len(sample), width=16, d_at_most=40, seconds=time.perf_counter() - t0, saddles_equal_to_the_gpu=int(agree),
                             note="tests/_findpath_np.search over whole-structure oracle energies, one Python process: context only")
    # the edges of the fast-folding graphs
    es, ea, eb = [], [], []
    for k in range(min(args.graphs, len(seqs))):
        for a, b in graph_edges(folds[k][1]):
            es.append(seqs[k]); ea.append(a); eb.append(b)
    t0 = time.perf_counter()
    erecs, _, _ = F.findpath_batch(es, ea, eb, width=16, both=True)
    dt = time.perf_counter() - t0
    excess = np.array([(r["saddle_dcal"] - max(r["start_dcal"], r["end_dcal"])) / 100.0 for r in erecs])
    out["graph_edges"] = dict(graphs=min(args.graphs, len(seqs)), edges=len(es), width=16, both=True, seconds=dt, d=quantiles([r["dist"] for r in erecs]),
                              excess_kcal=quantiles(excess), share_of_edges_with_excess=float((excess > 0).mean()),
                              median_rate_factor_at_kt_0_61=float(np.median(np.exp(-excess / 0.61))))
    if not args.no_profile:
        out["kernel_profile"] = kernel_profile(16)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
