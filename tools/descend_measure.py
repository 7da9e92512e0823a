"""Time rafft_amd's gradient walks (rafft_descend_batch) on the benchmark set.  DESIGN.md section 14.  Needs the MI355X.
    python tools/descend_measure.py [--reps R] [--samples N] [--no-profile] [OUT.json]      (default profiles/descend_headline.json)
Workload: the 2296 benchmark sequences, starts = N = 1000 structures per sequence drawn by sample_batch (seed 1), handed over as the
arrays sample_batch_raw returns (stride L + 1), no move buffers.  Every timed call ends with its rows on the host (the C call
synchronises its stream and copies them before it returns), so a host clock around it is a call time: one warm-up call, then R warm
calls, all kept, the median reported.  Beside the time: steps per walk, distinct minima per sequence, the share of samples whose
basin is the basin of the MFE row, the share of the final beam of the fold (n = 100, ms = 50) that are minima, the same call on the
sequences of each length class alone (what the longest cost), and the kernel's total from ONE run of this script's own child
(`--child`: one warm-up call and one call) under `rocprofv3 --kernel-trace --stats` - a profile of that run, not of the timed calls."""
import argparse
import csv
import ctypes
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
CLASSES = ((0, 100), (100, 200), (200, 500), (500, 1000), (1000, 4097))


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def quantiles(v):
    import numpy as np
    v = np.asarray(v, dtype=np.float64)
    return dict(min=float(v.min()), q25=float(np.percentile(v, 25)), median=float(np.median(v)), q75=float(np.percentile(v, 75)),
                q99=float(np.percentile(v, 99)), max=float(v.max()), mean=float(v.mean()))


def kernel_profile(n_samples):
    """the kernel's totals of one child run under rocprofv3 --kernel-trace --stats (None when rocprofv3 is not there)"""
    exe = next((p for p in ("/opt/rocm/bin/rocprofv3",) if os.path.exists(p)), None)
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                            "--child", "--samples", str(n_samples)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(error=(r.stderr or r.stdout)[-400:])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "descend" in name:
                    rows.append(dict(kernel=name.split("(")[0].replace("void ", ""), calls=int(row.get("Calls") or 0),
                                     total_ms=float(row["TotalDurationNs"]) / 1e6, average_ms=float(row.get("AverageNs") or 0.0) / 1e6,
                                     max_ms=float(row.get("MaxNs") or 0.0) / 1e6))
        return dict(note="one warm-up call and one call, both counted; a launch is a chunk of the call", kernels=rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "descend_headline.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import _native as N, descend as D, mccaskill, zuker
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    srec, rows, _ = mccaskill.sample_batch_raw(seqs, args.samples, 1)
    keep = [k for k, r in enumerate(srec) if r["status"] == 0]
    seqs, rows = [seqs[k] for k in keep], [rows[k] for k in keep]
    say(f"{len(seqs)} sequences sampled")
    call = lambda s, r: D.descend_batch_raw(s, r, moves=False)
    if args.child:
        for _ in range(2):
            call(seqs, rows)
        return
    lens = np.array([len(s) for s in seqs])
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), n_sequences=len(seqs), samples_per_sequence=args.samples,
               walks=len(seqs) * args.samples, reps=args.reps, workload="benchmark set; starts = sample_batch rows (seed 1), no move buffers, max_steps 0",
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())),
               clock="time.perf_counter around calls that end with their rows on the host; one warm-up call")
    t0 = time.perf_counter()
    call(seqs, rows)
    say(f"warm-up call: {time.perf_counter() - t0:.2f} s")
    secs = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        _, rrec, ends, _ = call(seqs, rows)
        secs.append(time.perf_counter() - t0)
        say(f"call: {secs[-1]:.2f} s")
    c = (ctypes.c_longlong * 4)()
    N.check(N.lib().rafft_descend_counters(ctypes.byref(c)))
    steps = np.concatenate([r["n_steps"] for r in rrec])
    status = np.concatenate([r["status"] for r in rrec])
    out.update(seconds_median=float(np.median(secs)), seconds_all=[float(v) for v in secs], walks_per_second_median=len(steps) / float(np.median(secs)),
               counters=dict(zip(("chunks", "launches", "walks_run", "steps"), (int(v) for v in c))),
               walks_stopped_by_the_bound=int((status == N.ERR_CAPACITY).sum()), steps_per_walk=quantiles(steps),
               starts_that_are_minima=float((steps == 0).mean()))
    # basins
    _, mrec, mends, _ = call(seqs, [[m.str_struct] for m in zuker.mfe_batch(seqs)])
    n_min, share = [], []
    for s in range(len(seqs)):
        uniq = np.unique(ends[s], axis=0)
        n_min.append(len(uniq))
        share.append(float((ends[s] == mends[s][0][None, :]).all(axis=1).mean()))
    out["distinct_minima_per_sequence"] = quantiles(n_min)
    out["share_of_samples_in_the_basin_of_the_mfe_row"] = dict(over_all_samples=float(np.mean(share)), per_sequence=quantiles(share))
    out["mfe_rows_that_are_minima"] = float(np.mean([int(r["n_steps"][0]) == 0 for r in mrec]))
    say("basins done")
    # the final beam of the fold
    folds = rafft_amd.fold_batch(seqs, nb_mode=100, max_stack=50, max_branch=1000)
    _, frec, _, _ = call(seqs, [[x.str_struct for x in f] for f in folds])
    fsteps = np.concatenate([r["n_steps"] for r in frec])
    out["final_beam_n100_ms50"] = dict(structures=int(len(fsteps)), share_that_are_minima=float((fsteps == 0).mean()), steps=quantiles(fsteps))
    say("final beams done")
    # what each length class costs: the same call on its sequences alone
    out["by_length"] = []
    for lo, hi in CLASSES:
        pick = [k for k in range(len(seqs)) if lo < len(seqs[k]) <= hi]
        if not pick:
            continue
        sub_s, sub_r = [seqs[k] for k in pick], [rows[k] for k in pick]
        call(sub_s, sub_r)
        t0 = time.perf_counter()
        _, r2, _, _ = call(sub_s, sub_r)
        dt = time.perf_counter() - t0
        st = np.concatenate([r["n_steps"] for r in r2])
        out["by_length"].append(dict(length_above=lo, up_to=hi, sequences=len(pick), walks=int(len(st)), seconds=dt, steps_median=float(np.median(st)), steps_max=int(st.max())))
        say(f"lengths {lo}-{hi}: {len(pick)} sequences, {dt:.2f} s")
    if not args.no_profile:
        out["kernel_profile"] = kernel_profile(args.samples)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
