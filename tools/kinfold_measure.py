"""Time rafft_amd's stochastic folding trajectories (rafft_kinfold_batch) on the benchmark set.  DESIGN.md section 16.  Needs the MI355X.
    python tools/kinfold_measure.py [--traj N] [--tmax T] [--max-steps M] [--max-len L] [--long-len L2] [--reps R] [--no-profile] [OUT.json]
                                                                                            (default profiles/kinfold_headline.json)
Workload: the benchmark sequences up to L = 200 nt, N = 1000 trajectories each from the open chain, the MFE row of mfe_batch the
stop row (`--stop mfe`), seed 1, t_max = T, at most M steps a trajectory (one the bound ends is counted as such, not as arrived), no
logs, no sample times.  Every timed call ends with its records on the host, so a host clock around it is a call time: one warm-up
call, then R warm calls, all kept, the median reported.  Beside the time: steps per second, steps per trajectory (median, 99th
percentile, maximum), the share arrived, ended by t_max and ended by the bound, the same call on the sequences of each length
class alone, one long sequence (the longest of the whole set up to --long-len = 600 nt, 64 trajectories of at most 16 steps from the
open chain: what a step costs there - from the open chain it grows with the cube of the length, section 16), and
the kernel's total from ONE run of this script's own child (`--child`: one warm-up call and one call) under
`rocprofv3 --kernel-trace --stats` - a profile of that run, not of the timed calls."""
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
CLASSES = ((0, 50), (50, 100), (100, 150), (150, 200))


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_profile(argv):
    """the kernel's totals of one child run under rocprofv3 --kernel-trace --stats (None when rocprofv3 is not there)"""
    exe = next((p for p in ("/opt/rocm/bin/rocprofv3",) if os.path.exists(p)), None)
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                            "--child"] + argv, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(error=(r.stderr or r.stdout)[-400:])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "kinfold" in name:
                    rows.append(dict(kernel=name.split("(")[0].replace("void ", ""), calls=int(row.get("Calls") or 0),
                                     total_ms=float(row["TotalDurationNs"]) / 1e6, average_ms=float(row.get("AverageNs") or 0.0) / 1e6,
                                     max_ms=float(row.get("MaxNs") or 0.0) / 1e6))
        return dict(note="one warm-up call and one call, both counted; a launch is a chunk of the call", kernels=rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "kinfold_headline.json"))
    ap.add_argument("--traj", type=int, default=1000)
    ap.add_argument("--tmax", type=float, default=20.0)
    ap.add_argument("--max-steps", type=int, default=4096)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--long-len", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import _native as N, kinfold as K, zuker
    every = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    seqs = [s for s in every if len(s) <= args.max_len]
    mfe = zuker.mfe_batch(seqs, raise_errors=False)
    keep = [k for k, m in enumerate(mfe) if m is not None]
    seqs, stops = [seqs[k] for k in keep], [[mfe[k].str_struct] for k in keep]
    say(f"{len(seqs)} sequences up to {args.max_len} nt")

    def call(s, w, n=args.traj, t_max=args.tmax, max_steps=args.max_steps):
        return K.kinfold_batch_raw(s, [None] * len(s), t_max, n_rep=n, watch=w, n_stop=1 if w else None, seeds=1, max_steps=max_steps)[1]

    def summary(trec, secs):
        t = np.concatenate(trec)
        steps, flags = t["n_steps"], t["flags"]
        return dict(trajectories=int(len(t)), seconds=secs, steps=int(steps.sum()), steps_per_second=float(steps.sum() / secs),
                    steps_per_trajectory=dict(median=float(np.median(steps)), q99=float(np.percentile(steps, 99)), max=int(steps.max()), mean=float(steps.mean())),
                    share_arrived=float(((flags & N.KF_STOP) != 0).mean()), share_ended_by_t_max=float(((flags & N.KF_TIME) != 0).mean()),
                    share_ended_by_the_bound=float(((flags & N.KF_MORE) != 0).mean()), share_absorbed=float(((flags & N.KF_ABSORBED) != 0).mean()))

    if args.child:
        for _ in range(2):
            call(seqs, stops)
        return
    lens = np.array([len(s) for s in seqs])
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), n_sequences=len(seqs), trajectories_per_sequence=args.traj,
               t_max=args.tmax, max_steps=args.max_steps, reps=args.reps,
               workload="benchmark sequences up to max_len; open chain, stop row = MFE row, seed 1, no logs, no sample times",
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())),
               clock="time.perf_counter around calls that end with their records on the host; one warm-up call")
    t0 = time.perf_counter()
    call(seqs, stops)
    say(f"warm-up call: {time.perf_counter() - t0:.2f} s")
    secs = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        trec = call(seqs, stops)
        secs.append(time.perf_counter() - t0)
        say(f"call: {secs[-1]:.2f} s")
    c = (ctypes.c_longlong * 4)()
    N.check(N.lib().rafft_kinfold_counters(ctypes.byref(c)))
    out.update(summary(trec, float(np.median(secs))), seconds_all=[float(v) for v in secs],
               counters=dict(zip(("chunks", "launches", "trajectories_run", "steps"), (int(v) for v in c))))
    out["by_length"] = []
    for lo, hi in CLASSES:
        pick = [k for k in range(len(seqs)) if lo < len(seqs[k]) <= hi]
        if not pick:
            continue
        sub_s, sub_w = [seqs[k] for k in pick], [stops[k] for k in pick]
        call(sub_s, sub_w)
        t0 = time.perf_counter()
        t2 = call(sub_s, sub_w)
        out["by_length"].append(dict(length_above=lo, up_to=hi, sequences=len(pick), **summary(t2, time.perf_counter() - t0)))
        say(f"lengths {lo}-{hi}: {len(pick)} sequences, {out['by_length'][-1]['seconds']:.2f} s")
    # the long-sequence cost: 64 trajectories of at most 16 steps from the open chain of the longest sequence up to --long-len
    longest = max((s for s in every if len(s) <= args.long_len), key=len)
    call([longest], None, 64, 1e9, 16)
    t0 = time.perf_counter()
    t3 = call([longest], None, 64, 1e9, 16)
    out["long_sequence"] = dict(length=len(longest), max_steps=16, **summary(t3, time.perf_counter() - t0))
    say(f"long sequence ({len(longest)} nt): {out['long_sequence']['seconds']:.2f} s")
    if not args.no_profile:
        out["kernel_profile"] = kernel_profile(["--traj", str(args.traj), "--tmax", repr(args.tmax), "--max-steps", str(args.max_steps), "--max-len", str(args.max_len)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
