"""Time rafft_amd's MFE folds under a base-pair span (rafft_mfe_span_batch).  DESIGN.md section 18.  Needs the MI355X.
    python tools/mfe_span_measure.py [--reps R] [--no-profile] [OUT.json]      (default profiles/mfe_span_headline.json)
Every timed call ends with its rows on the host (the C call synchronises its stream and copies them before it returns), so a host
clock around it is a call time: one warm-up call of each shape, then R warm calls, every repetition kept, the median reported.
* the benchmark set at span 150, beside rafft_mfe_batch on the same set in the same process, alternating;
* one random 32 768-nt sequence (seed 32768) at spans 150 and 600;
* for each of the two, how the time splits into the diagonals, the exterior loop and the traceback: the kernels' totals of ONE run
  of this script's own child (`--child SPAN`: a 9-nt call that loads the tables, then the long sequence once) under
  `rocprofv3 --kernel-trace --stats` - a profile of that run, not of the timed calls."""
import argparse
import csv
import glob
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
BENCH_SPAN = 150
LONG_SPANS = (150, 600)
PHASES = (("mfe_span_diag_kernel", "diagonals"), ("mfe_span_exterior_kernel", "exterior_loop"), ("mfe_span_traceback_kernel", "traceback"))


def long_sequence():
    import numpy as np
    return "".join(np.random.default_rng(32768).choice(list("ACGU"), 32768))


def kernel_profile(span):
    """the span kernels' totals of one child run under rocprofv3 --kernel-trace --stats (None when rocprofv3 is not there)"""
    exe = next((p for p in ("/opt/rocm/bin/rocprofv3",) if os.path.exists(p)), None)
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                            "--child", str(span)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return dict(error=(r.stderr or r.stdout)[-400:])
        ms = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for kernel, phase in PHASES:
                    if kernel in row.get("Name", ""):
                        ms[phase] = dict(launches=int(row.get("Calls") or 0), total_ms=float(row["TotalDurationNs"]) / 1e6)
        total = sum(v["total_ms"] for v in ms.values())
        for v in ms.values():
            v["share"] = v["total_ms"] / total if total else None
        return dict(note="a 9-nt call, then the 32 768-nt sequence once, both counted; kernel time only, no gaps between launches", phases=ms,
                    kernel_ms_total=total)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "mfe_span_headline.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import zuker
    big = long_sequence()
    if args.child:
        zuker.mfe_span_batch_raw(["GGGAAACCC"], args.child)
        zuker.mfe_span_batch_raw([big], args.child)
        return
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), reps=args.reps,
               clock="time.perf_counter around calls that end with their rows on the host; one warm-up call per shape")
    calls = dict(mfe_span_batch=lambda: zuker.mfe_span_batch_raw(seqs, BENCH_SPAN), mfe_batch=lambda: zuker.mfe_batch_raw(seqs))
    first = {name: call() for name, call in calls.items()}
    assert not any(first["mfe_span_batch"][3]) and not any(first["mfe_batch"][3])
    secs = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            secs[name].append(time.perf_counter() - t0)
    lens = sorted(map(len, seqs))
    out["benchmark_set"] = dict(span=BENCH_SPAN, sequences=len(seqs), length=dict(min=lens[0], median=lens[len(lens) // 2], max=lens[-1]),
                                seconds=secs, median_seconds={k: statistics.median(v) for k, v in secs.items()},
                                sequences_per_second={k: len(seqs) / statistics.median(v) for k, v in secs.items()},
                                sequences_longer_than_the_span=sum(n > BENCH_SPAN for n in lens),
                                sequences_whose_energy_the_span_raises=sum(a > b for a, b in zip(first["mfe_span_batch"][1], first["mfe_batch"][1])),
                                energies_below_mfe_batch=sum(a < b for a, b in zip(first["mfe_span_batch"][1], first["mfe_batch"][1])))
    out["one_sequence_of_32768_nt"] = {}
    for span in LONG_SPANS:
        rows, dcal, n_pairs, status = zuker.mfe_span_batch_raw([big], span)
        assert status == [0]
        back, st = rafft_amd.eval_structures([big], rows)
        assert st[0] == 0 and back[0] == dcal[0]
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            zuker.mfe_span_batch_raw([big], span)
            t.append(time.perf_counter() - t0)
        rec = dict(seconds=t, median_seconds=statistics.median(t), dcal=dcal[0], n_pairs=n_pairs[0], table_mib=4 * 32768 * span * 4 / 2 ** 20)
        if not args.no_profile:
            rec["kernel_profile"] = kernel_profile(span)
        out["one_sequence_of_32768_nt"][f"span_{span}"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
