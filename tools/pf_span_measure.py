"""Time rafft_amd's partition function under a base-pair span (rafft_pf_span_batch).  DESIGN.md section 19.  Needs the MI355X.
    python tools/pf_span_measure.py [--reps R] [--no-profile] [OUT.json]      (default profiles/pf_span_headline.json)
Every timed call ends with its results on the host (the C call synchronises its stream and copies them before it returns), so a
host clock around it is a call time: five warm calls of each shape, then R timed calls, every repetition kept, the median reported.
* the benchmark set at span 150 without probability buffers, beside rafft_mfe_span_batch on the same set in the same process,
  alternating (rafft_pf_span_batch runs rafft_mfe_span_batch itself first: its time is part of the first figure);
* one random 32 768-nt sequence (seed 32768) at spans 150 and 600, banded probabilities and unpaired read back: the share of pairs
  with P > 0.5, the statuses, the table bytes;
* for each of the two, how the kernel time splits into the inside diagonals, the exterior kernel, the outside diagonals and the
  probability kernel: the kernels' totals of ONE run of this script's own child (`--child SPAN`: a 9-nt call that loads the
  tables, then the long sequence once) under `rocprofv3 --kernel-trace --stats`, no counters - a profile of that run, not of the
  timed calls."""
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
WARM = 5
PHASES = (("pf_span_diag_kernel", "inside_diagonals"), ("pf_span_exterior_kernel", "exterior_sums"), ("pf_span_out_diag_kernel", "outside_diagonals"),
          ("pf_span_prob_kernel", "probabilities"), ("mfe_span_", "the_span_mfe_before_it"))


def long_sequence():
    import numpy as np
    return "".join(np.random.default_rng(32768).choice(list("ACGU"), 32768))


def kernel_profile(span):
    """the kernels' totals of one child run under rocprofv3 --kernel-trace --stats (None when rocprofv3 is not there)"""
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
                        v = ms.setdefault(phase, dict(launches=0, total_ms=0.0))
                        v["launches"] += int(row.get("Calls") or 0)
                        v["total_ms"] += float(row["TotalDurationNs"]) / 1e6
                        break
        total = sum(v["total_ms"] for v in ms.values())
        for v in ms.values():
            v["share"] = v["total_ms"] / total if total else None
        return dict(note="a 9-nt call, then the 32 768-nt sequence once, both counted; kernel time only, no gaps between launches", phases=ms,
                    kernel_ms_total=total)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "pf_span_headline.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import numpy as np
    import rafft_amd
    from rafft_amd import mccaskill, zuker
    big = long_sequence()
    if args.child:
        mccaskill.pf_span_batch_raw(["GGGAAACCC"], args.child)
        mccaskill.pf_span_batch_raw([big], args.child)
        return
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), reps=args.reps, warm_calls=WARM,
               clock="time.perf_counter around calls that end with their results on the host; five warm calls per shape first")
    calls = dict(pf_span_batch=lambda: mccaskill.pf_span_batch_raw(seqs, BENCH_SPAN, probs=False, unpaired=False),
                 mfe_span_batch=lambda: zuker.mfe_span_batch_raw(seqs, BENCH_SPAN))
    for _ in range(WARM):
        first = {name: call() for name, call in calls.items()}
    statuses = [r["status"] for r in first["pf_span_batch"][1]]
    secs = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            secs[name].append(time.perf_counter() - t0)
    lens = sorted(map(len, seqs))
    out["benchmark_set"] = dict(span=BENCH_SPAN, sequences=len(seqs), length=dict(min=lens[0], median=lens[len(lens) // 2], max=lens[-1]),
                                probability_buffers=False, seconds=secs, median_seconds={k: statistics.median(v) for k, v in secs.items()},
                                sequences_per_second={k: len(seqs) / statistics.median(v) for k, v in secs.items()},
                                statuses={str(k): statuses.count(k) for k in sorted(set(statuses))},
                                sequences_longer_than_the_span=sum(n > BENCH_SPAN for n in lens))
    out["one_sequence_of_32768_nt"] = {}
    for span in LONG_SPANS:
        for _ in range(WARM):
            rows, recs, probs, un = mccaskill.pf_span_batch_raw([big], span)
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            mccaskill.pf_span_batch_raw([big], span)
            t.append(time.perf_counter() - t0)
        P = probs[0]
        rec = dict(seconds=t, median_seconds=statistics.median(t), statuses=[r["status"] for r in recs], energy=recs[0]["energy"], mfe_dcal=recs[0]["mfe_dcal"],
                   centroid_pairs=recs[0]["n_pairs"], pairs_with_p_above_1e_5=int((P >= 1e-5).sum()), pairs_with_p_above_half=int((P > 0.5).sum()),
                   share_of_pairs_above_half=float((P > 0.5).sum() / max(1, (P >= 1e-5).sum())),
                   positions_in_a_pair_above_half=float(2 * (P > 0.5).sum() / len(big)), mean_unpaired=float(np.mean(un[0])),
                   table_bytes=6 * 32768 * span * 8, table_mib=6 * 32768 * span * 8 / 2 ** 20)
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
