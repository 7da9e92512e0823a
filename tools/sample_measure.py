"""Time rafft_amd's sampling from the ensemble on the benchmark set.  DESIGN.md section 11.  Needs the MI355X.
    python tools/sample_measure.py [--reps R] [--samples N] [OUT.json]      (default profiles/sample_headline.json, N = 1000)
Every timed call ends with its results on the host (the C call synchronises its stream before it returns and copies the rows into
the caller's arrays), so a host clock around it is a call time.  One warm-up call, then R repetitions, all kept.  The inside pass
beside it is the same call with n_samples = 0: the MFE, the inside tables and the exterior sums, no traceback and no rows."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()                                   # warm-up: tables uploaded, kernels loaded
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "sample_headline.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1000)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import mccaskill
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    lens = np.array([len(s) for s in seqs])
    n = args.samples
    t_all = timed(lambda: mccaskill.sample_batch_raw(seqs, n, seeds=1), args.reps)
    t_inside = timed(lambda: mccaskill.sample_batch_raw(seqs, 0), args.reps)
    recs, rows, dcal = mccaskill.sample_batch_raw(seqs, n, seeds=1)
    ok = np.array([r["status"] == 0 for r in recs])
    med, med_in = float(np.median(t_all)), float(np.median(t_inside))
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), n_seq=len(seqs), reps=args.reps, samples_per_sequence=n,
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())),
               clock="time.perf_counter around calls that end with their rows on the host; one warm-up call",
               sample_batch=dict(seconds_median=med, seconds_all=[float(v) for v in t_all], samples=int(ok.sum()) * n,
                                 samples_per_second_median=int(ok.sum()) * n / med if med else None, row_bytes=int(sum(r.nbytes for r in rows))),
               inside_pass_n_samples_0=dict(seconds_median=med_in, seconds_all=[float(v) for v in t_inside]),
               traceback_and_copies_seconds_median=med - med_in,
               sequences_ok=int(ok.sum()), lowest_sample_never_below_mfe=bool(all(d.min() >= r["mfe_dcal"] for d, r, o in zip(dcal, recs, ok) if o)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
