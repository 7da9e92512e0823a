"""Time rafft_amd's partition function on the benchmark set and count the sequences whose scaled tables left the fp64 range.
DESIGN.md section 10.  Needs the MI355X.
    python tools/pf_measure.py [--reps R] [OUT.json]      (default profiles/pf_headline.json)
Every timed call ends with its results on the host (the C call synchronises its stream before it returns), so a host clock around
it is a call time.  pf_batch_raw is called without prob_out: the pass for the probabilities runs (the centroid needs it), the L x L
arrays are not copied.  One warm-up call, then R repetitions, all kept; the same for mfe_batch_raw on the same sequences, because the
MFE is part of every partition-function call (its energy gives the scale)."""
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


def summary(values, n_seq):
    import numpy as np
    med = float(np.median(values))
    return dict(seconds_median=med, seconds_all=[float(v) for v in values], sequences=n_seq, sequences_per_second_median=n_seq / med if med else None)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "pf_headline.json"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import _native as N, mccaskill, zuker
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    lens = np.array([len(s) for s in seqs])
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), n_seq=len(seqs), reps=args.reps, scale_factor=1.07,
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())),
               clock="time.perf_counter around calls that end with their results on the host; one warm-up call")
    out["pf_batch_without_prob_out"] = summary(timed(lambda: mccaskill.pf_batch_raw(seqs, probs=False), args.reps), len(seqs))
    out["mfe_batch_same_sequences"] = summary(timed(lambda: zuker.mfe_batch_raw(seqs), args.reps), len(seqs))
    rows, recs, _ = mccaskill.pf_batch_raw(seqs, probs=False)
    status = np.array([r["status"] for r in recs])
    cap = status == N.ERR_CAPACITY
    out["status_counts"] = {str(int(k)): int(v) for k, v in zip(*np.unique(status, return_counts=True))}
    out["capacity"] = dict(sequences=int(cap.sum()), lengths=sorted(int(x) for x in lens[cap]))
    ok = status == 0
    en = np.array([r["energy"] for r in recs])
    mfe = np.array([r["mfe_dcal"] / 100.0 for r in recs])
    freq = np.array([r["mfe_frequency"] for r in recs])
    out["ensemble"] = dict(energy_never_above_mfe=bool((en[ok] <= mfe[ok] + 1e-9).all()), mfe_frequency_median=float(np.median(freq[ok])) if ok.any() else None,
                           centroid_pairs_total=int(sum(r["n_pairs"] for r in recs)), longest_ok=int(lens[ok].max()) if ok.any() else None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
