"""Time rafft_amd's maximum-expected-accuracy structures (rafft_mea_batch) on the benchmark set, beside rafft_pf_batch on the same
set in the same process, and score the MEA rows, the centroids and the MFE rows against the known structures.  DESIGN.md section
17.  Needs the MI355X.
    python tools/mea_measure.py [--reps R] [--gamma G] [OUT.json]      (default profiles/mea_headline.json)
Workload: the 2296 benchmark sequences.  Every timed call ends with its rows and records on the host (the C call synchronises its
stream and copies them before it returns), so a host clock around it is a call time: one warm-up call of each, then R warm calls of
each, alternating, every repetition kept, the median reported.  Neither call copies the probabilities (probs=False).  Accuracy:
rafft_amd.scoring.score (PPV and sensitivity in per cent) of every row against its known structure, the mean over the set."""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "mea_headline.json"))
    args = ap.parse_args()
    from rafft_amd import mccaskill, scoring, zuker
    fields = [line.rstrip("\n").split("\t") for line in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    seqs, known = [f[1] for f in fields], [f[8] for f in fields]
    calls = dict(mea_batch=lambda: mccaskill.mea_batch_raw(seqs, args.gamma, probs=False), pf_batch=lambda: mccaskill.pf_batch_raw(seqs, probs=False))
    results = {name: call() for name, call in calls.items()}                       # warm-up; kept for the scores
    seconds = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            seconds[name].append(time.perf_counter() - t0)
    mea_rows, mea_recs = results["mea_batch"][0], results["mea_batch"][1]
    pf_rows, pf_recs = results["pf_batch"][0], results["pf_batch"][1]
    mfe_rows = [m.str_struct for m in zuker.mfe_batch(seqs)]
    assert not any(r["status"] for r in mea_recs) and not any(r["status"] for r in pf_recs)
    assert [r["energy"] for r in mea_recs] == [r["energy"] for r in pf_recs]

    def mean_scores(rows):
        sc = [scoring.score(r, k) for r, k in zip(rows, known)]
        return dict(ppv=statistics.fmean(x[0] for x in sc), sensitivity=statistics.fmean(x[1] for x in sc))
    out = dict(workload=f"{len(seqs)} benchmark sequences, {min(map(len, seqs))}-{max(map(len, seqs))} nt, one call each, probs not copied",
               gamma=args.gamma, reps=args.reps,
               seconds={name: v for name, v in seconds.items()},
               median_seconds={name: statistics.median(v) for name, v in seconds.items()},
               sequences_per_second={name: len(seqs) / statistics.median(v) for name, v in seconds.items()},
               mea_over_pf=statistics.median(seconds["mea_batch"]) / statistics.median(seconds["pf_batch"]),
               accuracy=dict(mea=mean_scores(mea_rows), centroid=mean_scores(pf_rows), mfe=mean_scores(mfe_rows)),
               mean_pairs=dict(mea=statistics.fmean(r.count("(") for r in mea_rows), centroid=statistics.fmean(r.count("(") for r in pf_rows),
                               mfe=statistics.fmean(r.count("(") for r in mfe_rows)),
               mean_diversity=statistics.fmean(r["diversity"] for r in mea_recs))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("median_seconds", "sequences_per_second", "mea_over_pf", "accuracy")}))


if __name__ == "__main__":
    main()
