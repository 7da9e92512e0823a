"""Timing of the accuracy scoring at the headline size: fold the 2296 benchmark sequences (n=100, ms=50,
synchronous fold_batch), then in the same process time that fold call, rafft_score_result on its result and the host path
(scoring.best_of over all beams).  Host clock around calls that end in a device synchronise; medians of warm calls.
usage: score_probe.py [--out profiles/score_headline.json] [--calls 7] [--no-host] [--kernel-stats rocprofv3_kernel_stats.csv]
       score_probe.py --kernels-only        (fold once, score three times: the run to put under rocprofv3 --kernel-trace --stats)"""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def bench_set():
    seqs, known = [], []
    with gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt") as fh:
        for line in fh:
            f = line.rstrip("\n").split("\t")
            seqs.append(f[1]); known.append(f[8])
    return seqs, known


def kernel_stats(path):
    """the score kernels' lines of rocprofv3's kernel_stats.csv, plus the busiest other kernel"""
    import csv
    rows = list(csv.DictReader(open(path)))
    pick = lambda r: {k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r}
    out = [pick(r) for r in rows if "score_" in r.get("Name", "")]
    rest = [r for r in rows if "score_" not in r.get("Name", "")]
    if rest:
        out.append(pick(max(rest, key=lambda r: float(r.get("TotalDurationNs", 0) or 0))))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_headline.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats")
    args = ap.parse_args()
    import rafft_amd
    from rafft_amd import _native as N
    from rafft_amd import scoring
    seqs, known = bench_set()
    lib = N.lib()
    fold = lambda: rafft_amd.fold_batch(seqs, 100, 50, 1000)
    res = fold()                                                    # cold: allocations, tables
    total = sum(len(b) for b in res)
    karr = (C.c_char_p * len(known))(*[k.encode() for k in known])
    row_out, seq_out = np.zeros(total, scoring._row_dtype()), np.zeros(len(seqs), scoring._seq_dtype())
    score = lambda r: N.check(lib.rafft_score_result(r._owner.res, karr, row_out.ctypes.data_as(C.c_void_p), seq_out.ctypes.data_as(C.c_void_p)))
    if args.kernels_only:
        for _ in range(3):
            score(res)
        return

    def timed(f):
        t = time.perf_counter()
        r = f()
        return (time.perf_counter() - t) * 1e3, r

    fold_ms = []
    for _ in range(args.calls):
        ms, res = timed(fold)
        fold_ms.append(ms)
    this_fold_ms = fold_ms[-1]                                      # the call that produced the beams scored below
    score(res)                                                      # cold: the scoring buffers
    score_ms = [timed(lambda: score(res))[0] for _ in range(args.calls)]
    py_ms = [timed(lambda: scoring.score_batch_gpu(res, known))[0] for _ in range(3)]
    out = dict(config=dict(n_seq=len(seqs), nb_mode=100, max_stack=50, max_branch=1000, rows=int(total), row_bytes=int(sum(len(s) * len(b) for s, b in zip(seqs, res)))),
               fold_ms=dict(median=statistics.median(fold_ms), min=min(fold_ms), scored_call=this_fold_ms, calls=fold_ms),
               score_result_ms=dict(median=statistics.median(score_ms), min=min(score_ms), calls=score_ms),
               score_batch_gpu_ms=dict(median=statistics.median(py_ms), calls=py_ms),
               version=lib.rafft_version().decode())
    out["score_over_fold"] = out["score_result_ms"]["median"] / out["fold_ms"]["median"]
    if not args.no_host:
        t = time.perf_counter()
        host = [scoring.best_of(beam, kn) for beam, kn in zip(res, known)]
        out["host_best_of_ms"] = (time.perf_counter() - t) * 1e3
        out["host_over_score"] = out["host_best_of_ms"] / out["score_result_ms"]["median"]
        got = scoring.score_batch_gpu(res, known)
        out["picks_equal_host"] = all(beam[int(k)].str_struct == h[2] for beam, k, h in zip(res, got["pick_ppv"], host))
    if args.kernel_stats:
        out["kernels"] = kernel_stats(args.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in out if k not in ("kernels",)}))
    if not out["score_result_ms"]["median"] < min(out["fold_ms"]["median"], this_fold_ms):
        raise SystemExit("scoring the final beams took longer than the fold that produced them")


if __name__ == "__main__":
    main()
