"""Time rafft_amd's enumeration of the structures within an energy band on the benchmark set.  DESIGN.md section 12.  Needs the MI355X.
    python tools/subopt_measure.py [--reps R] [--delta KCAL] [--max-structs N] [OUT.json]
    (default profiles/subopt_headline.json, delta = 1 kcal/mol, N = 100 000)
Every timed call ends with its rows on the host (the C call synchronises its stream and copies the rows before it returns), so a
host clock around it is a call time.  One warm-up call, then R repetitions, all kept.  The split between filling the tables and
enumerating, the levels and the launches are the library's own counters of each call (rafft_subopt_counters): host clocks around the
two parts of every chunk, each ending with a synchronise."""
import argparse
import ctypes
import gzip
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

COUNTERS = ("levels_of_the_deepest_sequence", "enumeration_launches", "fill_launches", "chunks", "sequences_over_capacity", "fill_us", "enumerate_us")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "subopt_headline.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--delta", type=float, default=1.0)
    ap.add_argument("--max-structs", type=int, default=100000)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import _native as N, wuchty
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    lens = np.array([len(s) for s in seqs])
    delta_dcal = int(round(args.delta * 100))

    def call():
        t0 = time.perf_counter()
        recs, rows, dcal = wuchty.subopt_batch_raw(seqs, delta_dcal, args.max_structs)
        dt = time.perf_counter() - t0
        c = (ctypes.c_longlong * 7)()
        N.check(N.lib().rafft_subopt_counters(ctypes.byref(c)))
        return dt, recs, dict(zip(COUNTERS, (int(v) for v in c)))

    call()                                  # warm-up: tables uploaded, kernels loaded
    runs = [call() for _ in range(args.reps)]
    recs = runs[-1][1]
    status = np.array([r["status"] for r in recs])
    n_structs = np.array([r["n_structs"] for r in recs], dtype=np.int64)
    secs = [r[0] for r in runs]
    med = float(np.median(secs))
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), n_seq=len(seqs), reps=args.reps, delta_kcal=args.delta,
               max_structs=args.max_structs,
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())),
               clock="time.perf_counter around calls that end with their rows on the host (the copy into numpy arrays included); one warm-up call",
               subopt_batch=dict(seconds_median=med, seconds_all=[float(v) for v in secs], structures=int(n_structs.sum()),
                                 structures_per_second_median=int(n_structs.sum()) / med if med else None),
               counters_all=[r[2] for r in runs],
               sequences_ok=int((status == 0).sum()), sequences_over_capacity=int((status == N.ERR_CAPACITY).sum()),
               structures_per_sequence=dict(median=float(np.median(n_structs[status == 0])), max=int(n_structs.max())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
