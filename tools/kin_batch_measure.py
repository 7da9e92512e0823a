"""Time rafft_kin.kinetics_batch on the trajectories of the benchmark set (n=100, ms=50, -mt 30 -ns 100) against the per-graph route,
a loop of kinetics_gpu(method="implicit"), on a fixed 50-sequence sample of it.  Needs the MI355X.
    python tools/kin_batch_measure.py [--reps R] [--skip-all] [OUT.json]      (default profiles/kin_batch_headline.json)
Every timed call ends with its results on the host (the C call synchronises its stream before it returns; the per-graph route ends
in host arrays), so a host clock around it is a call time.  Each route is warmed up on the shapes it is timed on; on the sample
the two routes alternate, R times each, and every repetition is kept so the spread can be read next to the median."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

MAX_TIME, N_STEPS, N_MODE, MAX_STACK, N_SAMPLE = 30, 100, 100, 50, 50


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def summary(values):
    import numpy as np
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)), all=[float(v) for v in values])


def states(results):
    import numpy as np
    S = [len(r[2]) for r in results if r is not None]
    return dict(min=min(S), median=float(np.median(S)), max=max(S), over_128=sum(s > 128 for s in S), graphs=len(S))


def text_graphs(batch, n):
    """the graphs of a traj BatchResult as fast_paths with the one-decimal energies of the text format: what the per-graph route gets"""
    from rafft_amd.utils import Structure, text_energy
    return [[[Structure(st.str_struct, st.dcal, text_energy(st.energy)) for st in step] for step in batch[k][1]] for k in range(n)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "kin_batch_headline.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-all", action="store_true", help="only the 50-sequence sample, not the whole set")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import rafft_kin
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    sample = list(range(0, len(seqs), len(seqs) // N_SAMPLE))[:N_SAMPLE]
    out = dict(device=torch.cuda.get_device_name(0), n_seq=len(seqs), n_mode=N_MODE, max_stack=MAX_STACK, max_time=MAX_TIME, n_steps=N_STEPS,
               sample=sample, reps=args.reps, clock="time.perf_counter around calls that end with their results on the host")
    sub = rafft_amd.fold_batch([seqs[i] for i in sample], N_MODE, MAX_STACK, traj=True)
    graphs = text_graphs(sub, len(sample))
    batch = lambda: rafft_kin.kinetics_batch(sub, MAX_TIME, N_STEPS)
    loop = lambda: [rafft_kin.kinetics_gpu(g, MAX_TIME, N_STEPS, method="implicit") for g in graphs]
    out["sample_batch_first_call_s"], res = timed(batch)                      # warm-up, both routes, on the timed shapes
    out["sample_loop_first_call_s"], base = timed(loop)
    out["sample_states"] = states(res)
    d = [np.abs(np.array(a[0]) - np.array(b[0])) for a, b in zip(res, base)]
    early = int(0.6 * N_STEPS) + 1
    out["sample_batch_vs_loop_max_abs"] = dict(first_60_percent=float(max(x[:early].max() for x in d)), everywhere=float(max(x.max() for x in d)))
    tb, tl = [], []
    for _ in range(args.reps):
        tb.append(timed(batch)[0])
        tl.append(timed(loop)[0])
    out["sample_batch_s"], out["sample_loop_s"] = summary(tb), summary(tl)
    out["sample_speedup_of_medians"] = out["sample_loop_s"]["median"] / out["sample_batch_s"]["median"]
    print(json.dumps(out), flush=True)
    if not args.skip_all:
        out["fold_all_traj_s"], folded = timed(lambda: rafft_amd.fold_batch(seqs, N_MODE, MAX_STACK, traj=True))
        whole = lambda: rafft_kin.kinetics_batch(folded, MAX_TIME, N_STEPS)
        out["all_batch_first_call_s"], res = timed(whole)
        out["all_states"] = states(res)
        out["all_batch_s"] = summary([timed(whole)[0] for _ in range(args.reps)])
        print(json.dumps({k: out[k] for k in ("fold_all_traj_s", "all_batch_first_call_s", "all_states", "all_batch_s")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
