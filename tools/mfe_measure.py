"""Time rafft_amd.mfe_batch on the benchmark set and compare its energies with the published ViennaRNA MFE rows
(tests/golden/mfe_published.tsv.gz: the benchmark sequences of at most 120 nt).  DESIGN.md section 9.  Needs the MI355X.
    python tools/mfe_measure.py [--reps R] [OUT.json]      (default profiles/mfe_headline.json)
Every timed call ends with its results on the host (the C call synchronises its stream before it returns), so a host clock around
it is a call time.  One warm-up call per shape, then R repetitions, all kept.  Time per class: the sequences of each class in a
call of their own (those up to the LDS bound; the longer ones, which go through device memory), and the LDS-class sequences forced
through the device-memory class for comparison."""
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
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "mfe_headline.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import _native as N, zuker
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    lc = N.lib().rafft_mfe_lds_len()
    short, long_ = [s for s in seqs if len(s) <= lc], [s for s in seqs if len(s) > lc]
    lens = np.array([len(s) for s in seqs])
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), n_seq=len(seqs), lds_len=lc, reps=args.reps,
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())),
               clock="time.perf_counter around calls that end with their results on the host; one warm-up call per shape")
    out["whole_set"] = summary(timed(lambda: zuker.mfe_batch_raw(seqs), args.reps), len(seqs))
    out["lds_class"] = summary(timed(lambda: zuker.mfe_batch_raw(short), args.reps), len(short))
    if long_:
        out["hbm_class"] = summary(timed(lambda: zuker.mfe_batch_raw(long_), args.reps), len(long_))
    out["lds_class_sequences_through_hbm_class"] = summary(timed(lambda: zuker.mfe_batch_raw(short, max_lds_len=4), max(1, args.reps // 2)), len(short))
    # agreement with the published rows
    pub = [l.split() for l in gzip.open(os.path.join(ROOT, "tests", "golden", "mfe_published.tsv.gz"), "rt")]
    ps, pdb, pe = [r[0] for r in pub], [r[1] for r in pub], [int(r[2]) for r in pub]
    rows, dcal, _, status = zuker.mfe_batch_raw(ps)
    assert not any(status)
    own_of_pub, st, _ = rafft_amd.eval_structures_info(ps, pdb)               # the published structure under our tables
    _, _, guessed = rafft_amd.eval_structures_info(ps, rows)
    lower = [dict(index=k, length=len(ps[k]), ours=dcal[k], published=pe[k], published_structure_under_our_tables=own_of_pub[k] if not st[k] else None,
                  guessed=int(guessed[k]), structure=rows[k]) for k in range(len(ps)) if dcal[k] < pe[k]]
    higher = [k for k in range(len(ps)) if dcal[k] > pe[k]]
    out["published"] = dict(rows=len(ps), equal=sum(a == b for a, b in zip(dcal, pe)), lower=len(lower), higher=len(higher),
                            same_structure=sum(a == b for a, b in zip(rows, pdb)),
                            published_structure_evaluates_to_published_energy=sum(1 for k in range(len(ps)) if not st[k] and own_of_pub[k] == pe[k]),
                            lower_with_guessed_flag=sum(r["guessed"] for r in lower), lower_rows=lower, higher_rows=higher)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "published"}, indent=1))
    print({k: v for k, v in out["published"].items() if not k.endswith("_rows")})
    if higher:
        raise SystemExit(f"{len(higher)} sequences have an MFE above the published energy: a bug")


if __name__ == "__main__":
    main()
