"""A/B of the single-strand MFE call across two builds, and what a dimer fold costs beside it.  Needs the MI355X.
    python tools/cofold_ab.py PARENT_LIB [--reps R] [OUT.txt]      (default profiles/cofold_ab.txt)
The workload is that of tools/mfe_measure.py: rafft_mfe_batch on the whole benchmark set, one call, timed on the host (the C call
ends with its results there).  A repetition is a fresh process that loads one build (RAFFT_LIB), makes two warm-up calls and reports
the median of five timed calls; the repetitions of PARENT_LIB (the library built from the parent commit) and of this tree's library
alternate, R each.  The gate: the cut policy is meant to compile to nothing in the single-strand kernels, so this build's median has
to lie within the min-max range of the parent's own repetitions (or below it), and both builds must return the same records and
rows.  For information, in the processes of this build: rafft_cofold_batch on the same sequences cut in the middle, and without a
cut, beside rafft_mfe_batch."""
import argparse
import gzip
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
CALLS = 5


def child():
    """one repetition, in this process: a JSON line of medians in milliseconds"""
    import ctypes as C
    from rafft_amd import _native as N
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]

    def timed(fn):
        fn(); fn()
        out = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    # through ctypes alone, the same way for both builds (the binding of rafft_amd asks for every symbol of this tree's header)
    N._one_hip_runtime()
    L = C.CDLL(os.environ["RAFFT_LIB"])
    L.rafft_mfe_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_int, C.c_longlong, C.POINTER(N.MfeSeq), C.POINTER(C.c_void_p)]
    _, arr, lens, bufs, out = N.seq_arrays(seqs, rows=True)
    rec = (N.MfeSeq * len(seqs))()

    def mfe_batch():
        if L.rafft_mfe_batch(len(seqs), arr, lens, 37.0, 0, 0, rec, out):
            raise SystemExit("rafft_mfe_batch failed")

    res = dict(n_seq=len(seqs), mfe_batch=timed(mfe_batch))
    digest = hashlib.sha256(bytes(rec))
    for b in bufs:
        digest.update(b.value)
    res["records"] = digest.hexdigest()
    if os.environ.get("AB_COFOLD"):
        L.rafft_cofold_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_double, C.c_int, C.c_longlong,
                                         C.POINTER(N.CofoldSeq), C.POINTER(C.c_void_p)]
        crec = (N.CofoldSeq * len(seqs))()
        mid = (C.c_int * len(seqs))(*[len(s) // 2 for s in seqs])
        free = [(r.status, r.dcal, r.n_pairs) for r in rec], [b.value for b in bufs]

        def cofold(cuts):
            if L.rafft_cofold_batch(len(seqs), arr, lens, cuts, 37.0, 0, 0, crec, out):
                raise SystemExit("rafft_cofold_batch failed")

        res["cofold_no_cut"] = timed(lambda: cofold(None))
        assert ([(r.status, r.dcal, r.n_pairs) for r in crec], [b.value for b in bufs]) == free, "without a cut the dimer call is not rafft_mfe_batch"
        res["cofold_mid_cut"] = timed(lambda: cofold(mid))
        res["n_bound"] = sum(r.n_inter > 0 for r in crec)
    print("AB " + json.dumps(res), flush=True)


def repetition(lib, cofold):
    env = dict(os.environ, RAFFT_LIB=lib)
    env.pop("AB_COFOLD", None)
    if cofold:
        env["AB_COFOLD"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise SystemExit(f"a repetition with {lib} failed ({r.returncode}):\n{r.stdout}{r.stderr}")
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("AB "))[3:])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("parent_lib", nargs="?")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "cofold_ab.txt"))
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args(argv)
    if args.child:
        return child()
    if not args.parent_lib or args.reps < 5:
        raise SystemExit("usage: cofold_ab.py PARENT_LIB [--reps R >= 5] [OUT.txt]")
    own = os.path.join(ROOT, "rafft_amd", "libraffthip.so")
    parent, this = [], []
    for k in range(args.reps):                       # interleaved: parent, this, parent, this, ...
        parent.append(repetition(os.path.abspath(args.parent_lib), False))
        this.append(repetition(own, True))
        print(f"repetition {k}: parent {parent[-1]['mfe_batch']:.3f} ms, this {this[-1]['mfe_batch']:.3f} ms", flush=True)
    a, b = [r["mfe_batch"] for r in parent], [r["mfe_batch"] for r in this]
    same = len({r["records"] for r in parent + this}) == 1
    med = statistics.median(b)
    inside = min(a) <= med <= max(a)
    faster = med < min(a)
    series = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    info = lambda key: f"{series([r[key] for r in this])}   median {statistics.median(r[key] for r in this):.3f}"
    lines = [f"mfe_batch on the benchmark set ({this[0]['n_seq']} sequences), one call, ms; a repetition = a fresh process, 2 warm-up calls, median of {CALLS} calls",
             f"parent  : {series(a)}   median {statistics.median(a):.3f}  min {min(a):.3f}  max {max(a):.3f}",
             f"this    : {series(b)}   median {med:.3f}  min {min(b):.3f}  max {max(b):.3f}",
             f"gate    : the median of this build {'lies within' if inside else 'is below' if faster else 'LIES ABOVE'} the parent's min-max range"
             f" -> {'pass' if inside or faster else 'FAIL'}; records and rows of the two builds {'are the same' if same else 'DIFFER'}",
             "for information (this build, same processes, same set, the C calls):",
             f"cofold_batch, no cut               : {info('cofold_no_cut')}",
             f"cofold_batch, cut in the middle    : {info('cofold_mid_cut')}   ({this[0]['n_bound']} of the dimers hold a pair between the strands)",
             f"a dimer fold costs {statistics.median(r['cofold_mid_cut'] for r in this) / med:.3f} x the single-strand call"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if not ((inside or faster) and same):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
