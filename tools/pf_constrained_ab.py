"""A/B of the unconstrained partition-function call across two builds, and the price of the constraint pack.
Needs the MI355X.
    python tools/pf_constrained_ab.py PARENT_LIB [--reps R] [OUT.txt]      (default profiles/pf_constrained_ab.txt)
The workload is that of tools/pf_measure.py: rafft_pf_batch on the whole benchmark set without prob_out, one call, timed on the host
(the C call ends with its results there).  A repetition is a fresh process that loads one build (RAFFT_LIB), makes two warm-up calls
and reports the median of five timed calls; the repetitions of PARENT_LIB (the library built from the parent commit) and of this
tree's library alternate, R each.  The unconstrained call of this build must not be slower than the parent's: its median has to lie
within the min-max range of the parent's own repetitions (the policy is meant to compile to nothing there, so the parent's spread is
the margin), and both builds have to return the same bits.  For information, in the processes of this build and through
rafft_amd.mccaskill: pf_batch, pf_constrained_batch with no constraint at all and with all-'.' strings on the same set."""
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

    # rafft_pf_batch through ctypes alone, the same way for both builds (the binding of rafft_amd asks for every symbol of this tree's header)
    N._one_hip_runtime()
    L = C.CDLL(os.environ["RAFFT_LIB"])
    L.rafft_pf_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_double, C.c_double, C.c_longlong, C.POINTER(N.PfSeq),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    _, arr, lens, bufs, out = N.seq_arrays(seqs, rows=True)
    rec = (N.PfSeq * len(seqs))()

    def pf_batch():
        if L.rafft_pf_batch(len(seqs), arr, lens, 37.0, 0.0, 0, rec, out, None):
            raise SystemExit("rafft_pf_batch failed")

    res = dict(n_seq=len(seqs), pf_batch=timed(pf_batch))
    h = hashlib.sha256(bytes(rec))
    for b in bufs:
        h.update(b.raw)
    res["bits"] = h.hexdigest()                       # every record and every centroid row
    if os.environ.get("AB_CONSTRAINED"):
        from rafft_amd import mccaskill
        dots = ["." * len(s) for s in seqs]
        free = mccaskill.pf_batch_raw(seqs, probs=False)
        for con in (None, dots):
            got = mccaskill.pf_constrained_batch_raw(seqs, con, probs=False, unpaired=False)
            assert got[0] == free[0] and got[1] == free[1]
        res["pf_batch_python"] = timed(lambda: mccaskill.pf_batch_raw(seqs, probs=False))
        res["constrained_no_constraint"] = timed(lambda: mccaskill.pf_constrained_batch_raw(seqs, probs=False, unpaired=False))
        res["constrained_all_dots"] = timed(lambda: mccaskill.pf_constrained_batch_raw(seqs, dots, probs=False, unpaired=False))
    print("AB " + json.dumps(res), flush=True)


def repetition(lib, constrained):
    env = dict(os.environ, RAFFT_LIB=lib)
    env.pop("AB_CONSTRAINED", None)
    if constrained:
        env["AB_CONSTRAINED"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode:
        raise SystemExit(f"a repetition with {lib} failed ({r.returncode}):\n{r.stdout}{r.stderr}")
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("AB "))[3:])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("parent_lib", nargs="?")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "pf_constrained_ab.txt"))
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args(argv)
    if args.child:
        return child()
    if not args.parent_lib or args.reps < 5:
        raise SystemExit("usage: pf_constrained_ab.py PARENT_LIB [--reps R >= 5] [OUT.txt]")
    own = os.path.join(ROOT, "rafft_amd", "libraffthip.so")
    parent, this = [], []
    for k in range(args.reps):                       # interleaved: parent, this, parent, this, ...
        parent.append(repetition(os.path.abspath(args.parent_lib), False))
        this.append(repetition(own, True))
        print(f"repetition {k}: parent {parent[-1]['pf_batch']:.3f} ms, this {this[-1]['pf_batch']:.3f} ms", flush=True)
    a, b = [r["pf_batch"] for r in parent], [r["pf_batch"] for r in this]
    same = len({r["bits"] for r in parent + this}) == 1
    med = statistics.median(b)
    inside = min(a) <= med <= max(a)
    faster = med < min(a)
    series = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    info = lambda key: f"{series([r[key] for r in this])}   median {statistics.median(r[key] for r in this):.3f}"
    plain = statistics.median(r["pf_batch_python"] for r in this)
    lines = [f"pf_batch on the benchmark set ({this[0]['n_seq']} sequences, no prob_out), one call, ms; a repetition = a fresh process, 2 warm-up calls, median of {CALLS} calls",
             f"parent  : {series(a)}   median {statistics.median(a):.3f}  min {min(a):.3f}  max {max(a):.3f}",
             f"this    : {series(b)}   median {med:.3f}  min {min(b):.3f}  max {max(b):.3f}",
             f"gate    : the median of this build {'lies within' if inside else 'is below' if faster else 'LIES ABOVE'} the parent's min-max range"
             f" -> {'pass' if inside or faster else 'FAIL'}",
             f"bits    : the records and centroid rows of all repetitions of both builds are {'the same' if same else 'NOT THE SAME -> FAIL'}",
             "for information (this build, same processes, same set; through rafft_amd.mccaskill, whose packing of the arguments is in the time):",
             f"pf_batch                                  : {info('pf_batch_python')}",
             f"pf_constrained_batch, no constraint       : {info('constrained_no_constraint')}   {statistics.median(r['constrained_no_constraint'] for r in this) / plain:.3f} x",
             f"pf_constrained_batch, all-'.' constraints : {info('constrained_all_dots')}   {statistics.median(r['constrained_all_dots'] for r in this) / plain:.3f} x"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if not ((inside or faster) and same):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
