"""Time rafft_amd's exact barrier trees (rafft_barriers_batch) on the benchmark set.  DESIGN.md section 15.  Needs the MI355X.
    python tools/barriers_measure.py [--reps R] [--delta D] [--max-len L] [--max-seqs N] [--links N] [--no-profile] [OUT.json]
                                                                                   (default profiles/barriers_headline.json)
Workload: the benchmark sequences of up to 200 nt; per sequence the band of `delta` = 2 kcal/mol from subopt_batch_raw with max_structs
= 100 000 (sequences that end in RAFFT_ERR_CAPACITY there are counted and skipped), handed over as the arrays it returns (stride
L + 1).  Every timed call of barriers_batch_raw ends with its trees on the host, so a host clock around it is a call time: one
warm-up call, then R warm calls, all kept, the median reported, with rows, neighbour probes that hit, minima and edges per second
and per sequence.  (The library counts the probes that hit, not those it makes: the probes made are counted here, on a sample of
rows, by the tests' third way of generating neighbours.)  Host and device: the kernels' total from ONE run of this script's own
child (`--child`: one warm-up call and one call) under `rocprofv3 --kernel-trace --stats` - a profile of that run, not of the timed
calls; the rest of a call is host work (parsing rows twice, staging, the trees) and copies.  Against findpath: on up to --links
(minimum, father) links the saddle of findpath_batch(both=True) at widths 16 and 64 beside the tree's exact one."""
import argparse
import csv
import glob
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def quantiles(v):
    import numpy as np
    v = np.asarray(v, dtype=np.float64)
    return dict(min=float(v.min()), q25=float(np.percentile(v, 25)), median=float(np.median(v)), q75=float(np.percentile(v, 75)),
                q99=float(np.percentile(v, 99)), max=float(v.max()), mean=float(v.mean()))


def kernel_profile(argv):
    """the kernels' totals of one child run under rocprofv3 --kernel-trace --stats (None when rocprofv3 is not there)"""
    exe = next((p for p in ("/opt/rocm/bin/rocprofv3",) if os.path.exists(p)), None)
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                            "--child"] + argv, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(error=(r.stderr or r.stdout)[-400:])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "barriers_" in name:
                    rows.append(dict(kernel=name.split("(")[0].replace("void ", ""), calls=int(row.get("Calls") or 0),
                                     total_ms=float(row["TotalDurationNs"]) / 1e6, average_ms=float(row.get("AverageNs") or 0.0) / 1e6,
                                     max_ms=float(row.get("MaxNs") or 0.0) / 1e6))
        return dict(note="one warm-up call and one call, both counted: halve the totals for one call", kernels=rows,
                    total_ms_per_call=sum(k["total_ms"] for k in rows) / 2.0)


def loop_neighbours(seq, row):
    """the number of neighbours of a row: its pairs, and the pairs of unpaired members of one loop that may form"""
    canonical = {"AU", "UA", "GC", "CG", "GU", "UG"}
    n, members, stack = 0, {}, [-1]
    for x, c in enumerate(row):
        if c == "(":
            stack.append(x)
        elif c == ")":
            stack.pop()
            n += 1
        else:
            members.setdefault(stack[-1], []).append(x)
    for g in members.values():
        for a, i in enumerate(g):
            n += sum(1 for j in g[a + 1:] if j - i > 3 and seq[i] + seq[j] in canonical)
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "barriers_headline.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--delta", type=float, default=2.0)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--max-seqs", type=int, default=0, help="0: all")
    ap.add_argument("--max-structs", type=int, default=100000)
    ap.add_argument("--links", type=int, default=20000)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import rafft_amd
    from rafft_amd import _native as N, barriers as B, findpath as F, wuchty
    seqs = [l.split("\t")[1] for l in gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt")]
    seqs = [s for s in seqs if len(s) <= args.max_len]
    if args.max_seqs:
        seqs = seqs[:args.max_seqs]
    delta = int(round(args.delta * 100))
    t0 = time.perf_counter()
    recs, rows, dcal = wuchty.subopt_batch_raw(seqs, delta, args.max_structs)
    t_subopt = time.perf_counter() - t0
    over = sum(r["status"] == N.ERR_CAPACITY for r in recs)
    keep = [k for k, r in enumerate(recs) if r["status"] == 0]
    n_asked = len(seqs)
    seqs, rows, dcal = [seqs[k] for k in keep], [rows[k] for k in keep], [dcal[k] for k in keep]
    n_rows = np.array([len(d) for d in dcal])
    say(f"{n_asked} sequences up to {args.max_len} nt, {over} above max_structs, {len(seqs)} bands, {int(n_rows.sum())} rows, subopt {t_subopt:.2f} s")
    call = lambda: B.barriers_batch_raw(seqs, rows, dcal)
    if args.child:
        for _ in range(2):
            call()
        return
    lens = np.array([len(s) for s in seqs])
    out = dict(device=torch.cuda.get_device_name(0), params=rafft_amd.params_info(), sequences_asked=n_asked, sequences_above_max_structs=int(over),
               n_sequences=len(seqs), delta_kcal=args.delta, max_structs=args.max_structs, rows=int(n_rows.sum()), rows_per_sequence=quantiles(n_rows),
               length=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())), subopt_seconds=t_subopt, reps=args.reps,
               workload="benchmark set up to max-len; the arrays of subopt_batch_raw, max_edges 0, workspace 0",
               clock="time.perf_counter around calls that end with their trees on the host; one warm-up call")
    t0 = time.perf_counter()
    got = call()
    say(f"warm-up call: {time.perf_counter() - t0:.2f} s")
    secs = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = call()
        secs.append(time.perf_counter() - t0)
        say(f"call: {secs[-1]:.2f} s")
    c = B.barriers_counters()
    med = float(np.median(secs))
    bad = [g["status"] for g in got if g["status"]]
    out.update(seconds_median=med, seconds_all=[float(v) for v in secs], counters=c, sequences_with_a_status=len(bad),
               rows_per_second=c["rows"] / med, hits_per_second=c["hits"] / med, hits_per_row=c["hits"] / max(c["rows"], 1),
               minima_per_sequence=quantiles([len(g["rank"]) for g in got]), edges_per_sequence=quantiles([len(g["edges"]) for g in got]),
               roots_per_sequence=quantiles([int((g["father"] < 0).sum()) for g in got]))
    # probes made, on a sample of rows (the library makes each of them twice: once for down, once for the edges)
    rng = np.random.default_rng(1)
    made, of_rows = 0, 0
    for _ in range(2000):
        s = int(rng.integers(len(seqs)))
        r = int(rng.integers(len(dcal[s])))
        made += loop_neighbours(seqs[s], rows[s][r][:len(seqs[s])].tobytes().decode("ascii"))
        of_rows += 1
    per_row = made / of_rows
    out["probes"] = dict(per_row_on_a_sample_of_rows=per_row, sample=of_rows, per_pass_estimate=per_row * c["rows"], per_second_estimate_both_passes=2 * per_row * c["rows"] / med)
    # against findpath
    links = [(s, m, int(f)) for s, g in enumerate(got) for m, f in enumerate(g["father"].tolist()) if f >= 0]
    if len(links) > args.links:
        links = [links[k] for k in sorted(rng.choice(len(links), args.links, replace=False).tolist())]
    text = lambda s, r: rows[s][r][:len(seqs[s])].tobytes().decode("ascii")
    a = [text(s, int(got[s]["rank"][m])) for s, m, _ in links]
    b = [text(s, int(got[s]["rank"][f])) for s, _, f in links]
    exact = np.array([int(got[s]["saddle_dcal"][m]) for s, m, _ in links])
    out["against_findpath"] = dict(links=len(links), note="findpath_batch(both=True) between a minimum and its father; its saddle is an upper bound of the exact one "
                                   "wherever its path stays in the band")
    for width in (16, 64):
        t0 = time.perf_counter()
        frecs, _, _ = F.findpath_batch([seqs[s] for s, _, _ in links], a, b, width=width, both=True, raise_errors=False)
        dt = time.perf_counter() - t0
        ok = np.array([r["status"] == 0 for r in frecs])
        sad = np.array([r["saddle_dcal"] for r in frecs])
        excess = (sad - exact)[ok]
        out["against_findpath"][f"width_{width}"] = dict(seconds=dt, solved=int(ok.sum()), share_exact=float((excess == 0).mean()), below_the_exact_saddle=int((excess < 0).sum()),
                                                         mean_excess_kcal_where_above=float(excess[excess > 0].mean() / 100.0) if (excess > 0).any() else 0.0,
                                                         max_excess_kcal=float(excess.max() / 100.0))
        say(f"findpath width {width}: {dt:.2f} s, exact on {float((excess == 0).mean()):.4f}")
    # one large band, for the scaling with rows x neighbours: the longest sequence at a wider delta
    big = max(seqs, key=len)
    for wide in (4.0, 5.0, 6.0, 7.0):
        brec, brows, bdcal = wuchty.subopt_batch_raw([big], int(round(wide * 100)), 1 << 21)
        if brec[0]["status"] != 0 or len(bdcal[0]) >= 300000:
            break
    if brec[0]["status"] == 0:
        B.barriers_batch_raw([big], brows, bdcal)
        bsecs = []
        for _ in range(3):
            t0 = time.perf_counter()
            bg = B.barriers_batch_raw([big], brows, bdcal)[0]
            bsecs.append(time.perf_counter() - t0)
        bc = B.barriers_counters()
        out["one_large_band"] = dict(length=len(big), delta_kcal=wide, rows=len(bdcal[0]), status=bg["status"], seconds_median=float(np.median(bsecs)), seconds_all=bsecs,
                                     rows_per_second=len(bdcal[0]) / float(np.median(bsecs)), hits=bc["hits"], minima=bc["minima"], edges=bc["edges"],
                                     roots=int((bg["father"] < 0).sum()))
        say(f"one band of {len(bdcal[0])} rows: {float(np.median(bsecs)):.2f} s")
    if not args.no_profile:
        child = ["--delta", str(args.delta), "--max-len", str(args.max_len), "--max-seqs", str(args.max_seqs), "--max-structs", str(args.max_structs)]
        out["kernel_profile"] = kernel_profile(child)
        kp = out["kernel_profile"]
        if kp and "total_ms_per_call" in kp:
            out["device_share_of_a_call"] = kp["total_ms_per_call"] / 1e3 / med
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
