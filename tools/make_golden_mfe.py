"""Writes tests/golden/mfe_published.tsv.gz from the reference's published MFE table (benchmark_results/mfe_scores.csv, made by
bench_mfe.py with ViennaRNA's RNA.fold): sequence, published structure, published energy in dcal, for the sequences of the
benchmark set (tests/golden/bench_inputs.tsv.gz) of at most 120 nt, in the table's order.  Run where the reference tree is:

    python tools/make_golden_mfe.py REFERENCE_DIR

The fixture is data of the reference (results it recorded), not program text."""
import csv
import gzip
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_LEN = 120


def main(ref):
    rows, seen = [], set()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "bench_inputs.tsv.gz"), "rt") as fh:
        bench = {line.split("\t")[1] for line in fh}
    with open(os.path.join(ref, "benchmark_results", "mfe_scores.csv"), newline="") as fh:
        for r in csv.DictReader(fh):
            s = r["seq"].strip()
            if len(s) > MAX_LEN or s in seen or s not in bench:
                continue
            seen.add(s)
            assert len(r["struct"]) == len(s) and set(r["struct"]) <= set("().")
            rows.append((s, r["struct"], int(round(float(r["nrj"]) * 100))))
    out = os.path.join(ROOT, "tests", "golden", "mfe_published.tsv.gz")
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as gz:
        for s, d, e in rows:
            gz.write(f"{s}\t{d}\t{e}\n".encode("ascii"))
    print(len(rows), "rows,", os.path.getsize(out), "bytes ->", out)


if __name__ == "__main__":
    main(sys.argv[1])
