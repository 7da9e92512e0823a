"""`rafft` command line - same flags, defaults and output formats as the reference's
bin/rafft (bin/rafft:7-31,34-80), running the fold on the MI355X.

Differences, all additive: `-sf` may hold several FASTA records (they are folded as one
GPU batch and printed one after the other); `--nono` (the reference's to-be-removed
test implementation, bin/rafft:29) is not provided.

Energies: the reference evaluates with ViennaRNA's loaded parameter set (rafft/utils.py:17-21).  Here the set is read ONCE, up
front: from RAFFT_PARAMS=<ViennaRNA 2.x parameter file>, else through an importable `RNA` module (RNA.params_save),
else the built-in Turner-2004 37 C tables are used.  The built-in tables reproduce all 11 505 energies the reference
publishes, but entries no published energy exercises are rule-derived: out of sample about 1 structure in 20 gets
another energy than ViennaRNA's - supply ViennaRNA's own tables when that matters.  Which set is
active: `python -c "import rafft_amd; print(rafft_amd.params_info())"`."""
import argparse
import sys


# (flags, keyword arguments) - the option surface of the reference's CLI, bin/rafft:11-30.  `--pad`, `--min_bp`
# and `--bp_only` are accepted and ignored exactly as there (they are parsed but never forwarded, bin/rafft:50-52).
_OPTIONS = [
    (("--sequence", "-s"), dict(help="sequence")),
    (("--seq_file", "-sf"), dict(help="sequence file (FASTA or plain)")),
    (("--n_mode", "-n"), dict(type=int, default=100, help="number of positional lags searched for stems")),
    (("--max_stack", "-ms"), dict(type=int, default=1, help="number of structures kept per folding step")),
    (("--min_nrj", "-mn"), dict(type=float, default=0, help="a stem must change the energy by less than this")),
    (("--min_bp", "-mb"), dict(type=int, default=1, help="accepted, unused")),
    (("--min_hp", "-mh"), dict(type=int, default=3, help="minimum unpaired positions in a hairpin")),
    (("--pad", "-p"), dict(type=float, default=1.0, help="accepted, unused")),
    (("--max_branch",), dict(type=int, default=1000, help="maximum number of new structures per folding step")),
    (("--bp_only",), dict(action="store_true", help="accepted, unused")),
    (("--bench",), dict(action="store_true", help="one line per structure: seq len structure energy #pairs")),
    (("-tr", "--traj"), dict(action="store_true", help="print the whole fast-folding graph")),
    (("--temp",), dict(type=float, default=37.0, help="temperature in C (default 37).  Other temperatures need a ViennaRNA parameter file with\nenthalpies (RAFFT_PARAMS=<file>, or an importable RNA module): the built-in tables are 37 C only")),
    (("-gc", "--gc_wei"), dict(type=float, default=3.0, help="GC weight")),
    (("-au", "--au_wei"), dict(type=float, default=2.0, help="AU weight")),
    (("-gu", "--gu_wei"), dict(type=float, default=1.0, help="GU weight")),
    (("--batch",), dict(action="store_true", help="every record of -sf is its own sequence, all folded as one GPU batch: FASTA records,\n"
                                                  "one sequence per line, or a CSV with a header (column --csv_column; the reference's\n"
                                                  "benchmark_cleaned_all_length.csv has `seq`).  With --bench this replaces the process pool of\n"
                                                  "benchmark_results/bench_fft.py")),
    (("--csv_column",), dict(default="seq", help="sequence column of a CSV given to -sf --batch (default: seq)")),
    (("--scores",), dict(metavar="OUT.csv", help="with -sf CSV --batch: score the final beam of every sequence against its known structure on the\n"
                                                 "GPU (PPV / sensitivity as RNAstructure's scorer, one position of slip) and write the table of\n"
                                                 "benchmark_results/scoring.py: seq,len_seq,struct,nrj,nbp,pvv,sens,name.  The CSV has a header\n"
                                                 "(columns by name) or is the reference's headerless seq,struct,name file")),
    (("--select",), dict(choices=("ppv", "energy"), default="ppv", help="structure reported by --scores: the last one of the beam that reaches the\n"
                                                                        "highest PPV (scoring.py), or the first one (scoring.py --one)")),
    (("--known_column",), dict(default="struct", help="known-structure column of a CSV with a header (default: struct)")),
    (("--name_column",), dict(default="name", help="name column of a CSV with a header (default: name)")),
    (("--kin",), dict(metavar="OUT", help="with -sf FILE --batch: fold with trajectories and solve the folding kinetics of every sequence's\n"
                                          "fast-folding graph on the GPU, all in one call (rafft_kin.kinetics_batch).  OUT gets, per sequence,\n"
                                          "a `> index sequence` line and the table `rafft_kin` prints, sorted by final population")),
    (("--mfe",), dict(action="store_true", help="no RAFFT fold: the minimum-free-energy structure of every sequence on the GPU (rafft_amd.mfe_batch;\n"
                                                "dangles=2, lonely pairs allowed, interior loops up to 30 - RNA.fold's defaults), one line per sequence as\n"
                                                "benchmark_results/src/vrna_mfe.py prints it: seq len structure energy #pairs.  With --scores the table of\n"
                                                "mfe_scores.csv.  Works with -s SEQ and with -sf FILE --batch")),
    (("--span",), dict(type=int, default=None, metavar="W", help="with --mfe: only pairs (i, j) with j - i + 1 <= W, 1 <= W <= 4096 (rafft_amd.mfe_span_batch; as\n"
                                                                 "`RNAfold --maxBPspan W`), for sequences of up to 32768 nt.  Output and --scores as --mfe")),
    (("-C", "--constraint"), dict(action="store_true", dest="constraint",
                                  help="with --mfe or --pf: fold under hard constraints (rafft_amd.mfe_constrained_batch / pf_constrained_batch; as `RNAfold -C\n--enforceConstraint`).\n"
                                       "After each sequence of the -sf file, or on stdin after -s SEQ, comes a constraint line of the sequence's\n"
                                       "length: . nothing, x unpaired, | paired, < > paired with a partner downstream / upstream, ( ) this pair.\n"
                                       "Output as --mfe, with the pseudo-energy (kcal/mol) as one more column.  Not with --span")),
    (("--shape",), dict(default=None, metavar="FILE", help="with --mfe or --pf: SHAPE-directed folding (Deigan's pseudo-energies on stacked pairs, as `RNAfold --shape FILE`).\n"
                                                           "FILE holds lines `position reactivity`, 1-based; a missing position or a negative value means no\n"
                                                           "data.  With --batch one block per sequence, each introduced by a `>name` line, in the -sf file's\n"
                                                           "order.  Output as -C.  Not with --span")),
    (("--shape-slope",), dict(type=float, default=1.8, metavar="M", dest="shape_slope", help="with --shape: m of m ln(reactivity + 1) + b, kcal/mol (default 1.8)")),
    (("--shape-intercept",), dict(type=float, default=-0.6, metavar="B", dest="shape_intercept", help="with --shape: b, kcal/mol (default -0.6)")),
    (("--cofold",), dict(action="store_true", help="no RAFFT fold: the minimum-free-energy structure of every two-strand dimer on the GPU (rafft_amd.cofold_batch; as\n"
                                                   "RNAcofold's MFE).  Every sequence is written A&B, with one `&`; with -s \"A&B\" or with -sf FILE --batch.  Per\n"
                                                   "dimer one line `A&B len rowA&rowB energy n_inter`, n_inter the pairs between the strands.  Not with any of the\n"
                                                   "other modes, -C, --shape or --span")),
    (("--binding",), dict(action="store_true", help="with --cofold: four more columns, the MFE of the dimer, of A and of B and the difference E(AB) - E(A) - E(B), kcal/mol")),
    (("--pf",), dict(action="store_true", help="no RAFFT fold: the partition function of every sequence on the GPU (rafft_amd.pf_batch; the ensemble of --mfe),\n"
                                               "one line per sequence: seq len centroid energy #pairs mfe_frequency - the centroid holds the pairs with\n"
                                               "probability above 0.5, energy is the ensemble free energy.  With --scores the centroid rows are scored.\n"
                                               "Works with -s SEQ and with -sf FILE --batch; not with --mfe, --kin or --traj")),
    (("--pf-span",), dict(type=int, default=None, metavar="W", dest="pf_span",
                          help="with --pf: the ensemble restricted to pairs (i, j) with j - i + 1 <= W, 1 <= W <= 4096 (rafft_amd.pf_span_batch; as\n"
                               "`RNAfold -p --maxBPspan W`), for sequences of up to 32768 nt.  Output and --scores as --pf")),
    (("--bpp",), dict(type=str, default=None, metavar="FILE", help="with --pf: the pair probabilities of every sequence into FILE, one line `name i j p` per pair\n"
                                                                  "with p >= --bpp-cutoff, positions 1-based, i ascending then j.  With or without --pf-span")),
    (("--bpp-cutoff",), dict(type=float, default=1e-5, metavar="C", dest="bpp_cutoff", help="the smallest probability --bpp writes (default 1e-5)")),
    (("--mea",), dict(type=float, nargs="?", const=1.0, default=None, metavar="GAMMA",
                      help="no RAFFT fold: the maximum-expected-accuracy structure of every sequence on the GPU (rafft_amd.mea_batch; the\n"
                           "pair probabilities of --pf; GAMMA weighs a pair against an unpaired base, default 1.0), one line per sequence:\n"
                           "seq len structure energy_of_structure mea diversity.  With --scores the MEA rows are scored.  With --sample N\n"
                           "the consensus of the N sampled rows (rafft_amd.mea_from_probs on their pair frequencies: seq len structure mea\n"
                           "diversity) in place of the graph text.  Works with -s SEQ and with -sf FILE --batch; not with --mfe, --pf,\n"
                           "--subopt, --kin or --traj")),
    (("--sample",), dict(type=int, metavar="N", help="no RAFFT fold: N structures drawn from the Boltzmann ensemble of every sequence on the GPU\n"
                                                     "(rafft_amd.sample_batch; the ensemble of --pf).  Per sequence the fast-folding-graph text with a single\n"
                                                     "step 0 that holds the distinct sampled structures, energy ascending - `rafft_landscape OUT` draws the\n"
                                                     "sampled ensemble.  With --scores the samples of every sequence are scored as a beam.\n"
                                                     "Works with -s SEQ and with -sf FILE --batch; not with --mfe, --pf, --kin or --traj")),
    (("--subopt",), dict(type=float, metavar="DELTA", help="no RAFFT fold: every structure of every sequence within DELTA kcal/mol of its minimum free energy on\n"
                                                           "the GPU (rafft_amd.subopt_batch; the ensemble of --mfe; as `RNAsubopt -e DELTA -s`).  Per sequence the\n"
                                                           "fast-folding-graph text with a single step 0 that holds the band, energy ascending - `rafft_landscape OUT`\n"
                                                           "draws it.  With --scores the band of every sequence is scored as a beam.\n"
                                                           "Works with -s SEQ and with -sf FILE --batch; not with --mfe, --pf, --sample, --kin or --traj")),
    (("--max-structs",), dict(type=int, default=100000, metavar="N", help="with --subopt: a sequence with more than N structures in the band is an error\n"
                                                                          "(default 100000)")),
    (("--findpath",), dict(action="store_true", help="no RAFFT fold: with -sf FILE, a folding path with a low energy barrier between two structures of every\n"
                                                     "record on the GPU (rafft_amd.findpath_batch; the direct-path search of ViennaRNA's findpath: only the\n"
                                                     "pairs in which the two structures differ are removed or added).  A record of FILE is an optional\n"
                                                     "`>name` line, then three lines: the sequence, the start structure, the end structure (dot-brackets of\n"
                                                     "the sequence's length); empty lines are skipped.  Per record the output is the `>name` line if there was\n"
                                                     "one, the sequence, one line `structure energy` per structure of the path from start to end, and a\n"
                                                     "line `saddle S barrier B kcal/mol` - S the highest energy of the path, B = S minus the start's energy.\n"
                                                     "Not with any of the other modes")),
    (("--width",), dict(type=int, default=16, metavar="W", help="with --findpath: partial paths kept per step, 1 .. 1024 (default 16); more finds lower\n"
                                                                 "barriers and takes longer")),
    (("--both",), dict(action="store_true", help="with --findpath: search from the end to the start as well and report the path with the lower saddle")),
    (("--descend",), dict(action="store_true", help="gradient walks to local minima on the GPU (rafft_amd.descend_batch; insertion and deletion of single pairs,\n"
                                                    "steepest descent, as ViennaRNA's path_gradient).  With --sample N or --subopt DELTA every structure walks down\n"
                                                    "to its local minimum and the one-step graph holds the distinct minima, energy ascending, each followed by\n"
                                                    "the number of structures in its basin (`rafft_landscape OUT` draws it).  Alone, with -sf FILE: a record of\n"
                                                    "FILE is an optional `>name` line, the sequence and one or more dot-bracket lines; per record the output\n"
                                                    "is the `>name` line if there was one, the sequence and one line `structure energy count` per distinct\n"
                                                    "minimum its structures walk down to, energy ascending.  Not with --scores, --mfe, --pf, --findpath, --kin, --traj")),
    (("--max-steps",), dict(type=int, default=0, metavar="N", help="with --descend: a walk that is not at a minimum after N steps is an error (default 0: twice the\n"
                                                                    "sequence's length + 16, which no walk of the tests came near); with --kinfold: a trajectory that has\n"
                                                                    "not ended after N steps is an error (default 0: 2^20)")),
    (("--kinfold",), dict(type=int, default=None, metavar="N", help="with -sf FILE --batch and --tmax T: N stochastic folding trajectories per sequence from the open chain on\n"
                                                                   "the GPU (rafft_amd.kinfold_batch; insertion and deletion of single pairs, Metropolis rates, as ViennaRNA's\n"
                                                                   "Kinfold).  Per sequence the output is the `>name` line if there was one, the sequence, with --stop the line\n"
                                                                   "`structure energy` of the stop structure, the line `arrived SHARE median T mean T` over the first-passage\n"
                                                                   "times of the trajectories that reached it by T (`arrived 0.0000` alone when none did), and with --times K\n"
                                                                   "K lines `time mean-energy arrived-share`.  --seed S and --max-steps M apply.  Not with any of the other modes")),
    (("--tmax",), dict(type=float, default=None, metavar="T", help="with --kinfold: the time at which a trajectory ends, in units of 1 / (rate of a downhill move)")),
    (("--stop",), dict(default=None, metavar="mfe|FILE", help="with --kinfold: the structure at which a trajectory ends - `mfe`: the minimum-free-energy structure of\n"
                                                             "every sequence (rafft_amd.mfe_batch); FILE: one dot-bracket line per sequence")),
    (("--times",), dict(type=int, default=0, metavar="K", help="with --kinfold: a table of the mean energy and the arrived share at K log-spaced times up to T")),
    (("--barriers",), dict(action="store_true", help="with --subopt DELTA: the exact barrier tree of every sequence's band on the GPU (rafft_amd.barrier_trees; as\n"
                                                     "`RNAsubopt -e DELTA -s | barriers`): per sequence the `>name` line if there was one, the sequence and one\n"
                                                     "line `index structure energy father barrier` per local minimum, energy ascending (father 0: a root).\n"
                                                     "Not with --descend or --scores")),
    (("--minh",), dict(type=float, default=0.0, metavar="H", help="with --barriers: minima whose barrier is below H kcal/mol are folded into their fathers (default 0)")),
    (("--seed",), dict(type=int, default=0, help="with --sample or --kinfold: the seed (default 0); the same seed gives the same structures")),
    (("--max_time", "-mt"), dict(type=float, default=30, help="with --kin: max time (exp scale), as rafft_kin -mt")),
    (("--n_steps", "-ns"), dict(type=int, default=100, help="with --kin: number of sample times, as rafft_kin -ns")),
    (("--output", "-o"), dict(help="write the result there instead of stdout")),
    (("--sidecar",), dict(help="with --traj: also write the fast-folding graph as a binary side-car (exact dcal energies,\n"
                               "no strings to re-parse) that `rafft_kin --sidecar` reads; with several sequences the\n"
                               "files are <SIDECAR>.0, <SIDECAR>.1, ...")),
]


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    for flags, kw in _OPTIONS:
        parser.add_argument(*flags, **kw)
    return parser.parse_args(argv)


_SEQ_LETTERS = frozenset("ACGUTN")
_DB_LETTERS = frozenset("().<>[]")


def read_records(args):
    """(sequences, known structures or None, names or None) of the input.  Known structures and names exist for a CSV only:
    with a header line the columns --csv_column / --known_column / --name_column, without one the reference's three columns
    seq,struct,name (benchmark_cleaned_all_length.csv, read by read_true_struct, benchmark_results/scoring.py:31-36).  A first
    line is data, not a header, when its first field consists of the upper-case sequence letters only and its second field is a
    dot-bracket string of the same length."""
    assert args.sequence is not None or args.seq_file is not None, "error, the sequence is missing!"
    if args.sequence is not None:
        return [args.sequence], None, None
    lines = [l.strip() for l in open(args.seq_file)]
    if not args.batch:   # reference behaviour: all non-header lines joined (bin/rafft:42)
        return ["".join(l for l in lines if not l.startswith(">")).replace("T", "U")], None, None
    seqs, cur = [], []
    if lines and "," in lines[0] and not lines[0].startswith(">"):     # CSV
        import csv
        first = [f.strip() for f in lines[0].split(",")]
        with open(args.seq_file, newline="") as fh:
            if first[0] and set(first[0]) <= _SEQ_LETTERS and set(first[1]) <= _DB_LETTERS and len(first[1]) == len(first[0]):   # no header line: seq,struct,name
                rows = [r for r in csv.reader(fh) if r and r[0].strip()]
                col = lambda k: [r[k].strip() for r in rows] if all(len(r) > k for r in rows) else None
                return [r[0].strip().replace("T", "U") for r in rows], col(1), col(2)
            rd = csv.DictReader(fh)
            if args.csv_column not in (rd.fieldnames or []):
                raise SystemExit(f"{args.seq_file}: no column {args.csv_column!r} (columns: {rd.fieldnames})")
            rows = [r for r in rd if r[args.csv_column].strip()]
            col = lambda name: [(r[name] or "").strip() for r in rows] if name in rd.fieldnames else None
            return ([r[args.csv_column].strip().replace("T", "U") for r in rows],
                    col(getattr(args, "known_column", "struct")), col(getattr(args, "name_column", "name")))
    fasta = any(l.startswith(">") for l in lines)
    for l in lines:
        if fasta:
            if l.startswith(">"):
                if cur:
                    seqs.append("".join(cur))
                cur = []
            elif l:
                cur.append(l)
        elif l:
            seqs.append(l)
    if cur:
        seqs.append("".join(cur))
    return [s.replace("T", "U") for s in seqs], None, None


def read_sequences(args):
    return read_records(args)[0]


def write_scores(path, seqs, names, results, table, select="ppv", traj=False):
    """The reference's score table (benchmark_results/scoring.py:120-128): header `seq,len_seq,struct,nrj,nbp,pvv,sens,name`, one
    line per sequence - the last structure of the final beam that reaches the highest PPV (select="ppv", scoring.py:90-91) or the
    first one (select="energy", `--one`).  `table`: what scoring.score_batch_gpu returns."""
    import numpy as np
    from .utils import energies_from_dcal
    pick = np.asarray(table["pick_ppv" if select == "ppv" else "pick_first"])
    row0, n_known = np.asarray(table["row0"]), np.asarray(table["n_known"])
    with open(path, "w") as out:
        out.write("seq,len_seq,struct,nrj,nbp,pvv,sens,name\n")
        for k, s in enumerate(seqs):
            status = int(table["seq_status"][k])
            if status or pick[k] < 0:
                raise SystemExit(f"--scores: sequence {k} ({names[k]}): no scored structure (status {status})")
            raw = results.raw(k) if hasattr(results, "raw") else None
            if raw is not None:
                L, sizes, rows, dcal = raw
                at = len(rows) - sizes[-1] + int(pick[k])
                struct, nrj = rows[at].tobytes().decode("ascii"), float(energies_from_dcal(dcal[at:at + 1])[0])
            else:
                st = (results[k][0] if traj else results[k])[int(pick[k])]
                struct, nrj = st.str_struct, st.energy
            r = int(row0[k] + pick[k])
            n_pred, hit_pred, hit_known = int(table["n_pred"][r]), int(table["hit_pred"][r]), int(table["hit_known"][r])
            ppv = 100.0 * hit_pred / n_pred if n_pred else 0.0
            sens = 100.0 * hit_known / int(n_known[k]) if n_known[k] else 0.0
            out.write(f"{s},{len(s)},{struct},{nrj},{struct.count('(')},{round(ppv, 2)},{round(sens, 2)},{names[k]}\n")


def write_kinetics(path, seqs, tables):
    """--kin: per sequence `> index sequence` and the lines of rafft_kin (structure, final population, energy, index), sorted by
    final population.  `tables`: what rafft_kin.kinetics_batch returns; a sequence whose fold failed has a header line only."""
    with open(path, "w") as out:
        for k, s in enumerate(seqs):
            out.write(f"> {k} {s}\n")
            if tables[k] is None:
                continue
            for st, nrj, fp, si in sorted(tables[k][3], key=lambda el: el[2]):
                out.write("{} {:6.3f} {:5.1f} {:d}\n".format(st, fp, nrj, si))


def format_result(sequence, result, args):
    out = []
    if args.traj:
        final_struct, trajectory = result
        out.append(f"{sequence}")
        for si, fold_step in enumerate(trajectory):
            out.append("# {:-^20}".format(si))
            for struct in fold_step:
                out.append(f"{struct.str_struct} {struct.energy:6.1f}")
    else:
        if not args.bench:
            out.append(f"{sequence}")
        for struct in result:
            if args.bench:
                out.append(f"{sequence} {len(sequence)} {struct.str_struct} {struct.energy:6.1f} {struct.str_struct.count('(')}")
            else:
                out.append(f"{struct.str_struct} {struct.energy:6.1f}")
    return "\n".join(out)


def format_mfe_line(sequence, struct):
    """the line of benchmark_results/src/vrna_mfe.py:26"""
    return f"{sequence} {len(sequence)} {struct.str_struct} {struct.energy} {struct.str_struct.count('(')}"


def read_constrained_fasta(path):
    """(sequences, constraints, names) of a file for --mfe -C: per record an optional `>name` line, the sequence on one line and its
    constraint line, as `RNAfold -C` reads them"""
    seqs, cons, names, name = [], [], [], ""
    lines = [l.strip() for l in open(path)]
    body = []
    for l in lines + [">"]:
        if l.startswith(">"):
            if len(body) % 2:
                raise SystemExit(f"{path}: -C needs a constraint line after every sequence")
            for k in range(0, len(body), 2):
                seqs.append(body[k].replace("T", "U")); cons.append(body[k + 1]); names.append(name)
            body, name = [], l[1:].strip()
        elif l:
            body.append(l)
    return seqs, cons, names


def read_constraint_line():
    """The constraint of -s SEQ -C: one line on stdin, for --pf as for --mfe.  A stdin that gives none (closed, empty, not
    readable) is an error here, not a malformed constraint further down"""
    try:
        line = sys.stdin.readline().strip()
    except OSError:
        line = ""
    if not line:
        raise SystemExit("-C after -s SEQ reads the constraint line from stdin, for --pf as for --mfe: none came")
    return line


def read_shape(path, lens, batch):
    """The reactivities of a --shape file, one float array per sequence (NaN: no data): lines `position reactivity`, 1-based.  With
    `batch` one block per sequence, each introduced by a `>name` line, in the sequences' order; else one block, no `>` line needed."""
    import numpy as np
    blocks, cur = [], None
    for n, l in enumerate(open(path), 1):
        l = l.strip()
        if not l or l.startswith("#"):
            continue
        if l.startswith(">"):
            cur = []
            blocks.append(cur)
            continue
        if cur is None:
            if batch:
                raise SystemExit(f"{path}:{n}: with --batch every block of --shape begins with a `>name` line")
            cur = []
            blocks.append(cur)
        f = l.split()
        try:
            cur.append((int(f[0]), float(f[1])))
        except (ValueError, IndexError):
            raise SystemExit(f"{path}:{n}: --shape expects `position reactivity`")
    if not blocks and not batch:
        blocks.append([])
    if len(blocks) != len(lens):
        raise SystemExit(f"{path}: {len(blocks)} blocks of reactivities for {len(lens)} sequences")
    out = []
    for k, (block, L) in enumerate(zip(blocks, lens)):
        r = np.full(L, np.nan)
        for pos, val in block:
            if not 1 <= pos <= L:
                raise SystemExit(f"{path}: position {pos} outside sequence {k} of {L} nt")
            r[pos - 1] = val
        out.append(r)
    return out


def format_mfe_constrained_line(sequence, struct):
    """the line of --mfe and the pseudo-energy of the structure in kcal/mol"""
    return f"{format_mfe_line(sequence, struct)} {struct.pseudo_dcal / 100.0}"


def main_mfe(args, seqs, known, names, mfe_batch=None, scorer=None, constraints=None, mfe_constrained_batch=None):
    """--mfe: the MFE structures instead of the fold.  `scorer`: the callable (rows per sequence, known) -> score table that stands
    in for scoring.score_rows_gpu.  With -C (`constraints`: one string per sequence) or --shape the constrained fold."""
    if args.kin or args.traj:
        raise SystemExit("--mfe gives one structure per sequence: no --kin, no --traj")
    line = format_mfe_line
    if args.constraint or args.shape is not None:
        soft = None
        if args.shape is not None:
            from .zuker import shape_deigan
            soft = [shape_deigan(r, args.shape_slope, args.shape_intercept) for r in read_shape(args.shape, [len(s) for s in seqs], args.batch)]
        if mfe_constrained_batch is None:
            from .zuker import mfe_constrained_batch
        mfe_batch = lambda sequences, temp: mfe_constrained_batch(sequences, constraints, None, soft, temp)
        line = format_mfe_constrained_line
    if mfe_batch is None and args.span is not None:
        from .zuker import mfe_span_batch
        mfe_batch = lambda sequences, temp: mfe_span_batch(sequences, args.span, temp)
    if mfe_batch is None:
        from .zuker import mfe_batch
    structs = mfe_batch(seqs, args.temp)
    if args.scores:
        if scorer is None:
            from .scoring import score_rows_gpu as scorer
        beams = [[st] for st in structs]
        write_scores(args.scores, seqs, names, beams, scorer(beams, known), "energy")
        if not args.output:
            return
    text = "".join(line(s, st) + "\n" for s, st in zip(seqs, structs))
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


def format_pf_line(sequence, res):
    return f"{sequence} {len(sequence)} {res.centroid} {res.energy:.2f} {res.centroid.count('(')} {res.mfe_frequency:.4g}"


def write_bpp(path, names, results, cutoff, dense=False):
    """--bpp: `name i j p` per pair with p >= cutoff, 1-based; a result's probs are banded (L, W) under --pf-span, else L x L
    (`dense`: L x L although the results hold `unpaired`: those of pf_constrained_batch)"""
    from .mccaskill import band_pairs, dense_pairs
    with open(path, "w") as out:
        for k, r in enumerate(results):
            name = names[k] if names is not None and names[k] else str(k + 1)
            banded = r.unpaired is not None and not dense   # (what pf_span_batch fills)
            for i, j, p in (band_pairs if banded else dense_pairs)(r.probs, cutoff):
                out.write(f"{name} {i + 1} {j + 1} {p:.6g}\n")


def format_cofold_line(dimer, res, binding=False):
    """the line of --cofold: `A&B len rowA&rowB energy n_inter`, with --binding `E(AB) E(A) E(B) E(AB)-E(A)-E(B)` behind it"""
    line = f"{dimer} {len(dimer) - 1} {res.row} {res.energy} {res.n_inter}"
    return line + f" {res.energy} {res.energy_a} {res.energy_b} {res.binding}" if binding else line


def main_cofold(args, cofold_batch=None):
    """--cofold: the MFE structures of dimers instead of the fold"""
    others = (args.mfe or args.pf or args.kin or args.traj or args.scores or args.findpath or args.descend or args.barriers or args.constraint
              or args.shape is not None or args.span is not None or args.pf_span is not None or args.sample is not None or args.subopt is not None
              or args.mea is not None or args.kinfold is not None)
    if others:
        raise SystemExit("--cofold gives the MFE structure of every dimer: none of the other modes, no -C, no --shape, no --span")
    if args.sequence is None and not (args.seq_file and args.batch):
        raise SystemExit("--cofold needs -s \"A&B\" or -sf FILE --batch")
    seqs, _, _ = read_records(args)
    for k, s in enumerate(seqs):
        a, _, b = s.partition("&")
        if s.count("&") != 1 or not a or not b:
            raise SystemExit(f"--cofold: record {k} ({s[:40]!r}): a dimer is written A&B, with one '&' between two strands")
    if cofold_batch is None:
        from .cofold import cofold_batch
    results = cofold_batch(seqs, args.temp, args.binding)
    txt = "".join(format_cofold_line(s, r, args.binding) + "\n" for s, r in zip(seqs, results))
    if args.output:
        with open(args.output, "w") as out:
            out.write(txt)
    else:
        sys.stdout.write(txt)


def main_pf(args, seqs, known, names, pf_batch=None, scorer=None, constraints=None, pf_constrained_batch=None):
    """--pf: centroid, ensemble free energy and MFE share instead of the fold.  `scorer` as for main_mfe.  With -C (`constraints`: one
    string per sequence) or --shape the ensemble under them; the line is that of --pf."""
    if args.mfe or args.kin or args.traj:
        raise SystemExit("--pf gives the ensemble of every sequence: no --mfe, no --kin, no --traj")
    constrained = args.constraint or args.shape is not None
    if constrained:
        soft = None
        if args.shape is not None:
            from .zuker import shape_deigan
            soft = [shape_deigan(r, args.shape_slope, args.shape_intercept) for r in read_shape(args.shape, [len(s) for s in seqs], args.batch)]
        if pf_constrained_batch is None:
            from .mccaskill import pf_constrained_batch
        pf_batch = lambda sequences, temp: pf_constrained_batch(sequences, constraints, None, soft, temp, probs=bool(args.bpp))
    if pf_batch is None and args.pf_span is not None:
        from .mccaskill import pf_span_batch
        pf_batch = lambda sequences, temp: pf_span_batch(sequences, args.pf_span, temp, probs=bool(args.bpp))
    if pf_batch is None:
        from .mccaskill import pf_batch as _pf
        pf_batch = lambda sequences, temp: _pf(sequences, temp, probs=bool(args.bpp))
    results = pf_batch(seqs, args.temp)
    if args.bpp:
        write_bpp(args.bpp, names, results, args.bpp_cutoff, dense=bool(constrained))
    if args.scores:
        if scorer is None:
            from .scoring import score_rows_gpu as scorer
        beams = [[r] for r in results]
        write_scores(args.scores, seqs, names, beams, scorer(beams, known), "energy")
        if not args.output:
            return
    text = "".join(format_pf_line(s, r) + "\n" for s, r in zip(seqs, results))
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


MEA_EXCLUSIVE = "--mea gives the maximum-expected-accuracy structure of every sequence: no --mfe, no --pf, no --subopt, no --kin, no --traj"


def check_gamma(gamma):
    import math
    if not (math.isfinite(gamma) and gamma > 0.0):
        raise SystemExit("--mea GAMMA is a positive number")


class MeaRow:
    """a MEA row as the score table takes a structure: the row and ITS energy (a MeaResult's `energy` is the ensemble's)"""
    def __init__(self, res):
        self.str_struct, self.energy = res.structure, res.energy_of_structure


def format_mea_line(sequence, res):
    return f"{sequence} {len(sequence)} {res.structure} {res.energy_of_structure:.2f} {res.mea:.4f} {res.diversity:.4f}"


def format_consensus_line(sequence, res):
    return f"{sequence} {len(sequence)} {res.structure} {res.mea:.4f} {res.diversity:.4f}"


def main_mea(args, seqs, known, names, mea_batch=None, scorer=None):
    """--mea [GAMMA]: the MEA structures instead of the fold.  `scorer` as for main_mfe."""
    check_gamma(args.mea)
    if mea_batch is None:
        from .mccaskill import mea_batch
    results = mea_batch(seqs, args.mea, args.temp)
    if args.scores:
        if scorer is None:
            from .scoring import score_rows_gpu as scorer
        beams = [[MeaRow(r)] for r in results]
        write_scores(args.scores, seqs, names, beams, scorer(beams, known), "energy")
        if not args.output:
            return
    text = "".join(format_mea_line(s, r) + "\n" for s, r in zip(seqs, results))
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


def sampled_step(structs):
    """the distinct structures of a list of samples, energy ascending, ties by row text"""
    seen = {}
    for st in structs:
        seen.setdefault(st.str_struct, st)
    return sorted(seen.values(), key=lambda st: (st.dcal, st.str_struct))


def main_sample(args, seqs, known, names, sample_batch=None, scorer=None):
    """--sample N: structures drawn from the ensemble instead of the fold.  `scorer` as for main_mfe."""
    if args.mfe or args.pf or args.kin or args.traj:
        raise SystemExit("--sample gives structures drawn from the ensemble of every sequence: no --mfe, no --pf, no --kin, no --traj")
    if args.sample < 1:
        raise SystemExit("--sample needs a positive number of structures")
    if args.mea is not None:
        check_gamma(args.mea)
        if args.descend:
            raise SystemExit("--sample N --mea gives the consensus of the sampled rows: no --descend")
    if sample_batch is None:
        from .mccaskill import sample_batch
    samples = sample_batch(seqs, args.sample, args.seed, args.temp)
    if args.descend:
        text = descend_steps(args, seqs, samples)
    elif args.scores:
        if scorer is None:
            from .scoring import score_rows_gpu as scorer
        write_scores(args.scores, seqs, names, samples, scorer(samples, known), args.select)
        if not args.output:
            return
    if args.mea is not None:
        from .mccaskill import mea_from_probs, pair_frequencies
        consensus = mea_from_probs([pair_frequencies(sm) for sm in samples], args.mea)
        text = "".join(format_consensus_line(s, r) + "\n" for s, r in zip(seqs, consensus))
    elif not args.descend:
        from .utils import format_trajectory
        text = "".join(format_trajectory(s, [sampled_step(sm)]) for s, sm in zip(seqs, samples))
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


def descend_steps(args, seqs, lists, minima_batch=None):
    """with --descend: per sequence the text of a one-step graph of the distinct minima the structures of lists[s] walk down to,
    energy ascending (then by first appearance), each with the number of structures in its basin"""
    if args.scores:
        raise SystemExit("--descend gives the local minima of the structures: no --scores")
    if minima_batch is None:
        from .descend import minima_batch
    got = minima_batch(seqs, [[st.str_struct for st in sm] for sm in lists], args.temp, args.max_steps)
    out = []
    for s, (minima, counts, _) in zip(seqs, got):
        out.append("".join([s + "\n", "# {:-^20}\n".format(0)] + [f"{m.str_struct} {m.energy:6.1f} {c}\n" for m, c in zip(minima, counts)]))
    return "".join(out)


def read_descend_records(path):
    """(names, sequences, rows) of a --descend file: per record an optional `>name` line, the sequence, one or more dot-bracket lines"""
    names, seqs, rows = [], [], []
    name = None
    for ln in open(path):
        ln = ln.strip()
        if not ln:
            continue
        if ln.startswith(">"):
            name = ln
        elif set(ln) <= set("().") and seqs and name is None:
            rows[-1].append(ln)
        else:
            names.append(name); seqs.append(ln.replace("T", "U")); rows.append([])
            name = None
    if name is not None or any(not r for r in rows):
        raise SystemExit(f"{path}: a record is an optional `>name` line, the sequence and one or more dot-bracket lines")
    return names, seqs, rows


def main_descend(args, minima_batch=None):
    """--descend alone: the local minima the structures of every record walk down to"""
    if args.mfe or args.pf or args.kin or args.traj or args.scores:
        raise SystemExit("--descend gives the local minima of given structures: no --mfe, no --pf, no --kin, no --traj, no --scores")
    if args.seq_file is None:
        raise SystemExit("--descend needs -sf FILE with records of a sequence and its structures, or --sample N / --subopt DELTA")
    names, seqs, rows = read_descend_records(args.seq_file)
    if minima_batch is None:
        from .descend import minima_batch
    lines = []
    for k, (minima, counts, _) in enumerate(minima_batch(seqs, rows, args.temp, args.max_steps)):
        if names[k]:
            lines.append(names[k])
        lines.append(seqs[k])
        lines += [f"{m.str_struct} {m.dcal / 100.0:7.2f} {c}" for m, c in zip(minima, counts)]
    text = "".join(ln + "\n" for ln in lines)
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


SUBOPT_EXCLUSIVE = "--subopt gives every structure of every sequence within an energy band: no --mfe, no --pf, no --sample, no --kin, no --traj"


def main_subopt(args, seqs, known, names, subopt_batch=None, scorer=None):
    """--subopt DELTA: the structures within DELTA kcal/mol of the minimum instead of the fold.  `scorer` as for main_mfe."""
    if args.mfe or args.pf or args.sample is not None or args.kin or args.traj:
        raise SystemExit(SUBOPT_EXCLUSIVE)
    if not args.subopt >= 0.0:
        raise SystemExit("--subopt needs an energy band of 0 kcal/mol or more")
    if args.max_structs < 1:
        raise SystemExit("--max-structs needs a positive number of structures")
    if subopt_batch is None:
        from .wuchty import subopt_batch
    if args.barriers:
        return main_barriers(args, seqs, names)
    bands = subopt_batch(seqs, args.subopt, args.max_structs, args.temp)
    if args.descend:
        text = descend_steps(args, seqs, bands)
    elif args.scores:
        if scorer is None:
            from .scoring import score_rows_gpu as scorer
        write_scores(args.scores, seqs, names, bands, scorer(bands, known), args.select)
        if not args.output:
            return
    if not args.descend:
        from .utils import format_trajectory
        text = "".join(format_trajectory(s, [list(band)]) for s, band in zip(seqs, bands))          # (the library's order)
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


def main_barriers(args, seqs, names, barrier_trees=None):
    """--subopt DELTA --barriers: the barrier tree of every sequence's band instead of the band"""
    if args.descend or args.scores:
        raise SystemExit("--barriers gives the barrier tree of every band: no --descend, no --scores")
    if not args.minh >= 0.0:
        raise SystemExit("--minh needs a barrier height of 0 kcal/mol or more")
    if barrier_trees is None:
        from .barriers import barrier_trees
    trees = barrier_trees(seqs, args.subopt, args.max_structs, args.temp)
    text = []
    for k, (s, t) in enumerate(zip(seqs, trees)):
        if names is not None and names[k]:
            text.append(f">{names[k]}\n")
        text.append(s + "\n" + (t.prune(args.minh) if args.minh > 0 else t).format())
    text = "".join(text)
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


def read_findpath_records(path):
    """(names, sequences, starts, ends) of a --findpath file: per record an optional `>name` line, then sequence, start, end"""
    names, seqs, starts, ends = [], [], [], []
    name, cur = None, []
    for ln in open(path):
        ln = ln.strip()
        if not ln:
            continue
        if ln.startswith(">"):
            if cur:
                raise SystemExit(f"{path}: `{ln}` inside a record (a record is sequence, start, end)")
            name = ln
            continue
        cur.append(ln)
        if len(cur) == 3:
            names.append(name); seqs.append(cur[0].replace("T", "U")); starts.append(cur[1]); ends.append(cur[2])
            name, cur = None, []
    if cur:
        raise SystemExit(f"{path}: the last record is incomplete (a record is sequence, start, end)")
    return names, seqs, starts, ends


def main_findpath(args, findpath_batch=None):
    """--findpath: a low-barrier direct path between the two structures of every record instead of the fold"""
    if args.mfe or args.pf or args.sample is not None or args.subopt is not None or args.kin or args.traj or args.scores:
        raise SystemExit("--findpath gives a folding path between two given structures: no --mfe, no --pf, no --sample, no --subopt, no --kin, no --traj, no --scores")
    if args.seq_file is None:
        raise SystemExit("--findpath needs -sf FILE with records of sequence, start structure, end structure")
    if not 1 <= args.width <= 1024:
        raise SystemExit("--width is 1 .. 1024")
    names, seqs, starts, ends = read_findpath_records(args.seq_file)
    from .findpath import path_rows
    if findpath_batch is None:
        from .findpath import findpath_batch
    recs, moves, dcal = findpath_batch(seqs, starts, ends, args.width, args.both, args.temp)
    lines = []
    for k, s in enumerate(seqs):
        if names[k]:
            lines.append(names[k])
        lines.append(s)
        lines += [f"{row} {e / 100.0:7.2f}" for row, e in zip(path_rows(starts[k], moves[k]), dcal[k].tolist())]
        lines.append(f"saddle {recs[k]['saddle_dcal'] / 100.0:.2f} barrier {(recs[k]['saddle_dcal'] - recs[k]['start_dcal']) / 100.0:.2f} kcal/mol")
    text = "".join(ln + "\n" for ln in lines)
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


def kinfold_grid(t_max, k):
    """k log-spaced times ending at t_max, three decades (one time: t_max itself)"""
    return [t_max * 10.0 ** (-3.0 * (k - 1 - t) / max(k - 1, 1)) for t in range(k)]


def main_kinfold(args, seqs, names, kinfold_batch=None, mfe_batch=None):
    """--kinfold N: stochastic folding trajectories of every sequence from the open chain instead of the fold"""
    if (args.mfe or args.pf or args.sample is not None or args.subopt is not None or args.kin or args.traj or args.scores or args.descend
            or args.barriers):
        raise SystemExit("--kinfold gives folding trajectories of every sequence: no --mfe, no --pf, no --sample, no --subopt, no --kin, no --traj, "
                         "no --scores, no --descend")
    if not args.batch or args.seq_file is None:
        raise SystemExit("--kinfold needs -sf FILE --batch")
    if args.kinfold < 1:
        raise SystemExit("--kinfold needs a positive number of trajectories")
    if args.tmax is None or not args.tmax >= 0.0 or args.tmax == float("inf"):
        raise SystemExit("--kinfold needs --tmax T, a finite time of 0 or more")
    if args.times < 0:
        raise SystemExit("--times is 0 or more")
    import numpy as np
    from . import _native as N
    stops = None
    if args.stop == "mfe":
        if mfe_batch is None:
            from .zuker import mfe_batch
        stops = [m.str_struct for m in mfe_batch(seqs, args.temp)]
    elif args.stop is not None:
        stops = [ln.strip() for ln in open(args.stop) if ln.strip()]
        if len(stops) != len(seqs):
            raise SystemExit(f"{args.stop}: {len(stops)} structures for {len(seqs)} sequences")
    if kinfold_batch is None:
        from .kinfold import kinfold_batch
    grid = kinfold_grid(args.tmax, args.times)
    got = kinfold_batch(seqs, [[None]] * len(seqs), args.tmax, n_rep=args.kinfold, watch=[[st] for st in stops] if stops else None,
                        n_stop=1 if stops else None, seeds=args.seed, sample_times=grid, temp=args.temp, max_steps=args.max_steps)
    stop_dcal = None
    if stops:
        from .rafft import eval_structures
        stop_dcal, _ = eval_structures(seqs, stops, temp=args.temp)
    lines = []
    for k, (s, d) in enumerate(zip(seqs, got)):
        if names is not None and names[k]:
            lines.append(names[k])
        lines.append(s)
        if stops:
            lines.append(f"{stops[k]} {stop_dcal[k] / 100.0:7.2f}")
        hit = (d["flags"] & N.KF_STOP) != 0
        t = d["time"][hit]
        lines.append(f"arrived {hit.mean():.4f}" + (f" median {np.median(t):.6g} mean {t.mean():.6g}" if len(t) else ""))
        for ti, tau in enumerate(grid):
            at = d["samples"][:, ti, :]
            lines.append(f"{tau:.6g} {at[:, 0].mean() / 100.0:.4f} {(hit & (d['time'] <= tau)).mean():.4f}")
    text = "".join(ln + "\n" for ln in lines)
    if args.output:
        with open(args.output, "w") as out:
            out.write(text)
    else:
        sys.stdout.write(text)


def _table_note():
    """one line on stderr when the fold used rule / model values of the built-in tables (never with ViennaRNA's own tables loaded)"""
    try:
        from .rafft import last_stats
        st = last_stats()
    except Exception:
        return
    import os
    if st.get("n_kept_guessed", 0) > 0 and not os.environ.get("RAFFT_QUIET"):
        sys.stderr.write(f"rafft: built-in energy tables - {st['n_dE_guessed']} of {st['n_dE_evals']} stem energies ({st['n_kept_guessed']} kept "
                         "candidates) read an interior-loop entry that no published energy pins; set RAFFT_PARAMS=<ViennaRNA parameter file> "
                         "for ViennaRNA's own values (RAFFT_QUIET=1 silences this)\n")


def main(argv=None, fold_batch=None, scorer=None, kinetics=None, mfe_batch=None, pf_batch=None, sample_batch=None, subopt_batch=None, mea_batch=None,
         mfe_constrained_batch=None, pf_constrained_batch=None, cofold_batch=None):
    """`cofold_batch`: the callable (dimers, temp, monomers) that stands in for cofold.cofold_batch.  `fold_batch` / `scorer` / `kinetics` / `mfe_batch` / `pf_batch` / `sample_batch` / `subopt_batch`: injection points for tests (the fold, the
    callable (results, known) -> score table that stands in for scoring.score_batch_gpu - with --mfe, --pf and --sample for
    scoring.score_rows_gpu -, the callable (results, max_time, n_steps) that stands in for rafft_kin.kinetics_batch, the callable
    (sequences, temp) that stands in for zuker.mfe_batch, the callable (sequences, temp) that stands in for mccaskill.pf_batch,
    the callable (sequences, n_samples, seed, temp) that stands in for mccaskill.sample_batch, and the callable (sequences, delta,
    max_structs, temp) that stands in for wuchty.subopt_batch; `mea_batch`: the callable (sequences, gamma, temp) that stands in for
    mccaskill.mea_batch; `mfe_constrained_batch`: the callable (sequences, constraints, soft_unpaired, soft_stack, temp) that stands in
    for zuker.mfe_constrained_batch; `pf_constrained_batch`: the callable (sequences, constraints, soft_unpaired, soft_stack, temp,
    probs=) that stands in for mccaskill.pf_constrained_batch)."""
    args = parse_arguments(argv)
    if (args.constraint or args.shape is not None) and not (args.mfe or args.pf):
        raise SystemExit("-C and --shape FILE constrain the fold of --mfe or the ensemble of --pf: they need --mfe or --pf")
    if (args.constraint or args.shape is not None) and args.span is not None:
        raise SystemExit("-C and --shape FILE do not combine with --span")
    if (args.constraint or args.shape is not None) and args.pf_span is not None:
        raise SystemExit("-C and --shape FILE do not combine with --pf-span")
    if args.span is not None and not args.mfe:
        raise SystemExit("--span W restricts the pairs of --mfe: it needs --mfe")
    if args.span is not None and not 1 <= args.span <= 4096:
        raise SystemExit("--span is 1 to 4096")
    if (args.pf_span is not None or args.bpp) and not args.pf:
        raise SystemExit("--pf-span W and --bpp FILE belong to --pf: they need --pf")
    if args.pf_span is not None and not 1 <= args.pf_span <= 4096:
        raise SystemExit("--pf-span is 1 to 4096")
    if args.binding and not args.cofold:
        raise SystemExit("--binding adds the strands' energies to the lines of --cofold: it needs --cofold")
    if args.cofold:
        return main_cofold(args, cofold_batch)
    if args.findpath:
        if args.descend:
            raise SystemExit("--findpath and --descend are two modes")
        return main_findpath(args)
    if args.max_steps < 0:
        raise SystemExit("--max-steps is 0 or more")
    if args.barriers and args.subopt is None:
        raise SystemExit("--barriers needs --subopt DELTA: the tree is that of the band")
    if args.descend and args.sample is None and args.subopt is None:
        return main_descend(args)
    constraints = None
    if args.constraint and args.sequence is not None:
        seqs, known, names, constraints = [args.sequence], None, None, [read_constraint_line()]
    elif args.constraint and args.scores:              # the CSV of --scores (with a header line) carries the constraints in a column `constraint`
        import csv
        seqs, known, names = read_records(args)
        with open(args.seq_file, newline="") as fh:
            rd = csv.DictReader(fh)
            if "constraint" not in (rd.fieldnames or []):
                raise SystemExit(f"{args.seq_file}: -C with --scores needs a column 'constraint' (columns: {rd.fieldnames})")
            constraints = [(r["constraint"] or "").strip() for r in rd if r[args.csv_column].strip()]
    elif args.constraint:
        seqs, constraints, names = read_constrained_fasta(args.seq_file)
        known = None
    else:
        seqs, known, names = read_records(args)
    if args.kinfold is not None:
        return main_kinfold(args, seqs, names)
    if args.mea is not None and (args.mfe or args.pf or args.subopt is not None or args.kin or args.traj):
        raise SystemExit(MEA_EXCLUSIVE)
    if args.subopt is not None and (args.mfe or args.pf or args.sample is not None or args.kin or args.traj):
        raise SystemExit(SUBOPT_EXCLUSIVE)
    if args.sample is not None and (args.mfe or args.pf or args.kin or args.traj):
        raise SystemExit("--sample gives structures drawn from the ensemble of every sequence: no --mfe, no --pf, no --kin, no --traj")
    if args.pf and (args.mfe or args.kin or args.traj):
        raise SystemExit("--pf gives the ensemble of every sequence: no --mfe, no --kin, no --traj")
    if args.kin:
        if not args.batch or args.seq_file is None:
            raise SystemExit("--kin needs -sf FILE --batch")
        args.traj = True
    if args.scores:
        if not args.batch or known is None:
            raise SystemExit("--scores needs -sf CSV --batch with a known structure per sequence "
                             f"(column {args.known_column!r}, or the headerless seq,struct,name file)")
        names = names if names is not None else [""] * len(seqs)
    if args.subopt is not None:
        return main_subopt(args, seqs, known, names, subopt_batch, scorer)
    if args.sample is not None:
        return main_sample(args, seqs, known, names, sample_batch, scorer)
    if args.mea is not None:
        return main_mea(args, seqs, known, names, mea_batch, scorer)
    if args.pf:
        return main_pf(args, seqs, known, names, pf_batch, scorer, constraints, pf_constrained_batch)
    if args.mfe:
        return main_mfe(args, seqs, known, names, mfe_batch, scorer, constraints, mfe_constrained_batch)
    if fold_batch is None:
        from .rafft import fold_batch
    results = fold_batch(seqs, args.n_mode, args.max_stack, args.max_branch, args.min_hp, args.min_nrj, args.traj,
                         args.temp, args.gc_wei, args.au_wei, args.gu_wei)
    if args.scores:
        if scorer is None:
            from .scoring import score_batch_gpu as scorer
        write_scores(args.scores, seqs, names, results, scorer(results, known), args.select, args.traj)
        if not args.output:          # the table is the output; the structures are written as well when -o names a file
            _table_note()
            return
    if args.kin:
        if kinetics is None:
            from .rafft_kin import kinetics_batch as kinetics
        write_kinetics(args.kin, seqs, kinetics(results if hasattr(results, "raw") else [r[1] for r in results], args.max_time, args.n_steps))
        if not args.output:          # the tables are the output; the graphs are written as well when -o names a file
            _table_note()
            return
    out = open(args.output, "wb") if args.output else sys.stdout.buffer if hasattr(sys.stdout, "buffer") else None
    try:
        for k, s in enumerate(seqs):
            side = (args.sidecar if len(seqs) == 1 else f"{args.sidecar}.{k}") if (args.sidecar and args.traj) else None
            raw = results.raw(k) if hasattr(results, "raw") and out is not None else None
            if raw is not None:       # streaming: flat result buffers -> text, no Structure objects
                from .utils import write_result_text, write_sidecar_raw
                write_result_text(out, s, raw, traj=args.traj, bench=args.bench)
                if side:
                    write_sidecar_raw(side, s, raw)
            else:                     # an injected fold function (tests) or a captured text stdout
                txt = format_result(s, results[k], args) + "\n"
                if out is not None:
                    out.write(txt.encode("ascii"))
                else:
                    sys.stdout.write(txt)
                if side:
                    from .utils import write_sidecar
                    write_sidecar(side, s, results[k][1])
        if out is not None:
            out.flush()
        _table_note()
    finally:
        if args.output:
            out.close()


if __name__ == '__main__':
    main()
