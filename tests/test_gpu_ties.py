"""Tie-heavy, low-complexity sequences (repeats) through every expand class and the beam step, on a real MI355X (`-m gpu`).

On i.i.d. sequences the parallel code almost never has to break a tie; on CUG / GC / tandem-hairpin repeats nearly every
decision is one: "the 100 largest of 1099 equal lag values" (radix-select cut, bitonic rank, the skip path when
2n-1 <= nb_mode), the `>=` arg-max of window_slide over long identical runs (bit-mask and chunked forms), the max_stack cut of
the beam inside a run of equal energies, `seen` deduplication of one structure reached by many orders of the same stems.
Expected values: fixtures made by the reference's own Python and by the oracle (tools/make_golden_ties.py; the oracle is pinned
to them on the CPU by tests/test_ties.py), and the oracle itself.  Integers and bit-equal fp64 throughout: no tolerance."""
import pytest

import oracle
import rafft_amd
from rafft_amd import rafft as R
from conftest import load_json_gz

pytestmark = pytest.mark.gpu

FAMILIES = ("GC", "AU", "GU", "CUG", "GGGAAACCC", "GGGGCCCC", "GC+A", "GC+N5")
# both sides of every class edge: small teams of 16 / 32 lanes, 2n-1 crossing nb_mode = 100 (50 | 51), one wavefront (<= 256),
# 256 threads (<= 1024), the FFT-free / FFT plans (<= 4096), and a sequence too long for the LDS copy of the bases (4097)
EDGE_N = (16, 17, 32, 33, 50, 51, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 4096, 4097)
PAIRS = {"GC", "CG", "AU", "UA", "GU", "UG"}
KEYS = ("lag", "cor", "nb", "mi", "mj", "score", "ddcal", "kept")


@pytest.fixture(autouse=True, params=["classes_by_size", "classes_merged", "general_builds"])
def expand_class_routing(request, monkeypatch):
    """the three routings of tests/test_gpu_parity.py: every region to the class of its size, the regions of steps with few new
    structures merged into one wide class, and the general builds of the expand kernels instead of the production builds"""
    if request.param in ("classes_by_size", "general_builds"):
        monkeypatch.setenv("RAFFT_MERGE_BELOW", "0")
        monkeypatch.setenv("RAFFT_MERGE2_BELOW", "0")
    if request.param == "general_builds":
        monkeypatch.setenv("RAFFT_PROD", "0")
    yield


def family(name, L):
    """the unit repeated and cut to L nt; `GC+A`: one A at L//2, `GC+N5`: five N from L//3 (tools/make_golden_ties.py)"""
    unit = name.split("+")[0]
    s = (unit * (L // len(unit) + 1))[:L]
    if name == "GC+A":
        s = s[:L // 2] + "A" + s[L // 2 + 1:]
    if name == "GC+N5":
        s = s[:L // 3] + "NNNNN" + s[L // 3 + 5:]
    return s


def as_lists(traj):
    return [[[s.str_struct, s.dcal] for s in st] for st in traj]


def beam(structs):
    return [(s.str_struct, s.dcal) for s in structs]


def assert_no_step_lists_a_structure_twice(traj, what):
    for k, st in enumerate(traj):
        assert len({db for db, _ in st}) == len(st), (what, k)


# the oracle's answers are computed once and shared by the three routings (and by the tests that look at the same region)
_ORACLE_NODES, _ORACLE_BEAMS = {}, {}


def oracle_node(seq, db, pos, nb_mode):
    key = (seq, db, pos[0], pos[-1], len(pos), nb_mode)      # (a region of these tests is all unpaired positions of one loop)
    if key not in _ORACLE_NODES:
        _ORACLE_NODES[key] = oracle.expand_node(seq, db, pos, nb_mode)
    return _ORACLE_NODES[key]


def oracle_beams(seqs, ms, mb):
    from _oracle_pool import fold_many
    todo = [s for s in seqs if (s, ms, mb) not in _ORACLE_BEAMS]
    for s, b in zip(todo, fold_many([(s, 100, ms, mb, False) for s in todo])):
        _ORACLE_BEAMS[(s, ms, mb)] = b
    return [_ORACLE_BEAMS[(s, ms, mb)] for s in seqs]


def root_nb_modes(n):
    """1 and 7 cut inside the tie group of a repeat, 100 is the default, 101 is odd, the last takes every lag (as far as the
    LDS plans allow: below 2048, and below ~400 for a sequence of more than 4096 nt - rafft_plan.h)"""
    return sorted({1, 7, 100, 101, 399 if n > 4096 else min(2 * n - 1, 2047)})


def split(seq, a0, b0, k):
    """a dot-bracket with ONE stem of k pairs joining [a, a+k) to (b-k, b], a >= a0 and b <= b0 the first place where the bases
    pair -> (db, the non-contiguous exterior region [0, a) u (b, L), the interior region)"""
    L = len(seq)
    for k in range(k, 0, -1):              # (a CUG repeat has no three stacked pairs anywhere: U.U every third - then two)
        for a in range(a0, L):
            for b in range(b0, a + 2 * k + 2, -1):
                if all(seq[a + i] + seq[b - i] in PAIRS for i in range(k)):
                    db = "." * a + "(" * k + "." * (b - a - 2 * k + 1) + ")" * k + "." * (L - 1 - b)
                    assert len(db) == L and a >= 1 and b <= L - 2
                    return db, list(range(a)) + list(range(b + 1, L)), list(range(a + k, b - k + 1))
    raise AssertionError("no stem")


def splits(n):
    """a wide loop, a stem next to both ends (two-position exterior region), a small hairpin in the middle (long exterior region)"""
    return ((n // 5, n - 1 - n // 7, 3), (1, n - 2, 1), (n // 2 - 9, n // 2 + 12, 2))


def assert_node_equal(g, o, what):
    for key in KEYS:
        assert g[key] == o[key], (what, key)


# ---- 3a. folds against the reference's Python

@pytest.fixture(scope="module")
def tie_cases():
    return load_json_gz("fold_traj_ties.json.gz")


@pytest.fixture(scope="module")
def tie_records():
    return load_json_gz("node_expand_ties.json.gz")


def test_gpu_fold_ties_vs_reference_python(tie_cases):
    """full trajectories of every tie fixture case, batched per parameter set; then, for the GPU's output by itself: no step
    holds a structure twice (`seen` under many orders of the same stems), and the energy every final structure arrived at by
    incremental dE is the whole-structure evaluator's"""
    groups = {}
    for c in tie_cases:
        groups.setdefault(tuple(sorted(c["params"].items())), []).append(c)
    seqs, dbs, dcals = [], [], []
    for key, cases in groups.items():
        got = rafft_amd.fold_batch([c["seq"] for c in cases], traj=True, **dict(key))
        for c, (fin, traj) in zip(cases, got):
            t = as_lists(traj)
            what = (c["family"], len(c["seq"]), c["params"])
            assert t == c["traj"], what
            assert_no_step_lists_a_structure_twice(t, what)
            for db, dcal in t[-1]:
                seqs.append(c["seq"]), dbs.append(db), dcals.append(dcal)
    got, status = R.eval_structures(seqs, dbs)
    assert not any(status)
    assert got == dcals


# ---- 3b. single regions against the reference's Python and the oracle

def test_gpu_expand_node_ties_vs_reference_python_and_oracle(tie_records):
    for r in tie_records:
        args = (r["seq"], r["db"], r["pos"], r["nb_mode"], r["min_hp"], r["min_nrj"], r["gc"], r["au"], r["gu"])
        g = R.expand_node(*args)
        o = oracle.expand_node(*args)
        what = (r["family"], len(r["seq"]), r["db"])
        assert g["lag"] == r["lags"] == o["lag"], what
        assert g["cor"] == [r["cor"][k] for k in r["lags"]], what        # bit-exact fp64: integer counts, IEEE divide
        assert [[a, b, c, d] for a, b, c, d in zip(g["nb"], g["mi"], g["mj"], g["score"])] == r["ws"], what
        assert g["ddcal"] == o["ddcal"], what
        assert g["kept"] == o["kept"], what
        assert [[g["nb"][k], g["score"][k], g["mi"][k], g["mj"][k], g["ddcal"][k]] for k in g["kept"]] == r["sol"], what


# ---- 3c. root and split regions at every class edge against the oracle

@pytest.mark.parametrize("n", EDGE_N)
def test_gpu_root_regions_at_class_edges_vs_oracle(n):
    for fam in FAMILIES:
        seq, db, pos = family(fam, n), "." * n, list(range(n))
        for nb_mode in root_nb_modes(n):
            assert_node_equal(R.expand_node(seq, db, pos, nb_mode), oracle_node(seq, db, pos, nb_mode), (fam, n, nb_mode))


@pytest.mark.parametrize("n", [n for n in EDGE_N if n >= 64])
def test_gpu_split_regions_at_class_edges_vs_oracle(n):
    """the loops on both sides of one stem: the exterior region is non-contiguous, the interior one starts inside the sequence;
    nb_mode 7 cuts inside tie groups, 100 is the default"""
    for fam in FAMILIES:
        seq = family(fam, n)
        for a0, b0, k in splits(n):
            db, ext, inner = split(seq, a0, b0, k)
            for pos in (ext, inner):
                for nb_mode in (7, 100):
                    assert_node_equal(R.expand_node(seq, db, pos, nb_mode), oracle_node(seq, db, pos, nb_mode),
                                      (fam, n, db.index("("), db.rindex(")"), k, len(pos), nb_mode))


# ---- 3d. the f32 FFT on spectra concentrated in a few bins

@pytest.mark.parametrize("fft", ["one_wavefront_forced", "wide_plans"])
@pytest.mark.parametrize("n", [n for n in EDGE_N if n <= 4096])
def test_gpu_fft_on_periodic_sequences_rounds_to_exact_counts(monkeypatch, n, fft):
    """a periodic sequence puts its whole spectrum into a few bins - the hardest input for the claim that the f32 FFT rounds to
    exact integer pair counts.  RAFFT_FORCE_FFT=1: the one-wavefront class; RAFFT_DIRECT_N=0 with RAFFT_C3_DIRECT=0: the FFT
    plans of the wide classes.  Values and ranks bit-equal to the default run and to the oracle, at nb_mode 100 and with every
    lag ranked (up to the 2047 the LDS plans allow)."""
    roots = [(fam, family(fam, n), nb_mode) for fam in FAMILIES for nb_mode in sorted({100, min(2 * n - 1, 2047)})]
    db, pos = "." * n, list(range(n))
    default = [R.expand_node(seq, db, pos, nb_mode) for _, seq, nb_mode in roots]
    if fft == "one_wavefront_forced":
        monkeypatch.setenv("RAFFT_FORCE_FFT", "1")
    else:
        monkeypatch.setenv("RAFFT_DIRECT_N", "0")
        monkeypatch.setenv("RAFFT_C3_DIRECT", "0")
    for (fam, seq, nb_mode), d in zip(roots, default):
        g = R.expand_node(seq, db, pos, nb_mode)
        o = oracle_node(seq, db, pos, nb_mode)
        assert g["cor"] == d["cor"] == o["cor"], (fam, n, nb_mode)
        assert g["lag"] == d["lag"] == o["lag"], (fam, n, nb_mode)
        assert_node_equal(g, o, (fam, n, nb_mode))


@pytest.mark.parametrize("fft", ["one_wavefront_forced", "wide_plans"])
def test_gpu_fold_ties_with_fft_correlation(monkeypatch, tie_cases, long_cases, fft):
    """(the seam above always correlates regions of more than 64 positions by the FFT; a fold by default never does below 1025)
    the fixture folds at the default parameters and the cheap long ones, with the FFT in place of the popcount forms"""
    if fft == "one_wavefront_forced":
        monkeypatch.setenv("RAFFT_FORCE_FFT", "1")
    else:
        monkeypatch.setenv("RAFFT_DIRECT_N", "0")
        monkeypatch.setenv("RAFFT_C3_DIRECT", "0")
    base = dict(nb_mode=100, max_stack=20, max_branch=1000)
    cases = [c for c in tie_cases if c["params"] == base]
    for c, (fin, traj) in zip(cases, rafft_amd.fold_batch([c["seq"] for c in cases], traj=True, **base)):
        assert as_lists(traj) == c["traj"], (c["family"], len(c["seq"]))
    cases = [c for c in long_cases if c["family"] != "CUG" and len(c["seq"]) <= 1500]
    for c, (fin, traj) in zip(cases, rafft_amd.fold_batch([c["seq"] for c in cases], traj=True, **cases[0]["params"])):
        assert as_lists(traj) == c["traj"], (c["family"], len(c["seq"]))


# ---- 3e. beam ties across beam widths

BEAM_SEQS = [family("CUG", 130), family("GGGAAACCC", 130)]


@pytest.mark.parametrize("mb", [1000, 7])
@pytest.mark.parametrize("ms", [1, 7, 50, 300, 700])
def test_gpu_beam_cut_inside_equal_energies_vs_oracle(monkeypatch, ms, mb):
    """the max_stack cut of a beam whose members come in long runs of equal energy (347 adjacent equal pairs in the CUG fold
    at max_stack 20): one member, fewer than a wavefront, about a wavefront, and more than the 256-thread workgroup holds (the
    several-rounds beam step, RAFFT_WIDE_BELOW=0); few children per step (max_branch 7) moves the cut again"""
    if ms >= 300:
        monkeypatch.setenv("RAFFT_WIDE_BELOW", "0")
    want = oracle_beams(BEAM_SEQS, ms, mb)
    got = rafft_amd.fold_batch(BEAM_SEQS, 100, ms, mb)
    for k, s in enumerate(BEAM_SEQS):
        assert beam(got[k]) == want[k], (k, ms, mb)
        assert len({db for db, _ in want[k]}) == len(want[k])


@pytest.mark.parametrize("ms", [50, 700])
def test_gpu_seen_rehash_under_duplicate_pressure(monkeypatch, ms):
    """the same folds with every `seen` set starting in the smallest table (RAFFT_SEEN_FIXED=1): on a repeat one structure is
    reached by many orders of the same stems, so the set is rehashed while nearly every probe is a duplicate"""
    want = oracle_beams(BEAM_SEQS, ms, 1000)
    base = [beam(b) for b in rafft_amd.fold_batch(BEAM_SEQS, 100, ms, 1000)]
    monkeypatch.setenv("RAFFT_SEEN_FIXED", "1")
    fixed = [beam(b) for b in rafft_amd.fold_batch(BEAM_SEQS, 100, ms, 1000)]
    assert fixed == base == want


# ---- 3f. long tie-heavy folds against the oracle's committed trajectories

@pytest.fixture(scope="module")
def long_cases():
    return load_json_gz("fold_ties_long.json.gz")


@pytest.mark.parametrize("which", ["1100_and_1500_nt", "4200_nt_long_sequence_wave"])
def test_gpu_long_tie_heavy_folds_vs_oracle(long_cases, which):
    """GC, CUG and GGGGCCCC repeats of 1100 and 1500 nt (max_stack 4; up to 246 steps) and the GC repeat of 4200 nt
    (max_stack 2; a long-sequence wave): full trajectories"""
    cases = [c for c in long_cases if (len(c["seq"]) > 4096) == (which != "1100_and_1500_nt")]
    assert len(cases) == (6 if which == "1100_and_1500_nt" else 1)
    params = cases[0]["params"]
    assert all(c["params"] == params for c in cases)
    got = rafft_amd.fold_batch([c["seq"] for c in cases], traj=True, **params)
    for c, (fin, traj) in zip(cases, got):
        t = as_lists(traj)
        assert t == c["traj"], (c["family"], len(c["seq"]))
        assert_no_step_lists_a_structure_twice(t, (c["family"], len(c["seq"])))
