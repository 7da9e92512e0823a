"""rafft_mfe_constrained_batch on a real MI355X (`-m gpu`): the minimum of eval_kernel plus the soft terms over
every structure that satisfies the constraint, in one batch with repeated sequences and null entries; the tests' mirror of the
constrained recurrences at 60-105 nt, rows included, with candidates beyond lane 63 and must-pair positions at every edge; the same
bits in both size classes and with one sequence per chunk; the rows of rafft_mfe_batch where nothing constrains; the limits of
length and of the soft terms; other temperatures.  Integers and bytes: no tolerance."""
import numpy as np
import pytest

from rafft_amd import _native as N, params, rafft as R, zuker
import _loops as LP
import _mfe_np as MF
import _mfe_con_np as MC
import _par_reader as PR

pytestmark = pytest.mark.gpu

SEED = 79                       # of the drawn constraints, as tests/test_mfe_constrained_host.py


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    idx.update(ml_closing=-700, ml_intern=-300)
    out = dict(builtin=builtin, multiloops_win=idx, tie0=LP.tie_par(builtin, LP.TIE_ML[0]), tie1=LP.tie_par(builtin, LP.TIE_ML[1]),
               synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name in ("multiloops_win", "tie0", "tie1", "synthetic"):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=name)
    return out


def install(sets, which):
    if which == "builtin":
        params.reset_params()
    else:
        params.load_params(sets["paths"][which])


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()


def run(cases, **kw):
    """mfe_constrained_batch_raw of a list of (seq, con, u, b) cases; an array of nothing but None goes as no array at all"""
    col = lambda k: None if all(c[k] is None for c in cases) else [c[k] for c in cases]
    return zuker.mfe_constrained_batch_raw([c[0] for c in cases], col(1), col(2), col(3), **kw)


def check_rows(cases, raw, temp=37.0):
    """what holds for every result without an error: the row satisfies the constraint, its own energy is dcal - pseudo_dcal, the soft
    terms of the row are pseudo_dcal, the pair count is the row's; a sequence with an error has a row of dots and zeros"""
    rows, dcal, n_pairs, ps, status = raw
    keep = [k for k, st in enumerate(status) if st == 0]
    en, st = R.eval_structures([cases[k][0] for k in keep], [rows[k] for k in keep], temp=temp)
    assert not any(st)
    for k, e in zip(keep, en):
        s, con, u, b = cases[k]
        assert len(rows[k]) == len(s) and MC.satisfies(rows[k], con), (k, s, con, rows[k])
        assert e == dcal[k] - ps[k] and ps[k] == MC.pseudo(rows[k], u, b) and n_pairs[k] == rows[k].count("("), (k, s, con, rows[k], e, dcal[k], ps[k])
    for k, st in enumerate(status):
        if st:
            assert (rows[k], dcal[k], n_pairs[k], ps[k]) == ("." * len(cases[k][0]), 0, 0, 0)


# ---- 1. the exhaustive minimum

_INSIDE = {}


def exhaustive_batch():
    """the cases of the CPU test - hard, soft, both - and every sequence once with nothing, interleaved: one sequence appears
    fifteen times with different constraints, and null entries lie between the packs"""
    hard, soft, seqs = MC.exhaustive_cases(SEED), MC.exhaustive_cases(SEED, soft=True), MC.short_sequences()
    cases = []
    for k, s in enumerate(seqs):
        cases += hard[6 * k:6 * k + 3] + [(s, None, None, None)] + soft[7 * k:7 * k + 7] + hard[6 * k + 3:6 * k + 6] + [(s, "." * len(s), None, None)]
    return cases


@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_gpu_constrained_mfe_is_the_minimum_over_every_structure_that_satisfies_the_constraint(sets, which):
    install(sets, which)
    cases = exhaustive_batch()
    seqs = MC.short_sequences()
    assert len(cases) == 24 * 15 and sum(c[1] is None and c[2] is None for c in cases) == 24
    enum = {s: MF.enumerate_structures(s) for s in seqs}
    flat_s = [s for s in seqs for _ in enum[s]]
    en, st = R.eval_structures(flat_s, [r for s in seqs for r in enum[s]])          # every structure of every sequence, one call
    assert not any(st)
    energy, at = {}, 0
    for s in seqs:
        energy[s] = dict(zip(enum[s], en[at:at + len(enum[s])]))
        at += len(enum[s])
    want = []
    for k, (s, con, u, b) in enumerate(cases):
        if k not in _INSIDE:
            _INSIDE[k] = [(r, MC.pseudo(r, u, b)) for r in enum[s] if MC.satisfies(r, con)]
        want.append(min((energy[s][r] + p for r, p in _INSIDE[k]), default=None))
    raw = run(cases)                                                                # ONE batch
    rows, dcal, n_pairs, ps, status = raw
    assert status == [0 if w is not None else N.ERR_INFEASIBLE for w in want]
    assert [d for d, w in zip(dcal, want) if w is not None] == [w for w in want if w is not None]
    check_rows(cases, raw)
    n_inf = status.count(N.ERR_INFEASIBLE)
    assert n_inf >= 20 and status.count(0) >= 150
    first = status.index(N.ERR_INFEASIBLE)
    assert N.lib().rafft_last_error().decode() == f"sequence {first}: no structure satisfies its constraints"
    # neighbours of an infeasible case are untouched: the whole batch again, alone, case by case for a stretch of it
    a = max(first - 2, 0)
    for k in range(a, a + 6):
        one = run(cases[k:k + 1])
        assert tuple(x[0] for x in one) == tuple(x[k] for x in raw), k
    # no constraint and the all-'.' string: rafft_mfe_batch
    free = zuker.mfe_batch_raw(seqs)
    for j, s in enumerate(seqs):
        for k in (15 * j + 3, 15 * j + 14):
            assert (rows[k], dcal[k], n_pairs[k], ps[k], status[k]) == (free[0][j], free[1][j], free[2][j], 0, 0)
    assert sum(d > 0 for d, st_ in zip(dcal, status) if not st_) >= 3                # with u the open chain is no longer 0


# ---- 2. against the mirror where enumeration cannot reach

def dots(L, **at):
    con = ["."] * L
    for k, c in at.items():
        con[int(k[1:])] = c
    return "".join(con)


def adjacent_cases(seq, row):
    """A must-pair position directly inside a closing pair of `row`, the pair itself forced: | at i+1, at j-1 (the 5' and 3' side of
    the loop a pair (i,j) closes) and at p-1, q+1 (the two sides of the loop that encloses a pair (p,q)), where `row` leaves that
    position unpaired.  One case per kind, from the first pair that has one; for i+1 and j-1 a pair that encloses another pair and
    20 positions at least, so that the position can find a partner inside."""
    pt, L, out = MC.pair_table(row), len(seq), {}
    for i, j in enumerate(pt):
        if j < i:
            continue
        roomy = j - i > 20 and any(y > x for x, y in enumerate(pt[i + 1:j], i + 1))
        for kind, k in (("i+1", i + 1), ("j-1", j - 1), ("p-1", i - 1), ("q+1", j + 1)):
            inside_a_pair = any(a < k < pt[a] for a in range(min(i, k)) if pt[a] > a)
            if kind not in out and 0 <= k < L and pt[k] < 0 and (roomy if kind in ("i+1", "j-1") else inside_a_pair):
                out[kind] = (seq, dots(L, **{f"k{i}": "(", f"k{j}": ")", f"k{k}": "|"}), None, None)
    return out


def crossing_case(seq, row):
    """a forced pair that crosses a helix of at least three pairs of `row`: its 5' end in the helix's loop, its 3' end outside"""
    pt, L = MC.pair_table(row), len(seq)
    for i, j in enumerate(pt):
        if j > i and pt[i + 1] == j - 1 and pt[i + 2] == j - 2:
            for a in range(i + 3, j - 2):
                for b in range(j + 1, L):
                    if pt[a] < 0 and b - a >= 4 and seq[a] + seq[b] in MF.PAIRS:
                        return (seq, dots(L, **{f"k{a}": "(", f"k{b}": ")"}), None, None), (i, j)
    raise AssertionError("no crossing pair")


def consistent_constraint(rng, row):
    """a constraint that `row` satisfies, on every fifth position or so: x where it is unpaired, | or < at a 5' end, | or > at a 3'
    end - at 60 nt and more the density of draw_constraint leaves no structure"""
    pick = {".": "xx", "(": "|<", ")": "|>"}
    return "".join(pick[c][int(rng.integers(2))] if rng.random() < 0.2 else "." for c in row)


def mirror_cases(sets, which):
    """the (seq, con, u, b) cases of a table set at 60-105 nt and what marks them"""
    rng = np.random.default_rng(2077)
    rand = lambda n: "".join(rng.choice(list("ACGU"), n))
    marks = {}
    free = MF.Mirror(PR.tables_at(sets[which], 37.0))
    if which == "builtin":
        s60, s67, s75, s83, s90 = (rand(n) for n in (60, 67, 75, 83, 90))
        cases = [(s60, consistent_constraint(rng, free.fold(s60, "first")[1]), rng.integers(-150, 151, 60).astype(np.int32), rng.integers(-200, 101, 60).astype(np.int32)),
                 (s67, dots(67, k0="x", k66="x", k30="x"), None, None),
                 (s75, dots(75, k0="<", k74=">"), None, None),
                 (s75, dots(75, k0="<"), rng.integers(-100, 101, 75).astype(np.int32), None),
                 (s67, None, None, np.asarray(zuker.shape_deigan(rng.random(67) * 0.6)))]
        adj = {}
        for s in (s83, s90, s75):                                                   # the first sequence whose free fold has a case of a kind gives it
            adj = {**adjacent_cases(s, free.fold(s, "first")[1]), **adj}
        assert set(adj) == {"i+1", "j-1", "p-1", "q+1"}
        marks["adjacent"] = list(range(len(cases), len(cases) + 4))
        cases += [adj[k] for k in ("i+1", "j-1", "p-1", "q+1")]
        cross, helix = crossing_case(s90, free.fold(s90, "first")[1])
        marks["crossing"], marks["helix"], marks["free90"] = len(cases), helix, free.fold(s90, "first")
        cases.append(cross)
        # a hairpin of exactly 3 around a |: GGGG AUA CCCC has no hairpin candidate for its innermost pair once the U must pair
        hp = "GGGGAUACCCC"
        s = hp + rand(55)
        marks["hairpin3"] = len(cases)
        cases.append((s, dots(len(s), k5="|"), None, None))
        cases.append((s, dots(len(s), k3="(", k7=")", k5="|"), None, None))        # the pair forced as well: nothing is left
    else:
        tl = LP.tie_long_sequences()
        big, far, r100 = tl[10], tl[11], tl[3]
        assert len(big) == 105 and len(far) == 81 and len(r100) == 100
        cases = [(big, dots(105, k28="x", k29="x", k60="x", k0="<", k104=">"), None, None),      # M and C splits beyond lane 63
                 (far, dots(81, k0="<", k40="x", k80=">"), None, None),                           # the exterior stem begins at 68
                 (far, dots(81, k0="x", k80="x"), np.full(81, 7, dtype=np.int32), np.full(81, -30, dtype=np.int32)),
                 (r100, dots(100, k0="x", k99="x", k50="|"), None, None),
                 (tl[1], consistent_constraint(rng, free.fold(tl[1], "first")[1]), None, rng.integers(-200, 101, 60).astype(np.int32))]
    return cases, marks


_WANT = {}


@pytest.mark.parametrize("which", ["builtin", "tie0", "tie1"])
def test_gpu_constrained_mfe_equals_the_mirror_at_60_to_105_nt(sets, which):
    install(sets, which)
    cases, marks = mirror_cases(sets, which)
    if which not in _WANT:
        mirror = MC.ConMirror(PR.tables_at(sets[which], 37.0))
        _WANT[which] = [(mirror.fold(*c, order="first"), mirror.pseudo, dict(mirror.offsets)) for c in cases]
    want = _WANT[which]
    raw = run(cases)
    rows, dcal, n_pairs, ps, status = raw
    print("\n" + which, [(w[0][0], w[2]) for w in want])
    assert status == [0 if w[0][0] is not None else N.ERR_INFEASIBLE for w in want]
    for k, (w, pseudo, _) in enumerate(want):
        if w[0] is not None:
            assert (dcal[k], rows[k], ps[k]) == (w[0], w[1], pseudo), (which, k, cases[k][1], rows[k], w[1])
    check_rows(cases, raw)
    assert raw == run(cases, max_lds_len=4)
    off = lambda key: max(w[2][key] for w in want)
    if which == "builtin":
        assert off("I") >= 64                                                       # an interior candidate beyond lane 63 decides a cell
        assert status.count(0) >= 9
        for k in marks["adjacent"]:                                                 # the must-pair position is paired, the forced pair is there
            con = cases[k][1]
            assert status[k] == 0 and rows[k][con.index("|")] in "()" and rows[k][con.index("(")] == "("
        k = marks["crossing"]
        (i, j), (d_free, row_free) = marks["helix"], marks["free90"]
        assert status[k] == 0 and dcal[k] > d_free and row_free[i] == "(" and MC.pair_table(rows[k])[i] != j
        k = marks["hairpin3"]
        assert status[k] == 0 and rows[k][5] in "()" and MC.pair_table(rows[k])[3] != 7
        assert status[k + 1] == N.ERR_INFEASIBLE
        assert status[1] == 0 and rows[1][0] == rows[1][66] == "." and status[2] == 0 and rows[2][0] == "(" and rows[2][74] == ")"
    else:
        assert not any(status)
        assert max(off("M"), off("C")) > 64 and (which == "tie1" or off("F") >= 64)  # splits and exterior stems beyond lane 63
        assert rows[0][0] == "(" and rows[0][104] == ")" and rows[1][0] == "(" and rows[1][80] == ")" and rows[2][0] == rows[2][80] == "."


# ---- 3. the same bits in both classes and in every chunking

def test_gpu_constrained_mfe_same_bits_in_both_classes_and_every_chunking():
    rng = np.random.default_rng(5)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (33, 58, 71, 20, 64, 45, 80, 9, 40, 41)]
    cases = []
    for k, s in enumerate(seqs):
        u = rng.integers(-150, 151, len(s)).astype(np.int32) if k % 3 == 0 else None
        b = rng.integers(-200, 101, len(s)).astype(np.int32) if k % 2 == 0 else None
        cases.append((s, MC.draw_constraint(rng, s) if k % 4 != 3 else None, u, b))
    cases.append((seqs[1], None, None, None))
    whole = run(cases)
    assert whole[4].count(0) >= 5
    check_rows(cases, whole)
    assert run(cases, max_lds_len=40) == whole                                      # 33, 20, 9, 40 in LDS, the others in device memory
    assert run(cases, max_lds_len=1) == whole                                       # everything in device memory
    assert run(cases, max_lds_len=1, workspace_bytes=1) == whole                    # one sequence per chunk
    assert run(cases, max_lds_len=40, workspace_bytes=2 * 3 * 64 * 64 * 4) == whole
    order = [int(k) for k in rng.permutation(len(cases))]
    got = run([cases[k] for k in order], max_lds_len=40)
    assert [tuple(x[at] for x in got) for at in range(len(order))] == [tuple(x[k] for x in whole) for k in order]
    for k in (0, 3, len(cases) - 1):                                                # alone
        assert tuple(x[0] for x in run(cases[k:k + 1])) == tuple(x[k] for x in whole)


# ---- 4. where nothing constrains: rafft_mfe_batch

def neutral_sequences():
    rng = np.random.default_rng(77)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (60, 67, 75, 83, 90)]
    seqs.append("".join(rng.choice(list("GC"), 64)))
    for n_a in (30, 31):
        seqs.append("GGGCG" + "A" * n_a + "GCGCG" + "GAAA" + "CGCGC" + "CGCCC")
    return seqs + ["".join(np.random.default_rng(200).choice(list("ACGU"), 200))]


@pytest.mark.parametrize("which", ["builtin", "tie1"])
def test_gpu_constrained_mfe_is_mfe_batch_where_nothing_constrains(sets, which):
    install(sets, which)
    seqs = neutral_sequences()
    assert len(seqs[-1]) == 200 > N.lib().rafft_mfe_lds_len()
    free = zuker.mfe_batch_raw(seqs)
    assert not any(free[3])
    zero = lambda s: np.zeros(len(s), dtype=np.int32)
    forms = {"no arrays": [(s, None, None, None) for s in seqs],
             "all-'.' strings": [(s, "." * len(s), None, None) for s in seqs],
             "zero arrays": [(s, None, zero(s), zero(s)) for s in seqs],
             "all three": [(s, "." * len(s), zero(s), zero(s)) for s in seqs],
             "mixed": [(s, ("." * len(s), None)[k % 2], (zero(s), None, None)[k % 3], (None, zero(s))[k % 2]) for k, s in enumerate(seqs)]}
    for name, cases in forms.items():
        for kw in ({}, dict(max_lds_len=4)):
            rows, dcal, n_pairs, ps, status = run(cases, **kw)
            assert (rows, dcal, n_pairs, status) == free and ps == [0] * len(seqs), (which, name, kw)


# ---- 5. the limits

def test_gpu_constrained_mfe_at_its_limits():
    """4096 nt: two hairpins 4068 A apart with the pair (0, 4095) forced - positions up to 4095 in the pack and in the stack words;
    147 nt, the first length of the device-memory class, with u and b at +-RAFFT_MFE_SOFT_MAX; 4097 nt; a soft value of 20001"""
    h1, h2 = "GGGGGAAAACCCCC", "GCGCGGAAACGCGC"
    big = h1 + "A" * (N.MFE_MAX_LEN - 28) + h2
    rng = np.random.default_rng(147)
    s147 = "".join(rng.choice(list("ACGU"), 147))
    sign = lambda n: (rng.integers(0, 2, n) * 2 - 1).astype(np.int32) * N.MFE_SOFT_MAX
    cases = [(big, "(" + "." * (N.MFE_MAX_LEN - 2) + ")", None, None),
             (s147, None, sign(147), sign(147)),
             ("A" * (N.MFE_MAX_LEN + 1), None, None, None),
             (s147, MC.draw_constraint(rng, s147), np.full(147, N.MFE_SOFT_MAX, dtype=np.int32), np.full(147, -N.MFE_SOFT_MAX, dtype=np.int32))]
    assert [len(c[0]) for c in cases] == [4096, 147, 4097, 147] and len(s147) == N.lib().rafft_mfe_lds_len() + 1
    raw = run(cases)
    rows, dcal, n_pairs, ps, status = raw
    assert status[:3] == [0, 0, N.ERR_TOO_LONG] and status[3] in (0, N.ERR_INFEASIBLE)
    check_rows(cases, raw)
    # (the free minimum of `big` is that of the same two hairpins 40 A apart: tests/test_gpu_mfe.py, test_gpu_mfe_at_4096_nt)
    free = MF.Mirror(PR.tables_at(LP.builtin_par(), 37.0)).mfe(h1 + "A" * 40 + h2)
    assert rows[0][0] == "(" and MC.pair_table(rows[0])[0] == N.MFE_MAX_LEN - 1 and dcal[0] >= free and free < 0 and ps[0] == 0
    assert abs(dcal[1]) > 10 * N.MFE_SOFT_MAX and ps[1] != 0                         # the soft terms decide at this size
    assert dcal[1] <= MC.pseudo("." * 147, cases[1][2], cases[1][3])                 # never above the open chain
    soft = np.zeros(147, dtype=np.int32)
    soft[146] = N.MFE_SOFT_MAX + 1
    for where in ("soft_unpaired", "soft_stack"):
        with pytest.raises(N.RafftError) as e:
            zuker.mfe_constrained_batch_raw([s147, s147], **{where: [None, soft]})
        assert e.value.code == N.ERR_PARAM and "sequence 1" in str(e.value)


# ---- 6. other temperatures

@pytest.mark.parametrize("temp", [25.0, 60.0])
def test_gpu_constrained_mfe_at_another_temperature(sets, temp):
    install(sets, "synthetic")
    cases = [c for c in exhaustive_batch() if len(c[0]) >= 16][::7]
    assert len(cases) >= 12
    seqs = sorted({c[0] for c in cases})
    enum = {s: MF.enumerate_structures(s) for s in seqs}
    en, st = R.eval_structures([s for s in seqs for _ in enum[s]], [r for s in seqs for r in enum[s]], temp=temp)
    assert not any(st)
    energy, at = {}, 0
    for s in seqs:
        energy[s] = dict(zip(enum[s], en[at:at + len(enum[s])]))
        at += len(enum[s])
    want = [min((energy[s][r] + MC.pseudo(r, u, b) for r in enum[s] if MC.satisfies(r, con)), default=None) for s, con, u, b in cases]
    raw = run(cases, temp=temp)
    assert raw[4] == [0 if w is not None else N.ERR_INFEASIBLE for w in want] and raw[4].count(0) >= 5
    assert [d for d, w in zip(raw[1], want) if w is not None] == [w for w in want if w is not None]
    check_rows(cases, raw, temp)
    assert raw == run(cases, temp=temp, max_lds_len=4)
    at37 = run(cases)
    assert at37[4] == raw[4] and at37[1] != raw[1]
