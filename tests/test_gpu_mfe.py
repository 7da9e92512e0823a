"""rafft_mfe_batch on a real MI355X (`-m gpu`): the minimum over every structure of short sequences (evaluated by eval_kernel in one
call), the tests' own mirror of the recurrences where enumeration cannot reach, the published ViennaRNA MFE rows as an upper bound,
same input - same bits across batch position, order, chunking and size class, errors that stay with their sequence, the rows of the
mirror's traceback in the documented candidate order on tables that tie, other temperatures under a parameter file with enthalpies,
and the length limit of 4096 nt.  Integers and bytes: no tolerance."""
import gzip
import os
import time

import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, params, rafft as R, zuker
from conftest import GOLD
import _loops as LP
import _mfe_np as MF
import _par_reader as PR

pytestmark = pytest.mark.gpu

TABLES = ("builtin", "multiloops_win")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    idx.update(ml_closing=-700, ml_intern=-300)               # negative enough that multiloops win at 16-20 nt
    out = dict(builtin=builtin, multiloops_win=idx, tie0=LP.tie_par(builtin, LP.TIE_ML[0]), tie1=LP.tie_par(builtin, LP.TIE_ML[1]),
               synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name, comment in (("multiloops_win", "index-sensitive, multiloops win"), ("tie0", "flat, multiloops cost nothing"),
                          ("tie1", "flat, multiloops win"), ("synthetic", "made-up enthalpies")):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=comment)
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


def multiloops(db):
    """number of pairs of `db` that close a loop with two or more branches"""
    pt, n = LP.pair_table(db), 0
    for i, j in enumerate(pt):
        if j > i:
            k, br = i + 1, 0
            while k < j:
                if pt[k] > k:
                    br += 1
                    k = pt[k] + 1
                else:
                    k += 1
            n += br >= 2
    return n


def check_rows(seqs, raw, temp=37.0):
    """what holds for every result: the row's own energy is the reported one, the pair count is the row's, pairs are canonical"""
    rows, dcal, n_pairs, status = raw
    assert not any(status)
    got, st = R.eval_structures(seqs, rows, temp=temp)
    assert not any(st) and got == dcal
    assert n_pairs == [r.count("(") for r in rows]
    for s, r in zip(seqs, rows):
        assert len(r) == len(s)
        pt = LP.pair_table(r)
        assert all(j < 0 or (s[min(i, j)] + s[max(i, j)]) in MF.PAIRS for i, j in enumerate(pt))


# ---- 1. the exhaustive minimum

def exhaustive_sequences():
    rng = np.random.default_rng(20)
    seqs = ["A", "GC", "GAC", "GAAC"]                                              # lengths 1-4: no pair possible
    seqs += ["".join(rng.choice(list("ACGU"), n)) for n in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20, 20, 20)]
    seqs += ["".join(rng.choice(list("GCU"), n)) for n in (14, 16, 17)]
    for name in LP.KINDS:                                                          # GC hairpins around the special loops
        for sp in LP.OWN_SPECIAL[name]:
            seqs.append("GG" + sp + "CC")
    seqs += ["GGGACACCCAGGACCACCC", "G" * 10 + "U" * 10, "GU" * 9, "GGGUUUGGGUUUCCC", "GCGCAAAGCGCAAAGCGC", "GGGAAACCCAGGGAAACCCA"]
    return seqs + LP.N_SEQS                                                        # N pairs with nothing and reads row 0 of the mismatch tables


_ENUM = {}


def enumerated(seqs):
    for s in seqs:
        if s not in _ENUM:
            _ENUM[s] = MF.enumerate_structures(s)
    return [_ENUM[s] for s in seqs]


def exhaustive_minimum(seqs, temp=37.0):
    """the minimum of eval_kernel over every structure of each sequence, under the installed tables (one call)"""
    rows = enumerated(seqs)
    flat_s = [s for s, rr in zip(seqs, rows) for _ in rr]
    flat_r = [r for rr in rows for r in rr]
    en, st = R.eval_structures(flat_s, flat_r, temp=temp)
    assert not any(st)
    want, at = [], 0
    for rr in rows:
        want.append(min(en[at:at + len(rr)]))
        at += len(rr)
    return want


@pytest.mark.parametrize("which", TABLES)
def test_gpu_mfe_is_the_minimum_over_every_structure_in_both_classes(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    assert 40 <= len(seqs) <= 49 and max(map(len, seqs)) == 20 and sum("N" in s for s in seqs) == 4
    want = exhaustive_minimum(seqs)
    lds = zuker.mfe_batch_raw(seqs)
    hbm = zuker.mfe_batch_raw(seqs, max_lds_len=4)
    assert lds == hbm                                                              # rows, energies, pair counts: byte-identical
    assert lds[1] == want
    check_rows(seqs, lds)
    assert lds[0][:4] == [".", "..", "...", "...."] and lds[1][:4] == [0] * 4
    if which == "multiloops_win":
        assert sum(multiloops(r) > 0 for s, r in zip(seqs, lds[0]) if 16 <= len(s) <= 20) >= 3
    else:
        assert any("(" in r for r in lds[0])


# ---- 2. against the mirror where enumeration cannot reach

def mirror_sequences():
    rng = np.random.default_rng(77)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (60, 67, 75, 83, 90)]
    seqs.append("".join(rng.choice(list("GC"), 64)))
    # one good helix pair separated by an A-run on one side: 30 is an allowed bulge, 31 is not
    for run in (30, 31):
        seqs.append("GGGCG" + "A" * run + "GCGCG" + "GAAA" + "CGCGC" + "CGCCC")
    return seqs


_MIRROR = {}


@pytest.mark.parametrize("which", TABLES)
def test_gpu_mfe_equals_the_mirror_at_60_to_90_nt(sets, which):
    install(sets, which)
    seqs = mirror_sequences()
    if which not in _MIRROR:
        m = MF.Mirror(PR.tables_at(sets[which], 37.0))
        _MIRROR[which] = [m.mfe(s) for s in seqs]
    want = _MIRROR[which]
    lds = zuker.mfe_batch_raw(seqs)
    hbm = zuker.mfe_batch_raw(seqs, max_lds_len=4)
    assert lds[1] == want and hbm[1] == want
    assert lds == hbm
    check_rows(seqs, lds)
    if which == "builtin":
        # the run of 30 is bridged by one bulge; at 31 the cap binds: the outer helix is given up although closing it over the
        # bulge of 31 would evaluate lower
        r30, r31 = lds[0][-2], lds[0][-1]
        assert r30.startswith("(((((" + "." * 30 + "(((((") and not r31.startswith("(((((")
        bridged = "(((((" + "." * 31 + "(((((....))))))))))"
        en, st = R.eval_structures([seqs[-1]], [bridged])
        assert st == [0] and en[0] < lds[1][-1]


# ---- 3. the published rows

@pytest.fixture(scope="module")
def published():
    with gzip.open(os.path.join(GOLD, "mfe_published.tsv.gz"), "rt") as fh:
        rows = [line.split() for line in fh]
    assert len(rows) == 1733
    return [r[0] for r in rows], [r[1] for r in rows], [int(r[2]) for r in rows]


def test_gpu_mfe_never_above_the_published_rows(published):
    seqs, pub_db, pub_dcal = published
    raw = zuker.mfe_batch_raw(seqs)                                                # one call
    check_rows(seqs, raw)
    dcal = raw[1]
    higher = [(k, dcal[k], pub_dcal[k]) for k in range(len(seqs)) if dcal[k] > pub_dcal[k]]
    equal = sum(a == b for a, b in zip(dcal, pub_dcal))
    print(f"\nMFE against the published rows: {equal} equal, {len(seqs) - equal - len(higher)} lower, {len(higher)} higher of {len(seqs)}")
    assert not higher, higher[:10]
    sub = list(range(0, len(seqs), len(seqs) // 50))[:50]
    beams = rafft_amd.fold_batch([seqs[k] for k in sub], 100, 50)
    for k, beam in zip(sub, beams):
        assert dcal[k] <= min(int(x) for x in beam.dcal()), seqs[k]


# ---- 4. same input, same bits

def test_gpu_mfe_same_input_same_bits():
    rng = np.random.default_rng(5)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (33, 58, 71, 20, 64, 45, 80, 9)]
    for lds_len in (0, 4):
        whole = zuker.mfe_batch_raw(seqs, max_lds_len=lds_len)
        row = {s: (whole[0][k], whole[1][k], whole[2][k]) for k, s in enumerate(seqs)}
        for k in (0, 3, len(seqs) - 1):                                            # alone
            one = zuker.mfe_batch_raw([seqs[k]], max_lds_len=lds_len)
            assert (one[0][0], one[1][0], one[2][0]) == row[seqs[k]]
        for order in (seqs[::-1], [seqs[k] for k in rng.permutation(len(seqs))], seqs[1:] + seqs[:1]):
            got = zuker.mfe_batch_raw(order, max_lds_len=lds_len)
            assert [(got[0][k], got[1][k], got[2][k]) for k in range(len(order))] == [row[s] for s in order]
    # several chunks of the device-memory class: room for the tables of two 64-nt sequences, then for those of one 9-nt sequence
    for budget in (2 * 3 * 64 * 64 * 4, 3 * 9 * 9 * 4):
        assert zuker.mfe_batch_raw(seqs, max_lds_len=4, workspace_bytes=budget) == zuker.mfe_batch_raw(seqs, max_lds_len=4)
    assert zuker.mfe_batch_raw(seqs) == zuker.mfe_batch_raw(seqs, max_lds_len=4)


def test_gpu_mfe_at_the_lds_bound():
    lc = N.lib().rafft_mfe_lds_len()
    rng = np.random.default_rng(146)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (lc, lc + 1, lc, lc - 1)]
    routed = zuker.mfe_batch_raw(seqs)                                             # lc in LDS, lc + 1 in device memory
    forced = zuker.mfe_batch_raw(seqs, max_lds_len=lc - 1)                         # lc in device memory as well
    assert routed == forced
    check_rows(seqs, routed)
    assert all(d < 0 for d in routed[1])


# ---- 5. errors stay with their sequence

def test_gpu_mfe_errors_stay_with_their_sequence():
    good = ["GGGGAAAACCCC", "GGGAAACCCAGGGAAACCC", "GCGCUUCGGCGC", "ACGUACGUACGUACGUAGC"]
    alone = zuker.mfe_batch_raw(good)
    seqs = [good[0], "", good[1], "GGGXAAACCC", good[2], "A" * (N.MFE_MAX_LEN + 1), good[3]]
    rows, dcal, n_pairs, status = zuker.mfe_batch_raw(seqs)                        # returns: the call is RAFFT_OK
    assert status == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, 0, N.ERR_TOO_LONG, 0]
    assert N.lib().rafft_last_error().decode().startswith("sequence 1")
    assert [rows[k] for k in (1, 3, 5)] == ["", "." * 10, "." * (N.MFE_MAX_LEN + 1)]
    assert [dcal[k] for k in (1, 3, 5)] == [0, 0, 0] and [n_pairs[k] for k in (1, 3, 5)] == [0, 0, 0]
    keep = (0, 2, 4, 6)
    assert ([rows[k] for k in keep], [dcal[k] for k in keep], [n_pairs[k] for k in keep], [0] * 4) == alone
    assert zuker.mfe_batch_raw(seqs, max_lds_len=4)[:3] == (rows, dcal, n_pairs)
    got = rafft_amd.mfe_batch(seqs, raise_errors=False)
    assert [g is None for g in got] == [False, True, False, True, False, True, False]
    assert got[0].str_struct == rows[0] and got[0].dcal == dcal[0] and got[0].energy == rafft_amd.Structure("", dcal[0]).energy
    assert rafft_amd.mfe(good[0]).str_struct == rows[0]
    with pytest.raises(KeyError):
        rafft_amd.mfe_batch(seqs[2:4])
    for batch in (good, ["", "GGGXAACCC"]):                                        # the built-in tables are 37 C only, as for the fold
        with pytest.raises(N.RafftError) as e:
            zuker.mfe_batch_raw(batch, temp=25.0)
        assert e.value.code == N.ERR_TEMP


# ---- 6. the device-memory class at a length its own tests above do not reach

def test_gpu_mfe_hbm_class_at_1000_nt():
    """many workgroups per diagonal, a thousand launches, stack words with positions far above the LDS bound: the row's own energy
    is the reported one and every pair is canonical at 1000 nt; at 200 nt, where the mirror still takes seconds, the energy is the
    mirror's; neither depends on order or chunking"""
    rng = np.random.default_rng(1000)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (1000, 200, 333)]
    raw = zuker.mfe_batch_raw(seqs)
    check_rows(seqs, raw)
    assert all(d < 0 for d in raw[1]) and raw[2][0] > 100
    assert raw[1][1] == MF.Mirror(PR.tables_at(LP.builtin_par(), 37.0)).mfe(seqs[1])
    rev = zuker.mfe_batch_raw(seqs[::-1], workspace_bytes=1)                       # one chunk per sequence, the other order
    assert tuple(x[::-1] for x in rev) == raw


# ---- 7. the traceback's candidate order

_FOLD = {}


def mirror_folds(sets, which, seqs, temp=37.0):
    """Mirror.fold(s, "first") of every sequence under a table set: (dcal, row), computed once"""
    key = (which, temp)
    if key not in _FOLD:
        _FOLD[key] = (MF.Mirror(PR.tables_at(sets[which], temp)), {})
    mirror, done = _FOLD[key]
    for s in seqs:
        if s not in done:
            done[s] = mirror.fold(s, "first")
    return [done[s] for s in seqs]


def assert_rows_are_the_mirrors(sets, which, seqs, temp=37.0):
    want = mirror_folds(sets, which, seqs, temp)
    routed = zuker.mfe_batch_raw(seqs, temp=temp)
    forced = zuker.mfe_batch_raw(seqs, temp=temp, max_lds_len=4)
    assert routed == forced
    wrong = [(s, r, w[1]) for s, r, w in zip(seqs, routed[0], want) if r != w[1]]
    assert not wrong, (which, len(wrong), wrong[:3])
    assert routed[1] == [w[0] for w in want] and routed[2] == [w[1].count("(") for w in want]
    check_rows(seqs, routed, temp)
    return routed


@pytest.mark.parametrize("which", ["tie0", "tie1"])
def test_gpu_mfe_rows_follow_the_documented_order_where_the_tables_tie(sets, which):
    """flat tables: most of these sequences have several structures of minimum energy (tests/test_mfe_host.py counts them and shows
    that the reversed candidate order returns other rows), so the row is the documented order's or the test fails; the long list
    reaches the second and later rounds of the four ballots"""
    install(sets, which)
    assert_rows_are_the_mirrors(sets, which, LP.tie_short_sequences() + LP.tie_long_sequences())
    assert exhaustive_minimum(LP.tie_short_sequences()) == [w[0] for w in mirror_folds(sets, which, LP.tie_short_sequences())]


@pytest.mark.parametrize("which", TABLES)
def test_gpu_mfe_rows_are_the_mirrors_at_60_to_90_nt(sets, which):
    install(sets, which)
    assert_rows_are_the_mirrors(sets, which, mirror_sequences())


# ---- 8. other temperatures

@pytest.mark.parametrize("temp", [25.0, 60.0])
def test_gpu_mfe_at_another_temperature(sets, temp):
    """a parameter file with (made-up) enthalpies: at 25 and 60 C the energy is the minimum of eval_kernel at that temperature over
    every structure, the mirror's over tables rescaled by the tests' own reader at 60-90 nt, rows included; both classes agree; the
    results are not those of 37 C, and 37 C comes back afterwards"""
    install(sets, "synthetic")
    short, longer = exhaustive_sequences(), mirror_sequences()
    at37 = zuker.mfe_batch_raw(short + longer)
    lds = zuker.mfe_batch_raw(short, temp=temp)
    assert lds == zuker.mfe_batch_raw(short, temp=temp, max_lds_len=4)
    assert lds[1] == exhaustive_minimum(short, temp)
    check_rows(short, lds, temp)
    got = assert_rows_are_the_mirrors(sets, "synthetic", longer, temp)
    n_other = sum(a != b for a, b in zip(lds[1] + got[1], at37[1]))
    print(f"\n{temp} C: {n_other} of {len(at37[1])} energies differ from those at 37 C")
    assert n_other >= 1
    assert zuker.mfe_batch_raw(short + longer) == at37
    assert at37[1][len(short):] == [w[0] for w in mirror_folds(sets, "synthetic", longer)]


# ---- 9. the length limit

def test_gpu_mfe_at_4096_nt(sets):
    """positions up to 4095 through the 12-bit fields of the stack words.  Sequence 0: two hairpins 4068 A apart (no U: the spacer
    pairs with nothing; an interior loop spans at most 30; ml_base is 0, so a multiloop across the spacer costs the same at any
    length; a hairpin across it only gets dearer with lxc > 0) - its energy and row are the mirror's at a spacer of 40, stretched.
    Sequence 1: 2100 nt of tiled hairpins, bit 11 of the stack words.  Sequence 2 is one too long, sequence 3 is short."""
    h1, h2 = "GGGGGAAAACCCCC", "GCGCGGAAACGCGC"
    tile, tile_row = "GGGGGAAAACCCCCAA", "(((((....))))).."
    seqs = [h1 + "A" * (N.MFE_MAX_LEN - 28) + h2, tile * 131 + "GGGG", "A" * (N.MFE_MAX_LEN + 1), "GGGAAACCC"]
    assert [len(s) for s in seqs] == [4096, 2100, 4097, 9]
    assert sets["builtin"]["ml_base"] >= 0 and sets["builtin"]["lxc"] >= 0
    small = h1 + "A" * 40 + h2
    mirror = MF.Mirror(PR.tables_at(sets["builtin"], 37.0))
    d40, row40 = mirror.fold(small, "first")
    assert mirror.fold(small, "last") == (d40, row40)
    pt = LP.pair_table(row40)
    across = [(i, j) for i, j in enumerate(pt) if i < len(h1) and j >= len(h1) + 40]
    assert not any("(" not in row40[i + 1:j] for i, j in across)                 # no hairpin closed across the spacer
    t0 = time.perf_counter()
    rows, dcal, n_pairs, status = zuker.mfe_batch_raw(seqs)
    wall = time.perf_counter() - t0
    print(f"\n4096 + 2100 nt in one call: {wall:.2f} s; MFE {dcal[0]} and {dcal[1]} dcal/mol, {n_pairs[0]} and {n_pairs[1]} pairs")
    assert status == [0, 0, N.ERR_TOO_LONG, 0]
    assert dcal[0] == d40 and rows[0] == row40[:len(h1)] + "." * (N.MFE_MAX_LEN - 28) + row40[len(h1) + 40:]
    assert rows[0][N.MFE_MAX_LEN - 1] == ")" and LP.pair_table(rows[0])[N.MFE_MAX_LEN - 1] == N.MFE_MAX_LEN - len(h2)
    keep = (0, 1, 3)
    check_rows([seqs[k] for k in keep], ([rows[k] for k in keep], [dcal[k] for k in keep], [n_pairs[k] for k in keep], [0] * 3))
    tiled, st = R.eval_structures([seqs[1]], [tile_row * 131 + "...."])
    assert st == [0] and dcal[1] <= tiled[0] < 0
    assert max(LP.pair_table(rows[1])) >= 2048                                     # pairs beyond bit 11
    assert (rows[2], dcal[2], n_pairs[2]) == ("." * (N.MFE_MAX_LEN + 1), 0, 0)
    alone = zuker.mfe_batch_raw(seqs[3:])
    assert (rows[3], dcal[3], n_pairs[3]) == (alone[0][0], alone[1][0], alone[2][0])


# ---- 10. the command line with the real scorer

def test_gpu_cli_mfe_scores_table(tmp_path):
    from rafft_amd import cli, scoring
    rows = [("GGGGAAAACCCC", "((((....))))", "hp"), ("GGGAAACCCAGGGAAACCC", "(((...))).(((...)))", "two"), ("ACGUACGUAC", "..........", "none"),
            ("GCGCUUCGGCGCAAAAGGGAAACCC", "((((....))))....(.(...).)", "mixed")]
    csvf = tmp_path / "known.csv"
    csvf.write_text("".join(f"{s},{k},{n}\n" for s, k, n in rows))
    out, lines = tmp_path / "scores.csv", tmp_path / "lines.txt"
    cli.main(["-sf", str(csvf), "--batch", "--mfe", "--scores", str(out), "-o", str(lines)])
    got = out.read_text().splitlines()
    assert got[0] == "seq,len_seq,struct,nrj,nbp,pvv,sens,name" and len(got) == 1 + len(rows)
    want = rafft_amd.mfe_batch([r[0] for r in rows])
    for line, (s, known, name), st in zip(got[1:], rows, want):
        ppv, sens = scoring.score(st.str_struct, known)
        assert line == f"{s},{len(s)},{st.str_struct},{st.energy},{st.str_struct.count('(')},{round(ppv, 2)},{round(sens, 2)},{name}"
    assert lines.read_text().splitlines() == [cli.format_mfe_line(r[0], st) for r, st in zip(rows, want)]
    assert any("(" in st.str_struct for st in want)
