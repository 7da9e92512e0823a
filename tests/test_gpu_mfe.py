"""rafft_mfe_batch on a real MI355X (`-m gpu`): the minimum over every structure of short sequences (evaluated by eval_kernel in one
call), the tests' own mirror of the recurrences where enumeration cannot reach, the published ViennaRNA MFE rows as an upper bound,
same input - same bits across batch position, order, chunking and size class, and errors that stay with their sequence.
Integers and bytes: no tolerance."""
import gzip
import os

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
    path = tmp_path_factory.mktemp("par") / "multiloops_win.par"
    PR.write_par(idx, path, comment="index-sensitive, multiloops win")
    return dict(builtin=builtin, multiloops_win=idx, path=path)


def install(sets, which):
    if which == "builtin":
        params.reset_params()
    else:
        params.load_params(sets["path"])


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


def check_rows(seqs, raw):
    """what holds for every result: the row's own energy is the reported one, the pair count is the row's, pairs are canonical"""
    rows, dcal, n_pairs, status = raw
    assert not any(status)
    got, st = R.eval_structures(seqs, rows)
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
    return seqs


_ENUM = {}


def enumerated(seqs):
    for s in seqs:
        if s not in _ENUM:
            _ENUM[s] = MF.enumerate_structures(s)
    return [_ENUM[s] for s in seqs]


@pytest.mark.parametrize("which", TABLES)
def test_gpu_mfe_is_the_minimum_over_every_structure_in_both_classes(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    assert 36 <= len(seqs) <= 45 and max(map(len, seqs)) == 20
    rows = enumerated(seqs)
    flat_s = [s for s, rr in zip(seqs, rows) for _ in rr]
    flat_r = [r for rr in rows for r in rr]
    en, st = R.eval_structures(flat_s, flat_r)                                     # one call
    assert not any(st)
    want, at = [], 0
    for rr in rows:
        want.append(min(en[at:at + len(rr)]))
        at += len(rr)
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


# ---- 7. the command line with the real scorer

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
