"""The energy model entry by entry on a real MI355X (`-m gpu`): every constructed loop of tests/_loops.py through eval_kernel, the
evaluator's statuses, hand-made parents through the expand seam under every routing, and whole folds - with the built-in tables and
with index-sensitive ones (pairwise distinct entries: a transposed index cannot hide).  The reference is the oracle fed by the
tests' own parameter reader; the product reads the same file with its own.  Integers and bit-equal fp64: no tolerance."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rafft_amd
from rafft_amd import _native as N, params, rafft as R
import _loops as LP
import _par_reader as PR

pytestmark = pytest.mark.gpu

KEYS = ("lag", "cor", "nb", "mi", "mj", "score", "ddcal", "kept")
TABLES = ("builtin", "index_sensitive")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    d = tmp_path_factory.mktemp("par")
    PR.write_par(idx, d / "index_sensitive.par", comment="index-sensitive")
    return dict(builtin=builtin, idx=idx, dir=d, path=d / "index_sensitive.par", cases=LP.loop_cases(builtin))


def install(sets, which):
    if which == "builtin":
        params.reset_params()
        oracle.reset_tables()
    else:
        params.load_params(sets["path"])
        oracle.set_tables(PR.tables_at(sets["idx"], 37.0))


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()
    oracle.reset_tables()


_ORACLE_CASES, _ORACLE_NODES = {}, {}


def oracle_cases(sets, which):
    """(the caller has installed `which`) the oracle's energy of every loop case, computed once per table set"""
    if which not in _ORACLE_CASES:
        _ORACLE_CASES[which] = [oracle.eval_structure(c[2], c[3]) for c in sets["cases"]]
    return _ORACLE_CASES[which]


# ---- 1. eval_kernel against the oracle

@pytest.mark.parametrize("which", TABLES)
def test_gpu_eval_kernel_on_every_constructed_loop_vs_oracle(sets, which):
    install(sets, which)
    cases = sets["cases"]
    want = oracle_cases(sets, which)
    got, status = R.eval_structures([c[2] for c in cases], [c[3] for c in cases])
    assert not any(status)
    wrong = [(c[0], g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:10])
    got2, status2, guessed = R.eval_structures_info([c[2] for c in cases], [c[3] for c in cases])
    assert not any(status2) and got2 == want
    if which == "index_sensitive":
        assert not any(guessed)                          # a loaded file: every entry is the file's
    else:
        assert 0 < sum(guessed) < len(guessed)


# ---- 2. teeth: one entry of the device's tables differs from the oracle's

@pytest.mark.parametrize("table,idx,must_hit", [
    ("int21", (3, 6, 1, 2, 4), ("int21/n1/3/6/ACU", "int21/n2/3/6/ACU")),                 # the second is read through the n2 == 1 swap
    ("mismatch_interior_23", (4, 2, 3), ("2x3/outer/2x3/4/CG", "2x3/outer/3x2/4/CG", "2x3/inner/2x3/4/CG", "2x3/inner/3x2/4/CG")),
    ("mismatch_multi", (5, 3, 1), ("multi/closing_mm/5/GA", "multi/branch_mm/5/GA"))])
def test_gpu_one_changed_entry_shows_in_exactly_the_cases_that_read_it(sets, table, idx, must_hit):
    cases = sets["cases"]
    install(sets, "index_sensitive")
    want = oracle_cases(sets, "index_sensitive")
    par2 = dict(sets["idx"])
    a = np.asarray(par2[table]).copy()
    a[(idx[0] - 1,) + ((idx[1] - 1,) + idx[2:] if table == "int21" else idx[1:])] += 1      # (the file counts pair types from 0)
    par2[table] = a
    path2 = sets["dir"] / f"bumped_{table}.par"
    PR.write_par(par2, path2, comment="one entry bumped")
    # which cases read the entry: those whose oracle energy moves with it (the CPU bump check of tests/test_energy_model.py)
    oracle.set_tables(PR.tables_at(par2, 37.0))
    moved = {c[0] for c, w in zip(cases, want) if oracle.eval_structure(c[2], c[3]) != w}
    named = {c[0] for c in cases if c[1] == (table, idx)}
    assert named and named <= moved and set(must_hit) <= named, (named - moved, set(must_hit) - named)
    params.load_params(path2)
    got, status = R.eval_structures([c[2] for c in cases], [c[3] for c in cases])
    assert not any(status)
    differs = {c[0] for c, g, w in zip(cases, got, want) if g != w}
    assert differs == moved, (sorted(differs - moved)[:5], sorted(moved - differs)[:5])
    assert all(g >= w for g, w in zip(got, want))                 # (the device's entry is the larger one)


# ---- 3. statuses

def test_gpu_evaluator_statuses_in_a_mixed_batch(sets):
    install(sets, "builtin")
    cases = sets["cases"]
    want_all = oracle_cases(sets, "builtin")
    _, _, guessed_all = R.eval_structures_info([c[2] for c in cases], [c[3] for c in cases])
    k_guess = next(k for k, c in enumerate(cases) if c[0].startswith("int11/") and guessed_all[k])
    bad = LP.bad_rows()
    # a bad pair beside a loop that reads a rule / model value of the built-in tables: an error row is not "guessed"
    bad.append(("pair/beside_a_guessed_loop", cases[k_guess][2] + "AAGAAAAA", cases[k_guess][3] + ".(....).", "pair"))
    code = {"struct": N.ERR_STRUCT, "char": N.ERR_BAD_CHAR, "pair": N.ERR_STRUCT}
    seqs, dbs, want_st, want_e = [], [], [], []
    step = len(cases) // len(bad)
    for k, (name, s, d, kind) in enumerate(bad):
        good = k_guess if k == 0 else k * step
        seqs += [cases[good][2], s]; dbs += [cases[good][3], d]
        want_st += [0, code[kind]]; want_e += [want_all[good], None]
    seqs += ["", cases[7][2]]; dbs += ["", cases[7][3]]; want_st += [0, 0]; want_e += [0, want_all[7]]
    assert N.ERR_STRUCT == 8 and N.ERR_BAD_CHAR == 1
    for fn in ("plain", "info"):
        if fn == "plain":
            got, status = R.eval_structures(seqs, dbs)
            guessed = None
        else:
            got, status, guessed = R.eval_structures_info(seqs, dbs)
        assert status == want_st
        assert [g for g, w in zip(got, want_e) if w is not None] == [w for w in want_e if w is not None]
        if guessed is not None:
            assert guessed[0] == 1                                           # (the flag does work in this batch)
            assert [g for g, st in zip(guessed, want_st) if st] == [0] * sum(1 for st in want_st if st)
    # without a status array the call itself fails with the first bad status
    L = N.lib()
    out = C.c_int()
    for name, s, d, kind in bad:
        assert L.rafft_eval_structure(s.encode(), d.encode(), C.byref(out)) == code[kind], name
    assert L.rafft_eval_structure(cases[7][2].encode(), cases[7][3].encode(), C.byref(out)) == 0 and out.value == want_all[7]
    assert L.rafft_eval_structure(b"", b"", C.byref(out)) == 0 and out.value == 0
    rows = [(cases[7][2], cases[7][3]), ("GGGTAACCC", "(((...)))"), ("GGGAAACCC", "(((....))")]
    a = (C.c_char_p * 3)(*[r[0].encode() for r in rows])
    b = (C.c_char_p * 3)(*[r[1].encode() for r in rows])
    o3 = (C.c_int * 3)()
    assert L.rafft_eval_structures(3, a, b, o3, None) == N.ERR_BAD_CHAR


def test_gpu_evaluator_length_limit():
    """32 768 nt is the longest structure the 16-bit pair tables hold: accepted and equal to the oracle; 32 769 nt is refused"""
    seq = "G" + "GGGAAACCCA" * 3276 + "AAAAAA" + "C"              # a multiloop of 3276 branches closed by the first and the last position
    db = "(" + "(((...)))." * 3276 + "......" + ")"
    assert len(seq) == len(db) == 32768
    want = oracle.eval_structure(seq, db)
    got, status = R.eval_structures([seq, seq + "A"], [db, db + "."])
    assert status == [0, N.ERR_STRUCT] and got[0] == want


# ---- 4. the expand seam on constructed parents

@pytest.fixture(params=["classes_by_size", "classes_merged", "general_builds"])
def expand_class_routing(request, monkeypatch):
    """the three routings of tests/test_gpu_ties.py"""
    if request.param in ("classes_by_size", "general_builds"):
        monkeypatch.setenv("RAFFT_MERGE_BELOW", "0")
        monkeypatch.setenv("RAFFT_MERGE2_BELOW", "0")
    if request.param == "general_builds":
        monkeypatch.setenv("RAFFT_PROD", "0")
    yield request.param


def seam_settings(n):
    """(nb_mode, min_hp, min_nrj): each value of each setting with each value of the next (nb_mode 2n - 1 as far as the LDS plans
    rank lags: 2047)"""
    full = max(1, min(2 * n - 1, 2047))
    return ((100, 3, 0.0), (full, 0, 0.0), (100, 0, LP.HIGH_NRJ), (full, 3, LP.HIGH_NRJ))


@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("k", LP.PARENT_K)
def test_gpu_expand_node_on_constructed_parents_vs_oracle(sets, monkeypatch, expand_class_routing, k, which):
    install(sets, which)
    for name, seq, db, pos in LP.parent_cases((k,)):
        for setting in seam_settings(len(pos)):
            key = (which, name, setting)
            if key not in _ORACLE_NODES:
                _ORACLE_NODES[key] = oracle.expand_node(seq, db, pos, *setting)
            o = _ORACLE_NODES[key]
            for small in ("16,32", "16,16", "0,0"):
                monkeypatch.setenv("RAFFT_SMALL", small)
                g = R.expand_node(seq, db, pos, *setting)
                for kk in KEYS:
                    assert g[kk] == o[kk], (name, setting, small, kk)


# ---- 5. whole folds with the index-sensitive tables

def test_gpu_folds_with_index_sensitive_tables_vs_oracle(sets):
    rng = np.random.default_rng(1617)
    comp = {"A": "U", "U": "A", "G": "C", "C": "G"}
    seqs = []
    for nb in (17, 33):
        left = "".join(rng.choice(list("GCAU"), nb))
        right = "".join(comp[c] for c in reversed(left))
        wob = "".join(("U" if (c == "C" and rng.random() < 0.3) else c) for c in right)
        seqs.append("AC" + left + "GCAA" + wob + "UUA" if nb == 17 else
                    left + "GAAA" + right + "AAAA" + left[::-1] + "UUUU" + "".join(comp[c] for c in left))
    seqs += [("CUG" * 40)[:100], ("GGGAAACCC" * 12)[:100]]
    seqs += ["".join(rng.choice(list("ACGU"), n)) for n in (150, 420)]
    install(sets, "index_sensitive")
    got = rafft_amd.fold_batch(seqs, 100, 6, 1000, traj=True)
    for s, (fin, traj) in zip(seqs, got):
        _, o = oracle.fold(s, 100, 6, 1000, traj=True)
        assert [[(x.str_struct, x.dcal) for x in st] for st in traj] == [[(x.str_struct, x.dcal) for x in st] for st in o], len(s)
        assert len(traj) > 1
