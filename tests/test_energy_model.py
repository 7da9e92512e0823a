"""The constructed loops of tests/_loops.py on the CPU: the generators are deterministic and complete, every case reads the table
entry it is named after (the oracle's energy moves by the expected multiple when that entry is bumped), the oracle accepts and
rejects what tests/test_gpu_energy_model.py asserts of the device, and the hand-made parents of the expand seam hold the stems
they were built for.  Exact integers throughout."""
import numpy as np
import pytest

import oracle
from rafft_amd import params
import _loops as LP
import _par_reader as PR


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    path = tmp_path_factory.mktemp("par") / "index_sensitive.par"
    PR.write_par(idx, path, comment="index-sensitive")
    cases = LP.loop_cases(builtin)
    return dict(builtin=builtin, idx=idx, path=path, cases=cases, special=LP.special_lists(idx))


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def energies(cases):
    return [oracle.eval_structure(c[2], c[3]) for c in cases]


# ---- the generators

def test_generators_are_deterministic(sets):
    again = LP.loop_cases(LP.builtin_par())
    assert again == sets["cases"]
    assert list(LP.parent_cases()) == list(LP.parent_cases())
    a, b = LP.index_sensitive_par(sets["builtin"]), sets["idx"]
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert LP.bad_rows() == LP.bad_rows()


def test_no_two_cases_are_identical(sets):
    cases = sets["cases"]
    assert len({(c[2], c[3]) for c in cases}) == len(cases)
    assert len({c[0] for c in cases}) == len(cases)
    assert all(len(c[2]) == len(c[3]) for c in cases)
    assert sum(len(c[2]) < 60 for c in cases) > 0.97 * len(cases)


def test_index_sensitive_tables_are_distinct_up_to_the_imposed_symmetries(sets):
    old, par = sets["builtin"], sets["idx"]
    sym = {"stack": (1, 0), "int11": (1, 0, 3, 2), "int22": (1, 0, 4, 5, 2, 3)}
    part = {"hairpin": slice(3, None), "bulge": slice(1, None), "interior": slice(2, None)}
    for name in PR.SHAPES:
        a, o = np.asarray(par[name]), np.asarray(old[name])
        assert np.array_equal(a >= PR.INF, o >= PR.INF), name                       # INF entries stay
        assert np.array_equal(a[o >= PR.INF], o[o >= PR.INF]), name
        v = a[part.get(name, slice(None))]
        v = v[v < PR.INF]
        assert np.abs(v).max() < 8000, name                                        # int16 with room for sums
        if name in sym:
            assert np.array_equal(a, a.transpose(sym[name])), name
            idx = np.arange(a.size).reshape(a.shape)
            canon = idx <= idx.transpose(sym[name])
            assert len(set(a[canon].tolist())) == int(canon.sum()), name
        else:
            assert len(set(v.tolist())) == v.size, name
    for name in ("dangle5", "dangle3", "mismatch_multi", "mismatch_exterior"):      # (they survive the dangles = 2 clip to <= 0)
        assert np.asarray(par[name]).max() < 0, name
    sc = [par[k] for k in ("ml_base", "ml_closing", "ml_intern", "ninio", "max_ninio", "terminal_au")] + [int(par["lxc"])]
    assert len(set(sc)) == len(sc) and all(x % 2 == 1 for x in sc) and par["lxc"] == int(par["lxc"])
    for name in LP.KINDS:
        assert [s for s, _, _ in par[name]] == [s for s, _, _ in old[name]] + LP.OWN_SPECIAL[name]
    es = [e for name in LP.KINDS for _, e, _ in par[name]]
    assert len(set(es)) == len(es)


def test_product_reader_and_test_reader_agree_on_the_index_sensitive_file(sets, tmp_path):
    """two readers: the product loads the file the tests' writer made and writes it back; the tests' reader finds every value again"""
    params.load_params(sets["path"])
    back = tmp_path / "back.par"
    params.save_params(back)
    got, par = PR.read_par(back), sets["idx"]
    for name in PR.SHAPES:
        assert np.array_equal(got[name], par[name]), name
    for k in ("ml_base", "ml_closing", "ml_intern", "ninio", "max_ninio", "terminal_au", "lxc"):
        assert got[k] == par[k], k
    for name in LP.KINDS:
        assert [(s, e) for s, e, _ in got[name]] == [(s, e) for s, e, _ in par[name]]


def test_every_table_entry_is_the_target_of_a_case(sets):
    cases = sets["cases"]
    hit = {}
    for name, (table, idx), seq, db in cases:
        hit.setdefault(table, set()).add(idx)
    real = lambda table, idx: all(1 <= x <= 4 for x in idx[(2 if table.startswith("int") or table == "stack" else 1):])
    for table, size in LP.table_sizes().items():
        got = {i for i in hit[table] if table in ("hairpin", "bulge", "interior") or real(table, i)}
        assert len(got) == size, (table, len(got), size)
    for s in ("ml_intern", "term_au"):
        assert s in hit
    n_special = sum(len(v) for v in sets["special"].values())
    assert len(hit["special"]) == n_special == sum(len(sets["idx"][k]) for k in LP.KINDS)
    # both orientations of the 2 x 1 loop, for every entry
    n1 = {c[1][1] for c in cases if c[0].startswith("int21/n1/")}
    n2 = {c[1][1] for c in cases if c[0].startswith("int21/n2/")}
    assert len(n1) == len(n2) == 2304
    # an N base in every table with a base index
    with_n = {t for t, idxs in hit.items() for i in idxs if t not in ("stack", "hairpin", "bulge", "interior", "special") and 0 in i[-4:] and
              0 in i[(2 if t.startswith("int") else 1):]}
    assert with_n >= set(LP.MM_TABLES) | {"dangle5", "dangle3", "int11", "int21", "int22"}
    # the sizes and counts the issue names
    names = {c[0] for c in cases}
    for k in LP.ML_K:
        assert f"multi/{k}/adjacent" in names and f"multi/{k}/spaced" in names
    us = {n1 + n2 for n1 in LP.GENERIC_SIZES for n2 in LP.GENERIC_SIZES}
    assert {30, 31, 32} <= us and 29 in {1 + n for n in LP.ONE_N_SIZES}      # (no two of the generic sizes add up to 29: 1 x 28 does)
    nin, mx = sets["idx"]["ninio"], sets["idx"]["max_ninio"]
    ds = {abs(n1 - n2) * nin for n1 in LP.GENERIC_SIZES for n2 in LP.GENERIC_SIZES}
    assert any(0 < d < mx for d in ds) and any(d > mx for d in ds)


# ---- each case reads the entry it is named after

def table_values(T, special):
    """(table, index) -> value, from the tables in the oracle's layout"""
    def val(key):
        table, idx = key
        if table == "special":
            return T["special"][idx[0]][idx[1]][1]
        if table in LP.SCALARS:
            return T["scalars"][table]
        return int(T[table][idx])
    return val


def test_oracle_energy_is_the_sum_of_the_entries_a_case_reads(sets):
    """the loop decomposition of tests/_loops.py against the oracle, with tables in which no two entries are equal"""
    par = sets["idx"]
    T = PR.tables_at(par, 37.0)
    oracle.set_tables(T)
    val = table_values(T, sets["special"])
    cases = sets["cases"]
    for c, e in zip(cases, energies(cases)):
        r = LP.reads(c[2], c[3], sets["special"], par["ninio"], par["max_ninio"])
        assert c[1] == ("none", ()) or r[c[1]] >= 1, c[0]
        want = sum(n * val(k) for k, n in r.items() if k[0] != "lxc")
        want += sum(n * int(par["lxc"] * np.log(k[1][0] / 30.)) for k, n in r.items() if k[0] == "lxc")
        assert e == want, (c[0], e, want)


def test_bumping_the_targeted_entry_moves_the_oracle_energy_by_the_expected_multiple(sets):
    par = sets["idx"]
    T = PR.tables_at(par, 37.0)
    oracle.set_tables(T)
    cases = sets["cases"][::5]
    base = energies(cases)
    L = oracle.oracle.lib()
    import ctypes as C
    flat = {name: np.ascontiguousarray(T[name], dtype=np.int32).reshape(-1) for name in oracle.oracle.TABLE_NAMES}

    def put(name):
        assert L.oracle_set_table(name.encode(), flat[name].ctypes.data_as(C.POINTER(C.c_int)), flat[name].size) == 0

    for c, e0 in zip(cases, base):
        table, idx = c[1]
        mult = LP.reads(c[2], c[3], sets["special"], par["ninio"], par["max_ninio"])[c[1]]
        if table == "none":
            assert e0 == 0
            continue
        assert mult >= 1, c[0]
        if table in LP.SCALARS:
            sc = dict(T["scalars"]); sc[table] += 1
            L.oracle_set_scalars(sc["ml_base"], sc["ml_closing"], sc["ml_intern"], sc["ninio"], sc["max_ninio"], sc["term_au"], sc["lxc"])
        elif table == "special":
            sp = {k: list(v) for k, v in T["special"].items()}
            sp[idx[0]][idx[1]] = (sp[idx[0]][idx[1]][0], sp[idx[0]][idx[1]][1] + 1)
            oracle.set_tables(dict(T, special=sp))
        else:
            k = int(np.ravel_multi_index(idx, np.asarray(T[table]).shape))
            flat[table][k] += 1
            put(table)
        e1 = oracle.eval_structure(c[2], c[3])
        if table in LP.SCALARS or table == "special":
            oracle.set_tables(T)
        else:
            flat[table][k] -= 1
            put(table)
        assert e1 - e0 == mult, (c[0], e0, e1, mult)
    assert energies(cases) == base


# ---- the oracle accepts and rejects what the GPU test will assert

def test_oracle_evaluates_every_case_and_rejects_the_malformed_rows(sets):
    cases = sets["cases"]
    oracle.reset_tables()
    a = energies(cases)
    oracle.set_tables(PR.tables_at(sets["idx"], 37.0))
    b = energies(cases)
    assert a != b and len(a) == len(b) == len(cases)
    kinds = {"struct": 0, "char": 0, "pair": 0}
    for name, seq, db, kind in LP.bad_rows():
        with pytest.raises(ValueError):
            oracle.eval_structure(seq, db)
        kinds[kind] += 1
    assert kinds == {"struct": 4, "char": 2, "pair": 15}
    assert oracle.eval_structure("", "") == 0


# ---- the parents of the expand seam are not vacuous

def test_parent_cases_hold_the_stems_they_were_built_for():
    """every ranked lag of every parent, with min_nrj so high that each candidate stem gets its dE: the stems enclose 0, 1, 2, 16, 17,
    64, 65 and 128 and more branches of the parent, some have a branch inside a strand, and the regions and branch counts fall on
    both sides of every class limit"""
    enclosed, gapped, ns, ks = set(), 0, set(), set()
    for name, seq, db, pos in LP.parent_cases():
        if "/ext" not in name and "/GC" not in name and "/UA" not in name:
            continue                                     # (the closing pair does not change which stems a region holds)
        n = len(pos)
        br = LP.branches_of(db, pos)
        ns.add(n), ks.add(len(br))
        o = oracle.expand_node(seq, db, pos, min(2 * n - 1, 2047), 3, LP.HIGH_NRJ)
        stems = [r for r in range(len(o["lag"])) if o["nb"][r] > 0]
        assert sorted(o["kept"]) == stems, name            # every candidate got a dE and passed
        for r in stems:
            nb, mi, mj = o["nb"][r], o["mi"][r], o["mj"][r]
            enclosed.add(sum(1 for p, q in br if pos[mi] < p and q < pos[mj]))
            gapped += any(pos[mi - t + 1] - pos[mi - t] != 1 or pos[mj + t] - pos[mj + t - 1] != 1 for t in range(1, nb))
    assert {0, 1, 2, 16, 17, 64, 65, 128} <= enclosed and max(enclosed) >= 129, sorted(enclosed)
    assert gapped > 0
    for lim in (16, 32, 256, 1024):
        assert any(n <= lim for n in ns) and any(n > lim for n in ns), lim
    for lim in (16, 32, 128):
        assert lim in ks and lim + 1 in ks and any(k < lim for k in ks), lim
    assert 0 in ks and 1 in ks
