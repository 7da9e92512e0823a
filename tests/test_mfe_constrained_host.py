"""The host side of the constrained MFE folds (rafft_mfe_constrained_batch, rafft_amd.mfe_constrained_batch, `rafft --mfe -C`,
`rafft --mfe --shape FILE`) and the tests' mirror of them: the mirror equals the minimum of the oracle's
energy plus the soft terms over every structure that satisfies the constraint and says "infeasible" exactly when there is none,
with hard constraints, with soft terms and with both; under tables that tie both candidate orders return rows of the constrained
co-optimal set; the SHAPE conversion, the record, the constraint packs (tests/hostcheck/mfe_con_check.cpp, plain and under
sanitizers), every error the host detects and the option surface.  Integers and bytes: no tolerance.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from rafft_amd import _native, cli, params, zuker
import rafft_amd
from conftest import ROOT
import _loops as LP
import _mfe_np as MF
import _mfe_con_np as MC
import _par_reader as PR

SEED = 79                       # of the drawn constraints: the floors of the first test hold for it


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def table_set(which):
    par = LP.builtin_par()
    if which == "multiloops_win":
        par = LP.index_sensitive_par(par)
        par.update(ml_closing=-700, ml_intern=-300)
    elif which.startswith("tie"):
        par = LP.tie_par(par, LP.TIE_ML[int(which[3:])])
    if which != "builtin":
        oracle.set_tables(PR.tables_at(par, 37.0))
    return PR.tables_at(par, 37.0)


_ENUM = {}


def enumerated(which, s):
    """(rows, oracle energies) of every structure of s under the installed table set"""
    if (which, s) not in _ENUM:
        rows = MF.enumerate_structures(s)
        _ENUM[which, s] = (rows, [oracle.eval_structure(s, r) for r in rows])
    return _ENUM[which, s]


def filtered(which, s, con, u, b):
    """{row: objective} of the structures of s that satisfy con"""
    rows, en = enumerated(which, s)
    return {r: e + MC.pseudo(r, u, b) for r, e in zip(rows, en) if MC.satisfies(r, con)}


def test_helpers_on_hand_made_rows():
    assert MC.satisfies("(((...)))", "(x|...<>)") is False                          # x at a paired position
    assert MC.satisfies("(((...)))", "(.|xxx.>)") and MC.satisfies("(((...)))", "<<<...>>>") and MC.satisfies(".........", "...xxx...")
    assert not MC.satisfies(".((...)).", "(.......)") and not MC.satisfies("(((...)))", ">........") and not MC.satisfies(".........", "|........")
    assert not MC.satisfies("((.....))", "(((...)))") and MC.satisfies("(((...)))", None)
    u, b = np.arange(1, 10), np.array([1, 10, 100, 0, 0, 0, 1000, 10000, 100000])
    assert MC.pseudo(".........", u, b) == 45 and MC.pseudo("(((...)))", u, None) == 4 + 5 + 6
    assert MC.pseudo("(((...)))", None, b) == (1 + 100000 + 10 + 10000) + (10 + 10000 + 100 + 1000)     # two stacks, the hairpin's pair closes none
    assert MC.pseudo("(.(...).)", u, b) == 2 + 4 + 5 + 6 + 8                        # no pair stacked directly
    rng = np.random.default_rng(1)
    cons = [MC.draw_constraint(rng, "GGGAAACCCA") for _ in range(400)]
    assert all(len(c) == 10 and set(c) <= set(".x|<>()") and c.count("(") == c.count(")") <= 1 for c in cons)
    assert 150 <= sum("(" in c for c in cons) <= 250 and all(c.index(")") - c.index("(") >= 4 for c in cons if "(" in c)


@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_mirror_is_the_minimum_over_every_structure_that_satisfies_the_constraint(which):
    mirror, full = MC.ConMirror(table_set(which)), MF.Mirror(table_set(which))
    cases = MC.exhaustive_cases(SEED)
    seqs = MC.short_sequences()
    assert len(cases) == 144 and len(seqs) == 24 and min(map(len, seqs)) == 8 and max(map(len, seqs)) == 20
    n_feasible = n_differ = n_infeasible = 0
    chars = dict.fromkeys("x|<>()", 0)
    for s, con, u, b in cases:
        inside = filtered(which, s, con, u, b)
        dcal, row = mirror.fold(s, con)
        if not inside:
            assert dcal is None and row is None, (which, s, con)
            n_infeasible += 1
            continue
        assert dcal == min(inside.values()) == mirror.mfe(s, con), (which, s, con)
        assert row in inside and inside[row] == dcal and mirror.pseudo == 0, (which, s, con, row)
        n_feasible += 1
        n_differ += dcal != full.mfe(s)
        for c in set(con) & set(chars):
            chars[c] += 1
    print(f"\n{which}: {n_feasible} feasible, {n_differ} of them above the free minimum, {n_infeasible} infeasible; {chars}")
    assert n_feasible >= 40 and n_differ >= 30 and n_infeasible >= 10 and min(chars.values()) >= 10
    for s in seqs:                                                                  # no constraint, an all-'.' string, zeros: Mirror itself
        want = full.fold(s, "first")
        assert mirror.fold(s) == want == mirror.fold(s, "." * len(s), np.zeros(len(s), int), np.zeros(len(s), int))
        assert mirror.fold(s, order="last") == full.fold(s, "last")


def test_mirror_with_soft_terms_alone_and_with_hard_constraints():
    which = "builtin"
    mirror, full = MC.ConMirror(table_set(which)), MF.Mirror(table_set(which))
    cases = MC.exhaustive_cases(SEED, soft=True)
    assert len(cases) == 24 * 7 and sum(c[1] is None for c in cases) == 24
    n_feasible = n_soft_only_differ = n_positive = 0
    for s, con, u, b in cases:
        assert np.abs(u).max() <= 150 and -200 <= b.min() and b.max() <= 100
        inside = filtered(which, s, con, u, b)
        dcal, row = mirror.fold(s, con, u, b)
        if not inside:
            assert dcal is None
            continue
        assert dcal == min(inside.values()), (s, con, u, b)
        assert row in inside and inside[row] == dcal and mirror.pseudo == MC.pseudo(row, u, b), (s, con, row)
        assert oracle.eval_structure(s, row) == dcal - mirror.pseudo
        n_feasible += 1
        n_positive += dcal > 0
        n_soft_only_differ += con is None and row != full.fold(s, "first")[1]
    assert n_feasible >= 60 and n_soft_only_differ >= 5 and n_positive >= 3          # with u the open chain is no longer 0
    # u alone and b alone
    s = "GGGAAACCCAGGGAAACCCA"
    for u, b in ((np.full(20, 150), None), (None, np.full(20, 100)), (np.full(20, -150), None), (None, np.full(20, -200))):
        inside = filtered(which, s, None, u, b)
        dcal, row = mirror.fold(s, None, u, b)
        assert dcal == min(inside.values()) == inside[row] and mirror.pseudo == MC.pseudo(row, u, b)


@pytest.mark.parametrize("which", ["multiloops_win", "tie0", "tie1"])
def test_both_candidate_orders_return_rows_of_the_constrained_co_optimal_set(which):
    mirror = MC.ConMirror(table_set(which))
    n_two = 0
    for s, con, u, b in MC.exhaustive_cases(SEED)[::2] + [(s, "." * len(s), None, None) for s in LP.tie_short_sequences()[:6]]:
        inside = filtered(which, s, con, u, b)
        first, last = mirror.fold(s, con, order="first"), mirror.fold(s, con, order="last")
        if not inside:
            assert first == last == (None, None)
            continue
        best = min(inside.values())
        co = {r for r, e in inside.items() if e == best}
        assert first[0] == last[0] == best and first[1] in co and last[1] in co, (which, s, con)
        n_two += first[1] != last[1]
    print(f"\n{which}: the two orders differ on {n_two} cases")
    if which != "multiloops_win":
        assert n_two >= 5


def test_shape_deigan_on_hand_computed_values():
    got = rafft_amd.shape_deigan([0.0, np.e - 1, -1.0, float("nan"), -999.0, 1.0, 0.5])
    assert got.dtype == np.int32 and got.tolist() == [-60, 120, 0, 0, 0, 65, 13]       # 100 (1.8 ln 2 - 0.6) = 64.77; 100 (1.8 ln 1.5 - 0.6) = 12.98
    assert rafft_amd.shape_deigan([0.0, np.e - 1], m=1.0, b=0.0).tolist() == [0, 100]
    assert rafft_amd.shape_deigan([1e300, 0.0], m=1.8, b=-1000.0).tolist() == [_native.MFE_SOFT_MAX, -_native.MFE_SOFT_MAX]
    assert rafft_amd.shape_deigan([]).tolist() == []


def test_record_size_and_entry_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    assert ctypes.sizeof(_native.MfeConSeq) == 24 and [f[0] for f in _native.MfeConSeq._fields_] == ["status", "length", "dcal", "n_pairs", "pseudo_dcal", "_pad"]
    assert re.search(r"\}\s*rafft_mfe_con_seq;\s*/\* 24 bytes \*/", hdr)
    assert int(re.search(r"#define RAFFT_MFE_SOFT_MAX (\d+)", hdr).group(1)) == _native.MFE_SOFT_MAX == 20000
    assert int(re.search(r"RAFFT_ERR_INFEASIBLE = (\d+)", hdr).group(1)) == _native.ERR_INFEASIBLE == 10
    assert "rafft_mfe_constrained_batch" in _native.EXPORTS
    proto = re.search(r"int rafft_mfe_constrained_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_mfe_constrained_batch.argtypes) == 11
    assert {"mfe_constrained", "mfe_constrained_batch", "mfe_constrained_batch_raw", "shape_deigan"} <= set(dir(rafft_amd))


def test_host_pure_part_builds_and_passes_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "hostcheck", "mfe_con_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("mfe_con_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and " checks, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr


def test_bad_arguments_need_no_device():
    L = _native.lib()
    buf = ctypes.create_string_buffer(16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.MfeConSeq * 1)()
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    call = L.rafft_mfe_constrained_batch
    assert call(-1, seq, ln, 37.0, None, None, None, 0, 0, rec, out) == _native.ERR_PARAM
    assert call(1, None, ln, 37.0, None, None, None, 0, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, None, 37.0, None, None, None, 0, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, 0, 0, None, out) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, 0, 0, rec, None) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, -1, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, L.rafft_mfe_lds_len() + 1, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, ln, 37.0, None, None, None, 0, -1, rec, out) == _native.ERR_PARAM
    assert call(0, None, None, 37.0, None, None, None, 0, 0, None, None) == _native.OK
    # a soft value beyond the bound is an error of the call, before anything is launched
    for bad, where in ((20001, "soft_unpaired"), (-20001, "soft_stack")):
        soft = [0] * 9
        soft[4] = bad
        with pytest.raises(_native.RafftError) as e:
            zuker.mfe_constrained_batch_raw(["GGGAAACCC"], **{where: [soft]})
        assert e.value.code == _native.ERR_PARAM and "RAFFT_MFE_SOFT_MAX" in str(e.value) and "position 4" in str(e.value)
    with pytest.raises(_native.RafftError) as e:                                   # the temperature is checked first, as the fold checks it
        zuker.mfe_constrained_batch_raw(["GGGAAACCC"], ["(((...)))"], temp=25.0)
    assert e.value.code == _native.ERR_TEMP
    with pytest.raises(ValueError):
        zuker.mfe_constrained_batch_raw(["GGGAAACCC"], ["(((...)))", "."])
    with pytest.raises(ValueError):
        zuker.mfe_constrained_batch_raw(["GGGAAACCC"], soft_stack=[[0] * 8])


MALFORMED = ["(((...))", "(((...))).", "", "(((...)).", ".((...)))", ")(.......", "...(...).", "(.)......", ".(..)....", "[[[...]]]", "(((.X.)))", "((((.))))"]


def test_every_host_detected_error_of_a_sequence_without_a_device():
    """a batch of nothing but erroneous sequences never reaches the device: every malformed string is that sequence's
    RAFFT_ERR_STRUCT, the sequence's own errors come first, the first error in input order is named"""
    seqs = ["GGGAAACCC"] * len(MALFORMED)
    rows, dcal, n_pairs, pseudo, status = zuker.mfe_constrained_batch_raw(seqs, MALFORMED)
    assert status == [_native.ERR_STRUCT] * len(MALFORMED)
    assert rows == ["." * 9] * len(MALFORMED) and dcal == n_pairs == pseudo == [0] * len(MALFORMED)
    assert _native.lib().rafft_last_error().decode().startswith("sequence 0: a constraint string of another length")
    too_long = "A" * (_native.MFE_MAX_LEN + 1)
    seqs = ["GGGAAACCC", too_long, "", "GGGTAACCC", "GGGAAACCC"]
    rows, dcal, n_pairs, pseudo, status = zuker.mfe_constrained_batch_raw(seqs, ["(((..)))).", None, "(", "(((...)))", "((.....)"])
    assert status == [_native.ERR_STRUCT, _native.ERR_TOO_LONG, _native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_STRUCT]
    assert rows == ["." * 9, "." * len(too_long), "", "." * 9, "." * 9] and dcal == [0] * 5
    assert _native.lib().rafft_last_error().decode().startswith("sequence 0: a constraint")
    zuker.mfe_constrained_batch_raw(seqs[1:], [None, "(", "(((...)))", "((.....)"])
    assert _native.lib().rafft_last_error().decode() == "sequence 0: longer than RAFFT_MFE_MAX_LEN"
    assert rafft_amd.mfe_constrained_batch(seqs, ["(((..)))).", None, "(", "(((...)))", "((.....)"], raise_errors=False) == [None] * 5
    with pytest.raises(ValueError, match="malformed constraint"):
        rafft_amd.mfe_constrained("GGGAAACCC", "(((...))")
    with pytest.raises(ValueError, match="4096 nt"):
        rafft_amd.mfe_constrained(too_long, None)
    with pytest.raises(KeyError):
        rafft_amd.mfe_constrained("GGGTAACCC", "(((...)))")


def test_cli_constraint_and_shape_options(tmp_path, capsys):
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--mfe", "-C", "--shape", "r.shape", "--shape-slope", "2.0", "--shape-intercept", "-0.5"])
    assert a.mfe and a.constraint and a.shape == "r.shape" and a.shape_slope == 2.0 and a.shape_intercept == -0.5
    d = cli.parse_arguments(["-s", "GGGAAACCC", "--mfe"])
    assert not d.constraint and d.shape is None and d.shape_slope == 1.8 and d.shape_intercept == -0.6
    for argv in (["-s", "GGGAAACCC", "-C"], ["-s", "GGGAAACCC", "--shape", "x"], ["-s", "GGGAAACCC", "--pf", "-C"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--mfe" in str(e.value)
    for argv in (["-s", "GGGAAACCC", "--mfe", "--span", "40", "-C"], ["-s", "GGGAAACCC", "--mfe", "--span", "40", "--shape", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--span" in str(e.value)
    # the file formats: a constraint line after every sequence; `position reactivity` lines, 1-based, blocks introduced by >name
    fa = tmp_path / "seqs.fa"
    fa.write_text(">a\nGGGAAACCC\n(((...)))\n>b\nGGGGAAAACCCC\n....xxxx....\n")
    seqs, cons, names = cli.read_constrained_fasta(str(fa))
    assert seqs == ["GGGAAACCC", "GGGGAAAACCCC"] and cons == ["(((...)))", "....xxxx...."] and names == ["a", "b"]
    sh = tmp_path / "r.shape"
    sh.write_text(">a\n1 0.0\n3 1.718281828459045\n4 -999\n>b\n12 0.5\n")
    react = cli.read_shape(str(sh), [9, 12], batch=True)
    assert [len(r) for r in react] == [9, 12] and react[0][0] == 0.0 and react[0][3] < 0 and np.isnan(react[0][1]) and react[1][11] == 0.5
    assert rafft_amd.shape_deigan(react[0]).tolist() == [-60, 0, 120, 0, 0, 0, 0, 0, 0]
    one = tmp_path / "one.shape"
    one.write_text("2 0.0\n9 1.0\n")
    assert rafft_amd.shape_deigan(cli.read_shape(str(one), [9], batch=False)[0]).tolist() == [0, -60, 0, 0, 0, 0, 0, 0, 65]
    for text in ("10 0.5\n", "0 0.5\n", "x y\n"):
        one.write_text(text)
        with pytest.raises(SystemExit):
            cli.read_shape(str(one), [9], batch=False)
    # the output: the line of --mfe with the pseudo-energy as one more column
    seen = {}

    def fake(sequences, constraints, soft_unpaired, soft_stack, temp):
        seen.update(sequences=sequences, constraints=constraints, soft_unpaired=soft_unpaired, soft_stack=soft_stack)
        return [zuker.ConstrainedStructure("(((...)))", -2950, -29.5, 120)]
    one.write_text("1 0.0\n")
    cli.main(["-s", "GGGAAACCC", "--mfe", "--shape", str(one)], mfe_constrained_batch=fake)
    assert capsys.readouterr().out == "GGGAAACCC 9 (((...))) -29.5 3 1.2\n"
    assert seen["constraints"] is None and seen["soft_unpaired"] is None and seen["soft_stack"][0].tolist() == [-60] + [0] * 8
    cli.main(["-sf", str(fa), "--batch", "--mfe", "-C"], mfe_constrained_batch=lambda *a: (seen.update(constraints=a[1]), [fake(*a)[0]] * 2)[1])
    assert seen["constraints"] == ["(((...)))", "....xxxx...."] and capsys.readouterr().out.count("\n") == 2
    # with --scores the input is a CSV: the constraints are its column `constraint`
    csvf = tmp_path / "known.csv"
    csvf.write_text("seq,struct,name,constraint\nGGGAAACCC,(((...))),a,(.......)\n")
    table = dict(pick_first=[0], pick_ppv=[0], row0=[0], n_known=[3], seq_status=[0], n_pred=[3], hit_pred=[3], hit_known=[3])
    cli.main(["-sf", str(csvf), "--batch", "--mfe", "-C", "--scores", str(tmp_path / "scores.csv")], mfe_constrained_batch=fake, scorer=lambda beams, known: table)
    assert seen["constraints"] == ["(.......)"] and (tmp_path / "scores.csv").read_text().splitlines()[1] == "GGGAAACCC,9,(((...))),-29.5,3,100.0,100.0,a"
    csvf.write_text("seq,struct,name\nGGGAAACCC,(((...))),a\n")
    with pytest.raises(SystemExit, match="constraint"):
        cli.main(["-sf", str(csvf), "--batch", "--mfe", "-C", "--scores", str(tmp_path / "scores.csv")], mfe_constrained_batch=fake)
