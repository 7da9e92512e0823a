"""The host side of the dimer folds (rafft_cofold_batch, rafft_amd.cofold_batch, `rafft --cofold`) and the
tests' mirror of them: under four table sets the mirror's energy is the minimum of the definition (`dimer_energy`, loop by loop)
over every structure of the dimer, its row has that energy, swapping the strands changes nothing, a dimer never lies above its
two strands, cut 0 is the single-strand mirror, the two candidate orders differ where tables tie, and a mirror whose multiloops
forget the nick is caught; the cuts and sizes of the host-pure code (tests/hostcheck/cofold_check.cpp, plain and under sanitizers),
every error the host detects, the `&` parsing and the option surface.  Integers and bytes: no tolerance.  No GPU.

The case set: 40 dimers of seed SEED, strands of 3-8 nt, at most 14 nt in all - 28 drawn G/C/U-rich, 4 of two 5-nt hairpins around
the nick inside a closing pair, 8 with one of the eight 8-nt hairpins that lie below 0 under the built-in tables.  The floors are
counted where they can be met: under the built-in tables a hairpin needs 8 of the 14 positions to pay for itself, so no optimum
there holds an intra and an inter pair; "multiloops win" has them."""
import ctypes
import importlib
import os
import subprocess

import pytest

from rafft_amd import _native, cli, params
import rafft_amd
from conftest import ROOT
import _cofold_np as CF
import _loops as LP
import _mfe_np as MF
import _par_reader as PR

cofold = importlib.import_module("rafft_amd.cofold")        # (the package's attribute `cofold` is the function)

SEED = 1                        # of the drawn dimers: the floors below hold for it
DINIT = 410


def cases():
    return CF.draw_dimers(SEED, 40, n_hairpin=8, n_two=4)


def table_set(which):
    par = LP.builtin_par()
    if which == "multiloops_win":
        par = LP.index_sensitive_par(par)
        par.update(ml_closing=-700, ml_intern=-300)
    elif which.startswith("tie"):
        par = LP.tie_par(par, LP.TIE_ML[int(which[3:])])
    return PR.tables_at(par, 37.0)


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    params.reset_params()


def test_the_case_set():
    cs = cases()
    assert len(cs) == 40 == len(set(cs))
    for seq, c in cs:
        assert 3 <= c <= 8 and 3 <= len(seq) - c <= 8 and len(seq) <= 14 and set(seq) <= set("ACGU")
    assert CF.enumerate_dimer("GC", 1) == ["..", "()"] and CF.enumerate_dimer("GAAAC", 2) == [".....", "(...)"]
    full = MF.Mirror(table_set("builtin"))
    assert all(full.mfe(h) < 0 and len(h) == 8 for h in CF.STABLE_HAIRPINS)


@pytest.mark.parametrize("which", ["builtin", "multiloops_win", "tie0", "tie1"])
def test_mirror_is_the_minimum_of_the_definition_over_every_structure(which):
    tables = table_set(which)
    mirror, full = CF.CutMirror(tables, DINIT), MF.Mirror(tables)
    implied, forgets = CF.CutMirror(tables, DINIT, defect="split_k"), CF.CutMirror(tables, DINIT, defect="branch_start")
    n = dict(inter=0, both=0, apart_below_0=0, multiloop=0, orders_differ=0, caught=0)
    for seq, c in cases():
        rows = CF.enumerate_dimer(seq, c)
        en = [CF.dimer_energy(mirror, seq, c, r, DINIT) for r in rows]
        best = min(en)
        assert mirror.mfe_cut(seq, c) == best, (which, seq, c, rows[en.index(best)])
        dcal, row, n_inter = mirror.fold_cut(seq, c)
        assert dcal == best and row in rows and CF.dimer_energy(mirror, seq, c, row, DINIT) == dcal, (which, seq, c, row)
        pt = CF.pair_table(row)
        assert n_inter == sum(1 for x, y in enumerate(pt) if x < c <= y)
        last = mirror.fold_cut(seq, c, "last")
        assert last[0] == best and CF.dimer_energy(mirror, seq, c, last[1], DINIT) == best
        # swapping the strands: the exterior loop and the loop with the nick trade places
        assert mirror.mfe_cut(seq[c:] + seq[:c], len(seq) - c) == best, (which, seq, c)
        assert best <= full.mfe(seq[:c]) + full.mfe(seq[c:])
        n["inter"] += n_inter > 0
        n["both"] += 0 < n_inter < row.count("(")
        n["apart_below_0"] += n_inter == 0 and best < 0
        n["multiloop"] += CF.multiloop_with_cross_branch(row, c)
        n["orders_differ"] += last[1] != row
        # the k != c of the splits is implied by M1's i != c: dropping it alone changes no value; dropping both is a wrong model
        assert implied.mfe_cut(seq, c) == best
        n["caught"] += forgets.mfe_cut(seq, c) != best
    print(f"\n{which}: {n}")
    if which == "builtin":
        assert n["inter"] >= 15 and n["apart_below_0"] >= 5
    if which == "multiloops_win":
        assert n["both"] >= 5 and n["multiloop"] >= 3 and n["caught"] >= 1
    if which == "tie1":
        assert n["orders_differ"] >= 1


def test_cut_0_is_the_single_strand_mirror():
    tables = table_set("builtin")
    mirror, full = CF.CutMirror(tables, DINIT), MF.Mirror(tables)
    for seq, _ in cases()[:10]:
        for order in ("first", "last"):
            assert mirror.fold_cut(seq, 0, order) == full.fold(seq, order) + (0,)
        assert mirror.mfe_cut(seq, 0) == full.mfe(seq)


def test_host_pure_part_builds_and_passes_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "hostcheck", "cofold_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("cofold_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and " checks, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr


def test_bad_arguments_need_no_device(tmp_path):
    L = _native.lib()
    assert ctypes.sizeof(_native.CofoldSeq) == 24
    buf = ctypes.create_string_buffer(16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.CofoldSeq * 1)()
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    cut = (ctypes.c_int * 1)(4)
    call = L.rafft_cofold_batch
    assert call(-1, seq, ln, cut, 37.0, 0, 0, rec, out) == _native.ERR_PARAM
    assert call(1, None, ln, cut, 37.0, 0, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, None, cut, 37.0, 0, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, ln, cut, 37.0, 0, 0, None, out) == _native.ERR_PARAM
    assert call(1, seq, ln, cut, 37.0, 0, 0, rec, None) == _native.ERR_PARAM
    assert call(1, seq, ln, cut, 37.0, -1, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, ln, cut, 37.0, L.rafft_mfe_lds_len() + 1, 0, rec, out) == _native.ERR_PARAM
    assert call(1, seq, ln, cut, 37.0, 0, -1, rec, out) == _native.ERR_PARAM
    assert call(0, None, None, None, 37.0, 0, 0, None, None) == _native.OK
    with pytest.raises(_native.RafftError) as e:                                   # the temperature is checked first, as the fold checks it
        cofold.cofold_batch_raw(["GGGAAACCC"], [4], temp=25.0)
    assert e.value.code == _native.ERR_TEMP
    with pytest.raises(ValueError):
        cofold.cofold_batch_raw(["GGGAAACCC"], [4, 1])
    # duplex_init: Turner 2004's 410 with the built-in tables, the file's own value once one is loaded; no device needed
    assert rafft_amd.cofold_duplex_init() == 410
    with pytest.raises(_native.RafftError) as e:
        rafft_amd.cofold_duplex_init(25.0)
    assert e.value.code == _native.ERR_TEMP
    assert L.rafft_cofold_duplex_init(37.0, None) == _native.ERR_PARAM
    par = PR.synthetic_par(LP.builtin_par())
    par.update(duplex_init=360, duplex_init_dH=900)
    PR.write_par(par, tmp_path / "cofold.par", comment="cofold")
    params.load_params(tmp_path / "cofold.par")
    assert rafft_amd.cofold_duplex_init() == 360
    tempf = (25.0 + 273.15) / (37.0 + 273.15)
    assert rafft_amd.cofold_duplex_init(25.0) == int(900 - (900 - 360) * tempf)


def test_every_host_detected_error_of_a_sequence_without_a_device():
    """a batch of nothing but erroneous sequences never reaches the device: a cut outside 0 .. len - 1 is that sequence's
    RAFFT_ERR_STRUCT, the sequence's own errors come first, the first error in input order is named"""
    too_long = "A" * (_native.MFE_MAX_LEN + 1)
    seqs = ["GGGAAACCC", too_long, "", "GGGTAACCC", "GGGAAACCC", "GC"]
    rows, dcal, n_pairs, n_inter, cut, status = cofold.cofold_batch_raw(seqs, [9, 5, 0, 4, -1, 2])
    assert status == [_native.ERR_STRUCT, _native.ERR_TOO_LONG, _native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_STRUCT, _native.ERR_STRUCT]
    assert rows == ["." * 9, "." * len(too_long), "", "." * 9, "." * 9, ".."] and dcal == n_pairs == n_inter == cut == [0] * 6
    assert _native.lib().rafft_last_error().decode() == "sequence 0: cut outside 0 .. length - 1"
    cofold.cofold_batch_raw(seqs[1:], [5, 0, 4, -1, 2])
    assert _native.lib().rafft_last_error().decode() == "sequence 0: longer than RAFFT_MFE_MAX_LEN"
    assert rafft_amd.cofold_batch([("GGGTAA", "CCC")], raise_errors=False) == [None]
    with pytest.raises(KeyError):
        rafft_amd.cofold("GGGTAA", "CCC")
    for bad in ("GGGAAACCC", "GGG&AAA&CCC"):
        with pytest.raises(ValueError, match="one '&'"):
            rafft_amd.cofold_batch([bad])
    for bad in ("&GGG", "GGG&"):
        with pytest.raises(ValueError, match="empty strand"):
            rafft_amd.cofold_batch([bad])
    assert cofold.split_dimer("GGG&CC") == ("GGG", "CC")
    assert {"cofold", "cofold_batch", "cofold_batch_raw", "cofold_duplex_init", "CofoldResult"} <= set(dir(rafft_amd))
    assert {"rafft_cofold_batch", "rafft_cofold_duplex_init"} <= set(_native.EXPORTS)


def test_cli_cofold_option(tmp_path, capsys):
    a = cli.parse_arguments(["-s", "GGG&CCC", "--cofold", "--binding"])
    assert a.cofold and a.binding and not cli.parse_arguments(["-s", "GGG"]).cofold
    for argv, word in ((["-s", "GGG&CCC", "--binding"], "--cofold"), (["-s", "GGG&CCC", "--cofold", "--mfe"], "other modes"),
                       (["-s", "GGG&CCC", "--cofold", "--pf"], "other modes"), (["-s", "GGG&CCC", "--cofold", "-C"], "need --mfe"),
                       (["-s", "GGG&CCC", "--cofold", "--span", "9"], "needs --mfe"), (["-s", "GGG&CCC", "--cofold", "--traj"], "other modes"), (["-sf", "x.fa", "--cofold"], "--batch")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert word in str(e.value), argv
    fa = tmp_path / "dimers.fa"
    fa.write_text(">a\nGGGG&CCCC\n>b\nGGGAAACCC\n")
    with pytest.raises(SystemExit, match="record 1"):
        cli.main(["-sf", str(fa), "--batch", "--cofold"])
    with pytest.raises(SystemExit, match="record 0"):
        cli.main(["-s", "GG&G&CC", "--cofold"])
    with pytest.raises(SystemExit, match="record 0"):
        cli.main(["-s", "&GGCC", "--cofold"])
    seen = {}

    def fake(dimers, temp, monomers):
        seen.update(dimers=dimers, temp=temp, monomers=monomers)
        out = []
        for _ in dimers:
            r = cofold.CofoldResult("((((&))))", -530, -5.3, 4)
            r.energy_a, r.energy_b, r.binding = 0.0, -0.5, -4.8
            out.append(r)
        return out
    fa.write_text(">a\nGGGG&CCCC\n>b\nGGTG&CACC\n")
    cli.main(["-sf", str(fa), "--batch", "--cofold"], cofold_batch=fake)
    assert capsys.readouterr().out == "GGGG&CCCC 8 ((((&)))) -5.3 4\nGGUG&CACC 8 ((((&)))) -5.3 4\n"
    assert seen == dict(dimers=["GGGG&CCCC", "GGUG&CACC"], temp=37.0, monomers=False)
    cli.main(["-s", "GGGG&CCCC", "--cofold", "--binding", "-o", str(tmp_path / "out.txt")], cofold_batch=fake)
    assert (tmp_path / "out.txt").read_text() == "GGGG&CCCC 8 ((((&)))) -5.3 4 -5.3 0.0 -0.5 -4.8\n" and seen["monomers"] is True
    r = fake(["x"], 37.0, False)[0]
    assert r.row == r.str_struct == "((((&))))" and r.n_inter == 4 and r.dcal == -530 and r.pair_list == rafft_amd.paired_positions("(((())))")
