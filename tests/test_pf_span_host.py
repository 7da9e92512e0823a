"""The host side of the partition function under a base-pair span (rafft_pf_span_batch, rafft_amd.pf_span_batch, `rafft --pf --pf-span
W`) and the tests' mirror of it: the mirror's Z, every P(i,j) and every unpaired probability equal the sums over every structure of
a short sequence that obeys the span, under the oracle's energies; at span >= L it is PfMirror itself; the energy never falls as the
span shrinks; the layout of the call (tests/hostcheck/pf_span_check.cpp, plain and under sanitizers), the option surface, the banded
helpers and the errors that need no device.  No GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from rafft_amd import _native, cli, params
import rafft_amd
from conftest import ROOT
import _loops as LP
import _mfe_np as MF
import _par_reader as PR
import _pf_np as PF
import _pf_span_np as PS
from test_pf_host import short_sequences


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def spans_of(L):
    return sorted({1, 4, 5, 6, 8, 12, max(L - 1, 1), L})


def table_set(which):
    par = LP.builtin_par()
    if which != "builtin":
        par = LP.index_sensitive_par(par)
        par.update(ml_closing=-700, ml_intern=-300)
        oracle.set_tables(PR.tables_at(par, 37.0))
    return PR.tables_at(par, 37.0)


@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_span_mirror_equals_the_sums_over_every_structure_that_obeys_the_span(which):
    tabs = table_set(which)
    full = PF.PfMirror(tabs)
    kt = PF.kt_of(37.0)
    worst_z = worst_p = worst_u = 0.0
    n_bound = 0
    for s in short_sequences():
        rows = MF.enumerate_structures(s)
        en = dict(zip(rows, (oracle.eval_structure(s, r) for r in rows)))
        last = None
        for span in spans_of(len(s)):
            inside = PS.rows_within(rows, span)
            Z, P = PF.exact(inside, [en[r] for r in inside], kt)
            Zm, Pm, Um = PS.PfSpanMirror(tabs, span).run(s)
            worst_z, worst_p = max(worst_z, abs(Zm / Z - 1.0)), max(worst_p, float(np.abs(Pm - P).max()))
            worst_u = max(worst_u, float(np.abs(Um - PS.unpaired_of(P)).max()))
            assert abs(Zm / Z - 1.0) <= 1e-10, (which, s, span)
            assert np.abs(Pm - P).max() <= 1e-10, (which, s, span)
            assert np.abs(Um - PS.unpaired_of(P)).max() <= 1e-10, (which, s, span)
            i, j = np.nonzero(Pm)
            assert not len(i) or (j - i + 1).max() <= span
            if span <= 4:
                assert Zm == 1.0 and not Pm.any() and (Um == 1.0).all()
            assert last is None or Zm >= last * (1.0 - 1e-12), (which, s, span)        # a wider span only adds structures
            last = Zm
            n_bound += len(inside) < len(rows) and Z < math.fsum(math.exp(-e / (100.0 * kt)) for e in en.values()) * (1.0 - 1e-6)
        Zf, Pf = full.run(s)
        for span in (len(s), 4096):
            Zm, Pm, _ = PS.PfSpanMirror(tabs, span).run(s)
            assert Zm == Zf and np.array_equal(Pm, Pf), (which, s, span)
    print(f"\n{which}: largest relative error of Z {worst_z:.3g}, largest error of P {worst_p:.3g}, of unpaired {worst_u:.3g}; the span binds in {n_bound} cases")
    assert n_bound >= 10


def test_span_mirror_at_longer_sequences():
    """at 69 nt, where enumeration cannot reach: span >= L is PfMirror bit for bit, the energy never falls as the span shrinks, no
    probability beyond the span"""
    tabs = table_set("builtin")
    s = "GGGCGCAAGCGCCCAAAAGGGCGCAAGCGCCCAAAAGGGCGCAAGCGCCCAAAGGCGCAAGCGCCAAAA"
    full = PF.PfMirror(tabs)
    Zf, Pf = full.run(s)
    last = None
    for span in (4096, len(s), len(s) - 1, 30, 14, 10):
        m = PS.PfSpanMirror(tabs, span)
        Z, P, U = m.run(s)
        e = m.energy(Z)
        assert last is None or e >= last - 1e-12
        last = e
        i, j = np.nonzero(P)
        assert (j - i + 1).max() <= span and 0.0 <= U.min() and U.max() <= 1.0
        if span >= len(s):
            assert Z == Zf and np.array_equal(P, Pf)
    assert PS.PfSpanMirror(tabs, 14).energy(PS.PfSpanMirror(tabs, 14).run(s)[0]) > full.energy(Zf) + 1e-3


def test_host_pure_part_builds_and_passes_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "hostcheck", "pf_span_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("pf_span_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and " checks, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr


def test_pf_span_entry_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    assert "rafft_pf_span_batch" in _native.EXPORTS
    proto = re.search(r"int rafft_pf_span_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_pf_span_batch.argtypes) == 11
    assert "48 L W + 8 (3 L + 2 W + 6) + 8 (L + 1) + L + 1" in hdr and "RNAfold -p --maxBPspan" in hdr and "BANDED" in hdr
    lay = open(os.path.join(ROOT, "rafft_amd", "csrc", "rafft_batch_layout.h")).read()
    assert "48 L W + 8 (3 L + 2 W + 6) + 8 (L + 1) + L + 1" in lay                  # the count tests/hostcheck/pf_span_check.cpp checks
    assert {"pf_span", "pf_span_batch", "pf_span_batch_raw", "band_to_dense", "band_pairs"} <= set(dir(rafft_amd))


def test_bad_arguments_need_no_device():
    L = _native.lib()
    buf = ctypes.create_string_buffer(b"untouched!", 16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.PfSeq * 1)()
    rec[0].status, rec[0].energy = 77, 7.5
    pr, un = np.full((9, 9), 3.25), np.full(9, 2.5)
    pp, up = (ctypes.c_void_p * 1)(pr.ctypes.data), (ctypes.c_void_p * 1)(un.ctypes.data)
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    for span in (0, -1, _native.MFE_MAX_LEN + 1):
        assert L.rafft_pf_span_batch(1, seq, ln, 37.0, 0.0, span, 0, rec, out, pp, up) == _native.ERR_PARAM
        assert b"max_span" in L.rafft_last_error()
    for args in ((-1, seq, ln, 37.0, 0.0, 40, 0, rec, out, pp, up), (1, None, ln, 37.0, 0.0, 40, 0, rec, out, pp, up), (1, seq, None, 37.0, 0.0, 40, 0, rec, out, pp, up),
                 (1, seq, ln, 37.0, 0.0, 40, 0, None, out, pp, up), (1, seq, ln, 37.0, 0.0, 40, 0, rec, None, pp, up), (1, seq, ln, 37.0, -1.0, 40, 0, rec, out, pp, up),
                 (1, seq, ln, 37.0, float("nan"), 40, 0, rec, out, pp, up), (1, seq, ln, 37.0, float("inf"), 40, 0, rec, out, pp, up),
                 (1, seq, ln, 37.0, 0.0, 40, -1, rec, out, pp, up)):
        assert L.rafft_pf_span_batch(*args) == _native.ERR_PARAM, args
    assert buf.value == b"untouched!" and rec[0].status == 77 and rec[0].energy == 7.5 and (pr == 3.25).all() and (un == 2.5).all()
    assert L.rafft_pf_span_batch(0, None, None, 37.0, 0.0, 40, 0, None, None, None, None) == _native.OK


def test_errors_of_a_sequence_without_a_device():
    """a batch of nothing but erroneous sequences never reaches the device; the limit named is this call's"""
    from rafft_amd import mccaskill as M
    too_long = "A" * (_native.MFE_SPAN_MAX_LEN + 1)
    rows, recs, probs, un = M.pf_span_batch_raw([too_long, "", "GGGTAACCC"], 40)
    assert [r["status"] for r in recs] == [_native.ERR_TOO_LONG, _native.ERR_EMPTY, _native.ERR_BAD_CHAR]
    assert rows == ["." * len(too_long), "", "." * 9]
    assert all(r["energy"] == 0.0 and r["mfe_frequency"] == 0.0 and r["n_pairs"] == 0 and r["mfe_dcal"] == 0 for r in recs)
    assert probs[0] is None and un[0] is None and probs[2].shape == (9, 9) and not probs[2].any() and not un[2].any()
    assert _native.lib().rafft_last_error().decode() == "sequence 0: longer than RAFFT_MFE_SPAN_MAX_LEN"
    with pytest.raises(ValueError, match="32768 nt"):
        rafft_amd.pf_span(too_long, 40)
    with pytest.raises(KeyError):
        rafft_amd.pf_span("GGGTAACCC", 40)
    with pytest.raises(_native.RafftError) as e:             # the temperature is checked first, as the fold checks it
        M.pf_span_batch_raw(["", "GGGXAACCC"], 40, temp=25.0)
    assert e.value.code == _native.ERR_TEMP
    with pytest.raises(_native.RafftError) as e:
        M.pf_span_batch_raw(["GGGAAACCC"], 0)
    assert e.value.code == _native.ERR_PARAM
    assert rafft_amd.pf_span_batch(["", "GGGXAACCC"], 40, raise_errors=False) == [None, None]


def test_band_helpers():
    rng = np.random.default_rng(3)
    L, W = 9, 6
    dense = np.triu(rng.random((L, L)), 1)
    i, j = np.indices((L, L))
    dense[j - i >= W] = 0.0
    band = PS.dense_to_band(dense, W)
    assert band.shape == (L, W) and np.array_equal(rafft_amd.band_to_dense(band), dense)
    assert np.array_equal(rafft_amd.band_to_dense(np.zeros((1, 1))), np.zeros((1, 1)))
    wide = np.triu(rng.random((L, L)), 1)                                                          # a band as wide as the sequence
    assert np.array_equal(rafft_amd.band_to_dense(PS.dense_to_band(wide, L)), wide)
    band[:] = 0.0
    band[0, 5], band[0, 4], band[3, 5], band[2, 4], band[8, 4] = 0.5, 0.25, 1e-5, 9e-6, 0.9       # [8][4] lies beyond the sequence
    assert rafft_amd.band_pairs(band, 1e-5) == [(0, 4, 0.25), (0, 5, 0.5), (3, 8, 1e-5)]
    assert rafft_amd.band_pairs(band, 0.3) == [(0, 5, 0.5)]
    assert rafft_amd.band_pairs(band) == rafft_amd.band_pairs(band, 1e-5)
    from rafft_amd.mccaskill import dense_pairs
    band[8, 4] = 0.0
    assert dense_pairs(rafft_amd.band_to_dense(band), 1e-5) == rafft_amd.band_pairs(band, 1e-5)


def test_cli_pf_span_option(tmp_path, capsys):
    from rafft_amd.mccaskill import PfResult
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--pf", "--pf-span", "150", "--bpp", "p.txt"])
    assert a.pf and a.pf_span == 150 and a.span is None and a.bpp == "p.txt" and a.bpp_cutoff == 1e-5
    assert cli.parse_arguments(["-s", "GGGAAACCC", "--pf"]).pf_span is None
    for argv in (["-s", "GGGAAACCC", "--span", "40"], ["-s", "GGGAAACCC", "--pf", "--span", "40"]):      # --span keeps its meaning
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--mfe" in str(e.value)
    for argv in (["-s", "GGGAAACCC", "--pf-span", "40"], ["-s", "GGGAAACCC", "--mfe", "--pf-span", "40"], ["-s", "GGGAAACCC", "--bpp", "x.txt"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--pf" in str(e.value) and "need" in str(e.value)
    for bad in ("0", "4097"):
        with pytest.raises(SystemExit) as e:
            cli.main(["-s", "GGGAAACCC", "--pf", "--pf-span", bad])
        assert "--pf-span" in str(e.value)
    band = np.zeros((9, 9))
    band[0, 8], band[1, 6], band[2, 4] = 0.9, 0.8, 1e-7
    dense = rafft_amd.band_to_dense(band)

    def stub(seqs, temp):
        return [PfResult(-3.456, "(((...)))", 0.87654321, -3.07, band, np.ones(9)) for s in seqs]

    def dense_stub(seqs, temp):
        return [PfResult(-3.456, "(((...)))", 0.87654321, -3.07, dense) for s in seqs]

    out = tmp_path / "bpp.txt"
    cli.main(["-s", "GGGAAACCC", "--pf", "--pf-span", "40", "--bpp", str(out)], pf_batch=stub)
    assert capsys.readouterr().out == "GGGAAACCC 9 (((...))) -3.46 3 0.8765\n"
    assert out.read_text().splitlines() == ["1 1 9 0.9", "1 2 8 0.8"]
    cli.main(["-s", "GGGAAACCC", "--pf", "--bpp", str(out), "--bpp-cutoff", "1e-8"], pf_batch=dense_stub)
    assert out.read_text().splitlines() == ["1 1 9 0.9", "1 2 8 0.8", "1 3 7 1e-07"]
    csvf = tmp_path / "k.csv"
    csvf.write_text("GGGAAACCC,((.....)),x1\n")
    cli.main(["-sf", str(csvf), "--batch", "--pf", "--pf-span", "40", "--bpp", str(out), "-o", str(tmp_path / "o.txt")], pf_batch=stub)
    assert out.read_text().splitlines() == ["x1 1 9 0.9", "x1 2 8 0.8"]
