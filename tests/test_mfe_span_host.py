"""The host side of the MFE folds under a base-pair span (rafft_mfe_span_batch, rafft_amd.mfe_span_batch, `rafft --mfe --span W`)
and the tests' mirror of them: the mirror equals the minimum of the oracle's energy over every structure that obeys the span, its
row is one of them, at span >= L it is Mirror itself, the energy never rises with the span; the layout of the call
(tests/hostcheck/mfe_span_check.cpp, plain and under sanitizers), the option surface and the errors that need no device.  No GPU."""
import ctypes
import os
import re
import subprocess

import pytest

import oracle
from rafft_amd import _native, cli, params
import rafft_amd
from conftest import ROOT
import _loops as LP
import _mfe_np as MF
import _mfe_span_np as MS
import _par_reader as PR
from test_mfe_host import short_sequences


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def spans_of(L):
    return sorted({1, 4, 5, 6, 8, 12, max(L - 1, 1), L})


def table_set(which):
    par = LP.builtin_par()
    if which == "multiloops_win":
        par = LP.index_sensitive_par(par)
        par.update(ml_closing=-700, ml_intern=-300)
        oracle.set_tables(PR.tables_at(par, 37.0))
    return PR.tables_at(par, 37.0)


@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_span_mirror_is_the_minimum_over_every_structure_that_obeys_the_span(which):
    tables = table_set(which)
    mirror, full = MS.SpanMirror(tables), MF.Mirror(tables)
    n_bound = 0
    for s in short_sequences():
        rows = MF.enumerate_structures(s)
        en = dict(zip(rows, (oracle.eval_structure(s, r) for r in rows)))
        last = None
        for span in spans_of(len(s)):
            inside = MS.rows_within(rows, span)
            want = min(en[r] for r in inside)
            dcal, row = mirror.fold(s, span)
            assert dcal == want == mirror.mfe(s, span), (which, s, span)
            assert row in inside and en[row] == dcal, (which, s, span)
            assert last is None or dcal <= last, (which, s, span)        # a wider span only adds structures
            last = dcal
            n_bound += want > min(en.values())
        assert mirror.fold(s, len(s)) == full.fold(s, "first") == mirror.fold(s, 4096), (which, s)
        if len(s) > 1:
            assert mirror.fold(s, 4)[1] == "." * len(s)
    assert n_bound >= 10                                                 # the span binds: the restricted minimum lies above the free one


def test_span_mirror_window_and_longer_sequences():
    """at 60-90 nt, where enumeration cannot reach: span >= L is Mirror, the energy never rises with the span, every row obeys it"""
    tables = table_set("builtin")
    mirror, full = MS.SpanMirror(tables), MF.Mirror(tables)
    s = "GGGCGCAAGCGCCCAAAAGGGCGCAAGCGCCCAAAAGGGCGCAAGCGCCCAAAGGCGCAAGCGCCAAAA"
    last = None
    for span in (10, 14, 30, len(s) - 1, len(s), 4096):
        dcal, row = mirror.fold(s, span)
        assert MS.obeys(row, span) and oracle.eval_structure(s, row) == dcal
        assert last is None or dcal <= last
        last = dcal
    assert mirror.fold(s, len(s)) == full.fold(s, "first")
    assert mirror.fold(s, 14)[0] > mirror.fold(s, len(s))[0]


def test_host_pure_part_builds_and_passes_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "hostcheck", "mfe_span_check.cpp")
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("mfe_span_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and " checks, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr


def test_mfe_span_entry_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    assert re.search(r"#define RAFFT_MFE_SPAN_MAX_LEN RAFFT_MAX_LEN\b", hdr)
    assert int(re.search(r"#define RAFFT_MAX_LEN (\d+)", hdr).group(1)) == _native.MFE_SPAN_MAX_LEN == 32768
    assert "rafft_mfe_span_batch" in _native.EXPORTS
    proto = re.search(r"int rafft_mfe_span_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_mfe_span_batch.argtypes) == 8
    assert {"mfe_span", "mfe_span_batch", "mfe_span_batch_raw"} <= set(dir(rafft_amd))


def test_bad_arguments_need_no_device():
    L = _native.lib()
    buf = ctypes.create_string_buffer(16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.MfeSeq * 1)()
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    for span in (0, -1, _native.MFE_MAX_LEN + 1):
        assert L.rafft_mfe_span_batch(1, seq, ln, 37.0, span, 0, rec, out) == _native.ERR_PARAM
        assert b"max_span" in L.rafft_last_error()
    assert L.rafft_mfe_span_batch(-1, seq, ln, 37.0, 40, 0, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_span_batch(1, None, ln, 37.0, 40, 0, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_span_batch(1, seq, None, 37.0, 40, 0, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_span_batch(1, seq, ln, 37.0, 40, 0, None, out) == _native.ERR_PARAM
    assert L.rafft_mfe_span_batch(1, seq, ln, 37.0, 40, 0, rec, None) == _native.ERR_PARAM
    assert L.rafft_mfe_span_batch(1, seq, ln, 37.0, 40, -1, rec, out) == _native.ERR_PARAM
    assert L.rafft_mfe_span_batch(0, None, None, 37.0, 40, 0, None, None) == _native.OK


def test_errors_of_a_sequence_without_a_device():
    """a batch of nothing but erroneous sequences never reaches the device; the limit named is this call's, and rafft_mfe_batch's
    text is what it was"""
    from rafft_amd import zuker as M
    too_long = "A" * (_native.MFE_SPAN_MAX_LEN + 1)
    rows, dcal, n_pairs, status = M.mfe_span_batch_raw([too_long, "", "GGGTAACCC"], 40)
    assert status == [_native.ERR_TOO_LONG, _native.ERR_EMPTY, _native.ERR_BAD_CHAR]
    assert rows == ["." * len(too_long), "", "." * 9] and dcal == [0] * 3 and n_pairs == [0] * 3
    assert _native.lib().rafft_last_error().decode() == "sequence 0: longer than RAFFT_MFE_SPAN_MAX_LEN"
    M.mfe_batch_raw(["A" * (_native.MFE_MAX_LEN + 1)])
    assert _native.lib().rafft_last_error().decode() == "sequence 0: longer than RAFFT_MFE_MAX_LEN"
    with pytest.raises(ValueError, match="32768 nt"):
        rafft_amd.mfe_span(too_long, 40)
    with pytest.raises(KeyError):
        rafft_amd.mfe_span("GGGTAACCC", 40)
    with pytest.raises(_native.RafftError) as e:             # the temperature is checked first, as the fold checks it
        M.mfe_span_batch_raw(["", "GGGXAACCC"], 40, temp=25.0)
    assert e.value.code == _native.ERR_TEMP
    assert rafft_amd.mfe_span_batch(["", "GGGXAACCC"], 40, raise_errors=False) == [None, None]


def test_cli_span_option(capsys):
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--mfe", "--span", "150"])
    assert a.mfe and a.span == 150
    assert cli.parse_arguments(["-s", "GGGAAACCC", "--mfe"]).span is None
    for argv in (["-s", "GGGAAACCC", "--span", "40"], ["-s", "GGGAAACCC", "--pf", "--span", "40"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--mfe" in str(e.value)
    for bad in ("0", "4097"):
        with pytest.raises(SystemExit) as e:
            cli.main(["-s", "GGGAAACCC", "--mfe", "--span", bad])
        assert "--span" in str(e.value)
    from rafft_amd.utils import Structure
    cli.main(["-s", "GGGAAACCC", "--mfe", "--span", "40"], mfe_batch=lambda seqs, temp: [Structure("(((...)))", -3070)])
    assert capsys.readouterr().out == "GGGAAACCC 9 (((...))) -30.700000762939453 3\n"
