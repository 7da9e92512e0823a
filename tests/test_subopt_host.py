"""The grammar of rafft_subopt_batch before any kernel runs: the tests' own walk of the decision tree
(`_subopt_np.band`) returns exactly the structures of a short sequence whose oracle energy lies in the band, each once, with the
oracle's energy, in ascending order, and its frontier never holds more states than the answer has rows - under the built-in tables,
tables under which multiloops win, and the two flat sets under which most sequences tie.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from rafft_amd import _native, params
from conftest import ROOT
import _loops as LP
import _mfe_np as MF
import _par_reader as PR
import _subopt_np as SB

MULTILOOP_SEQS = ["GAGAAACGAAACGAAACC", "GAGAAACGAAACGAAACAC", "GAAGAAACGAAACGAAACC", "GUGAAACGAAACGAAACAU", "GAGAAACGAAACGAAACCA"]
DELTAS = (0, 150, 500, 100000)
# sequences of the list with two or more co-optimal structures under the flat tables, as the walk finds them (test_mfe_host.py
# reports 8 / 16 of its 20)
FLOOR = dict(tie0=11, tie1=22)


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def rand(rng, n, letters="ACGU"):
    return "".join(rng.choice(list(letters), n))


def exhaustive_sequences():
    """the list of tests/test_gpu_pf.py"""
    rng = np.random.default_rng(1971)
    seqs = ["A", "GC", "GAC", "GAAC"]
    seqs += [rand(rng, n) for n in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20, 20, 20)]
    seqs += [rand(rng, n, "GCU") for n in (14, 16, 17)]
    for name in LP.KINDS:
        for sp in LP.OWN_SPECIAL[name]:
            seqs.append("GG" + sp + "CC")
    seqs += ["GGGACACCCAGGACCACCC", "G" * 10 + "U" * 10, "GU" * 9, "GGGUUUGGGUUUCCC", "GCGCAAAGCGCAAAGCGC", "GGGAAACCCAGGGAAACCCA", "NGGGAAACCCN"]
    return seqs + LP.N_SEQS + MULTILOOP_SEQS


def table_set(which):
    par = LP.builtin_par()
    if which == "multiloops_win":
        par = LP.index_sensitive_par(par)
        par.update(ml_closing=-700, ml_intern=-300)
    elif which != "builtin":
        par = LP.tie_par(par, LP.TIE_ML[int(which[-1])])
    if which != "builtin":
        oracle.set_tables(PR.tables_at(par, 37.0))
    return PR.tables_at(par, 37.0)


_ENUM = {}


def enumerated(s):
    if s not in _ENUM:
        _ENUM[s] = MF.enumerate_structures(s)
    return _ENUM[s]


@pytest.mark.parametrize("which", ["builtin", "multiloops_win", "tie0", "tie1"])
def test_band_is_the_set_of_enumerated_structures_in_the_band(which):
    mirror = MF.Mirror(table_set(which))
    seqs = exhaustive_sequences()
    assert max(map(len, seqs)) == 20 and sum("N" in s for s in seqs) >= 4 and set(MULTILOOP_SEQS) <= set(seqs)
    n_cooptimal = n_rows = 0
    for s in seqs:
        rows = enumerated(s)
        en = dict(zip(rows, (oracle.eval_structure(s, r) for r in rows)))
        mfe = min(en.values())
        assert mirror.mfe(s) == mfe, (which, s)
        for delta in DELTAS:
            got, stats = SB.band(mirror, s, delta, with_stats=True)
            want = {r for r, e in en.items() if e <= mfe + delta}
            assert len({r for r, _ in got}) == len(got), (which, s, delta)                      # no row twice
            assert {r for r, _ in got} == want, (which, s, delta)
            assert all(e == en[r] for r, e in got), (which, s, delta)                           # every dcal is the oracle's
            assert all(a[1] <= b[1] for a, b in zip(got, got[1:])), (which, s, delta)           # energies ascend
            assert stats["frontier"] <= len(got), (which, s, delta, stats)
            assert got[0][1] == mfe
            n_rows += len(got)
            if delta == 0:
                n_cooptimal += len(got) >= 2
            if delta == DELTAS[-1]:
                assert len(got) == len(rows)
    print(f"\n{which}: {n_rows} rows over {len(seqs)} sequences and {len(DELTAS)} bands; {n_cooptimal} sequences with two or more co-optimal structures")
    if which.startswith("tie"):
        assert n_cooptimal >= FLOOR[which]


def test_band_order_is_enumeration_order_within_an_energy():
    """the decision tree of GAAACGAAAC by hand: the exterior loop takes "9 unpaired" first, below it the open chain and the 5'
    hairpin; then the stems ending at 9, i ascending - (0,9), then (5,9) with the exterior loop of 0..4 pending.  Rows of one
    energy keep that order"""
    leaves = ["..........", "(...).....", "(........)", ".....(...)", "(...)(...)"]
    n_ties = 0
    for which in ("builtin", "tie0", "tie1"):
        mirror = MF.Mirror(table_set(which))
        got = SB.band(mirror, "GAAACGAAAC", 100000)
        assert sorted(r for r, _ in got) == sorted(leaves)
        assert [e for _, e in got] == sorted(e for _, e in got)
        for a, b in zip(got, got[1:]):
            if a[1] == b[1]:
                n_ties += 1
                assert leaves.index(a[0]) < leaves.index(b[0]), (which, got)
    assert n_ties >= 1


def test_subopt_records_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\}\s*rafft_subopt_seq;", hdr).group(1), flags=re.S)
    names = [n.strip(" *") for group in re.findall(r"\b(?:const )?(?:int32_t|int64_t|char)\s+([\w, *]+);", body) for n in group.split(",")]
    assert names == [n for n, _ in _native.SuboptSeq._fields_] == ["status", "length", "mfe_dcal", "n_structs", "n_reached", "db", "dcal"]
    assert ctypes.sizeof(_native.SuboptSeq) == 40 and ctypes.sizeof(_native.SuboptResult) == 24
    assert _native.SUBOPT_MAX_STRUCTS == 1 << 24 and _native.SUBOPT_MAX_DELTA == 1000000
    assert re.search(r"#define RAFFT_SUBOPT_MAX_STRUCTS \(1 << 24\)", hdr) and re.search(r"#define RAFFT_SUBOPT_MAX_DELTA\s+1000000", hdr)
    assert {"rafft_subopt_batch", "rafft_subopt_free"} <= set(_native.EXPORTS)
    proto = re.search(r"int\s+rafft_subopt_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_subopt_batch.argtypes) == 8


def test_bad_arguments_and_erroneous_sequences_need_no_device():
    from rafft_amd import wuchty
    L = _native.lib()
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    out = ctypes.POINTER(_native.SuboptResult)()
    ref = ctypes.byref(out)
    assert L.rafft_subopt_batch(-1, seq, ln, 37.0, 100, 10, 0, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, None, ln, 37.0, 100, 10, 0, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, None, 37.0, 100, 10, 0, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, ln, 37.0, 100, 10, 0, None) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, ln, 37.0, -1, 10, 0, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, ln, 37.0, _native.SUBOPT_MAX_DELTA + 1, 10, 0, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, ln, 37.0, 100, 0, 0, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, ln, 37.0, 100, _native.SUBOPT_MAX_STRUCTS + 1, 0, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, ln, 37.0, 100, 10, -1, ref) == _native.ERR_PARAM
    assert L.rafft_subopt_batch(1, seq, ln, 25.0, 100, 10, 0, ref) == _native.ERR_TEMP          # the built-in tables have no enthalpies
    assert not out
    L.rafft_subopt_free(None)
    # a batch of nothing but erroneous sequences never reaches the device
    recs, rows, dcal = wuchty.subopt_batch_raw(["", "GGGTAACCC", "A" * (_native.MFE_MAX_LEN + 1)], 100, 10)
    assert [r["status"] for r in recs] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG]
    assert [r["n_structs"] for r in recs] == [0, 0, 0] and [r["length"] for r in recs] == [0, 9, _native.MFE_MAX_LEN + 1]
    assert all(len(r) == 0 for r in rows) and all(len(d) == 0 for d in dcal)
    assert L.rafft_last_error().decode().startswith("sequence 0")
    assert wuchty.subopt_batch(["", "GGGXAACCC"], raise_errors=False) == [None, None]
    with pytest.raises(KeyError):
        wuchty.subopt("GGGTAACCC")
    with pytest.raises(ValueError, match="4096 nt"):
        wuchty.subopt("A" * (_native.MFE_MAX_LEN + 1))
    with pytest.raises(ValueError):
        wuchty.subopt_batch(["GGGAAACCC"], delta=-1.0)
