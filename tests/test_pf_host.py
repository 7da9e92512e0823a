"""The host side of the partition function (rafft_pf_batch, rafft_amd.pf_batch, `rafft --pf`) and the tests' own mirror of its
recurrences: the mirror's Z and every P(i,j) equal the sums over every structure of a short sequence under the oracle's energies,
the MFE's ambiguous M fed to the same check misses (so the check sees that trap), the record's layout, the option surface, and the
errors that need no device.  No GPU."""
import ctypes
import math
import os
import re

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

# closing pair, an unpaired base (two in the third), three GAAAC hairpins: under ml_closing = -700, ml_intern = -300 the multiloop
# with the unpaired base before its first stem holds nearly all of Z, and two stems follow that base - what the ambiguous M counts twice
MULTILOOP_SEQS = ["GAGAAACGAAACGAAACC", "GAGAAACGAAACGAAACAC", "GAAGAAACGAAACGAAACC", "GUGAAACGAAACGAAACAU", "GAGAAACGAAACGAAACCA"]


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


def short_sequences():
    rng = np.random.default_rng(1971)
    seqs = ["A", "GC", "GAC", "GAAC"]                                                       # lengths 1-4: one structure
    seqs += ["".join(rng.choice(list("ACGU"), n)) for n in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20)]
    seqs += ["".join(rng.choice(list("GC"), n)) for n in (9, 12, 14)]
    seqs += ["GGGGAAAACCCC", "GACAC", "GGACACC", "GUGUGUGUGUGUGU", "GGGUUUGGGUUUCCC", "NGGGAAACCCN", "GCGCAAAGCGCAAAGC", "GGGAAACCCAGGGAAACCCA"]
    return seqs + LP.N_SEQS + MULTILOOP_SEQS


def table_set(which):
    par = LP.builtin_par()
    if which != "builtin":
        par = LP.index_sensitive_par(par)
        par.update(ml_closing=-700, ml_intern=-300)
        oracle.set_tables(PR.tables_at(par, 37.0))
    return PR.tables_at(par, 37.0)


@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_mirror_equals_the_sums_over_every_structure(which):
    tabs = table_set(which)
    mirror, ambiguous = PF.PfMirror(tabs), PF.PfMirror(tabs, ambiguous=True)
    kt = PF.kt_of(37.0)
    worst_z = worst_p = 0.0
    n_leading = n_missed = 0
    for s in short_sequences():
        rows = MF.enumerate_structures(s)
        en = [oracle.eval_structure(s, r) for r in rows]
        Z, P = PF.exact(rows, en, kt)
        Zm, Pm = mirror.run(s)
        worst_z, worst_p = max(worst_z, abs(Zm / Z - 1.0)), max(worst_p, float(np.abs(Pm - P).max()))
        assert abs(Zm / Z - 1.0) <= 1e-10, (which, s)
        assert np.abs(Pm - P).max() <= 1e-10, (which, s)
        if len(s) <= 4:
            assert Z == 1.0 and not P.any()
        lead = math.fsum(math.exp(-e / (100.0 * kt)) for r, e in zip(rows, en) if PF.has_leading_unpaired_multiloop(r)) / Z
        n_leading += lead > 1e-3
        n_missed += abs(ambiguous.inside(s) / Z - 1.0) > 1e-6
    print(f"\n{which}: largest relative error of Z {worst_z:.3g}, largest error of P {worst_p:.3g}; {n_leading} sequences with a leading unpaired base "
          f"in a multiloop above 1e-3 of Z, the ambiguous M misses {n_missed}")
    if which == "multiloops_win":
        # the condition under which an ambiguous M cannot pass unnoticed - and it does not
        assert n_leading >= 3
        assert n_missed >= 3


def test_ambiguous_m_misses_on_each_multiloop_sequence():
    tabs = table_set("multiloops_win")
    mirror, ambiguous = PF.PfMirror(tabs), PF.PfMirror(tabs, ambiguous=True)
    for s in MULTILOOP_SEQS:
        z = mirror.inside(s)
        assert abs(ambiguous.inside(s) / z - 1.0) > 1e-6, s


def test_exact_helper_and_multiloop_detector():
    kt = PF.kt_of(37.0)
    Z, P = PF.exact([".....", "(...)"], [0, -100], kt)
    w = math.exp(1.0 / kt)
    assert Z == 1.0 + w and P[0, 4] == w / (1.0 + w) and P.sum() == P[0, 4]
    assert PF.has_leading_unpaired_multiloop("(.(...)(...))") and PF.has_leading_unpaired_multiloop("..((.(...)(...)..))")
    assert not PF.has_leading_unpaired_multiloop("((...)(...).)") and not PF.has_leading_unpaired_multiloop("(.(...).)") and not PF.has_leading_unpaired_multiloop(".(...).(...)")


def test_pf_record_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*rafft_pf_seq;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for _, group in re.findall(r"\b(int32_t|double)\s+([\w, ]+);", body) for n in group.split(",")]
    assert names == [n for n, _ in _native.PfSeq._fields_] == ["status", "length", "mfe_dcal", "n_pairs", "energy", "mfe_frequency"]
    assert ctypes.sizeof(_native.PfSeq) == 32
    assert "#define RAFFT_PF_MAX_LEN RAFFT_MFE_MAX_LEN" in hdr and _native.PF_MAX_LEN == _native.MFE_MAX_LEN
    assert "rafft_pf_batch" in _native.EXPORTS
    proto = re.search(r"int rafft_pf_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_pf_batch.argtypes) == 9
    assert "vrna_mfe.py:25" in hdr and "RNA.fold_compound(seq, md).pf()" in hdr and "bpp()" in hdr and "P > 0.5" in hdr
    assert rafft_amd.pf is not None and rafft_amd.pf_batch is not None


def test_bad_arguments_need_no_device():
    L = _native.lib()
    buf = ctypes.create_string_buffer(b"untouched!", 16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.PfSeq * 1)()
    rec[0].status, rec[0].energy = 77, 7.5
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    for args in ((-1, seq, ln, 37.0, 0.0, 0, rec, out, None), (1, None, ln, 37.0, 0.0, 0, rec, out, None), (1, seq, None, 37.0, 0.0, 0, rec, out, None),
                 (1, seq, ln, 37.0, 0.0, 0, None, out, None), (1, seq, ln, 37.0, 0.0, 0, rec, None, None), (1, seq, ln, 37.0, -1.0, 0, rec, out, None),
                 (1, seq, ln, 37.0, float("nan"), 0, rec, out, None), (1, seq, ln, 37.0, float("inf"), 0, rec, out, None),
                 (1, seq, ln, 37.0, 0.0, -1, rec, out, None)):
        assert L.rafft_pf_batch(*args) == _native.ERR_PARAM, args
        assert buf.value == b"untouched!" and rec[0].status == 77 and rec[0].energy == 7.5
    assert L.rafft_pf_batch(0, None, None, 37.0, 0.0, 0, None, None, None) == _native.OK


def test_errors_of_a_sequence_without_a_device():
    from rafft_amd import mccaskill as M
    rows, recs, probs = M.pf_batch_raw(["", "GGGTAACCC", "gggaaaccc", "A" * (_native.PF_MAX_LEN + 1)])
    assert [r["status"] for r in recs] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG]
    assert rows == ["", "." * 9, "." * 9, "." * (_native.PF_MAX_LEN + 1)]
    assert all(r["energy"] == 0.0 and r["mfe_frequency"] == 0.0 and r["n_pairs"] == 0 and r["mfe_dcal"] == 0 for r in recs)
    assert probs[3] is None and not probs[1].any() and probs[1].shape == (9, 9)
    assert _native.lib().rafft_last_error().decode().startswith("sequence 0")
    with pytest.raises(np.exceptions.AxisError):
        rafft_amd.pf("")
    with pytest.raises(KeyError):
        rafft_amd.pf("GGGTAACCC")
    with pytest.raises(ValueError, match="4096 nt"):
        rafft_amd.pf("A" * (_native.PF_MAX_LEN + 1))
    with pytest.raises(_native.RafftError) as e:             # the temperature is checked first, as the fold checks it
        M.pf_batch_raw(["", "GGGXAACCC"], temp=25.0)
    assert e.value.code == _native.ERR_TEMP
    assert rafft_amd.pf_batch(["", "GGGXAACCC"], raise_errors=False) == [None, None]


def test_cli_parses_pf():
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--pf", "-o", "out.txt"])
    assert a.pf and a.batch and not a.mfe and a.output == "out.txt"
    assert cli.parse_arguments(["-s", "GGGAAACCC", "--pf"]).pf
    assert not cli.parse_arguments(["-s", "GGGAAACCC"]).pf


def test_cli_pf_lines_scores_and_exclusions(tmp_path, capsys):
    from rafft_amd.mccaskill import PfResult
    calls = []

    def stub(seqs, temp):
        calls.append((list(seqs), temp))
        return [PfResult(-3.456, "(((...)))", 0.87654321, -3.07) if len(s) == 9 else PfResult(0.0, "." * len(s), 1.0, 0.0) for s in seqs]

    cli.main(["-s", "GGGAAACCC", "--pf"], pf_batch=stub)
    assert capsys.readouterr().out == "GGGAAACCC 9 (((...))) -3.46 3 0.8765\n"
    fa = tmp_path / "s.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nAAAA\n")
    out = tmp_path / "o.txt"
    cli.main(["-sf", str(fa), "--batch", "--pf", "-o", str(out)], pf_batch=stub)
    assert out.read_text().splitlines() == ["GGGAAACCC 9 (((...))) -3.46 3 0.8765", "AAAA 4 .... 0.00 0 1"]
    assert calls[-1] == (["GGGAAACCC", "AAAA"], 37.0)
    csvf = tmp_path / "k.csv"
    csvf.write_text("GGGAAACCC,((.....)),x1\nAAAA,....,x2\n")
    seen = {}

    def scorer(beams, known):
        seen["beams"], seen["known"] = [[st.str_struct for st in b] for b in beams], list(known)
        z = np.zeros(2, dtype=np.int32)
        return dict(pick_ppv=z, pick_first=z, row0=np.array([0, 1]), n_known=np.array([2, 0]), seq_status=z, n_pred=np.array([3, 0]),
                    hit_pred=np.array([2, 0]), hit_known=np.array([2, 0]))

    sc = tmp_path / "scores.csv"
    cli.main(["-sf", str(csvf), "--batch", "--pf", "--scores", str(sc)], pf_batch=stub, scorer=scorer)
    assert seen == {"beams": [["(((...)))"], ["...."]], "known": ["((.....))", "...."]}
    assert sc.read_text().splitlines() == ["seq,len_seq,struct,nrj,nbp,pvv,sens,name", "GGGAAACCC,9,(((...))),-3.456,3,66.67,100.0,x1", "AAAA,4,....,0.0,0,0.0,0.0,x2"]
    for extra in (["--mfe"], ["--traj"], ["--kin", str(tmp_path / "kin.txt")]):
        with pytest.raises(SystemExit):
            cli.main(["-sf", str(fa), "--batch", "--pf"] + extra, pf_batch=stub)
