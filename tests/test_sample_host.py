"""The host side of sampling from the ensemble (rafft_sample_batch, rafft_amd.sample_batch, `rafft --sample`): the statistical check
on draws that are right and on draws that are not, the Philox generator of rafft_rng.h against a restatement in Python integers, the
record's layout, the errors that need no device, and the command line through its injection point.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rafft_amd
from rafft_amd import _native, cli, params
from rafft_amd.utils import Structure, parse_rafft_output
from conftest import ROOT
import _mfe_np as MF
import _pf_np as PF
import _sample_stats as ST


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()
    params.reset_params()


# ---- 1. the check sees a wrong sampler and lets a right one pass

def test_check_passes_exact_draws_and_fails_draws_at_another_kt():
    """an enumerated ensemble under the oracle's energies; numpy draws structures with the exact Boltzmann weights (passes) and with
    the weights of 1.05 kT (fails): structure counts and pair counts, as the GPU tests use the check"""
    seq = "GGGACACCCAGGACCACCC"
    rows = MF.enumerate_structures(seq)
    en = np.array([oracle.eval_structure(seq, r) for r in rows])
    kt = PF.kt_of(37.0)
    Z, P = PF.exact(rows, list(en), kt)
    p = np.exp(-en / (100.0 * kt)) / Z
    member = np.zeros((len(rows), len(seq), len(seq)))
    for x, r in enumerate(rows):
        for i, j in PF.pairs_of(r):
            member[x, i, j] = 1.0
    n = 200000
    rng = np.random.default_rng(11)
    for factor, ok in ((1.0, True), (1.05, False)):
        q = np.exp(-en / (100.0 * kt * factor))
        counts = np.bincount(rng.choice(len(rows), n, p=q / q.sum()), minlength=len(rows))
        bad_s = ST.misses(counts, n, p)
        bad_p = ST.misses(np.tensordot(counts, member, 1), n, P)
        print(f"\nkT x {factor}: {len(bad_s)} of {len(rows)} structure counts and {len(bad_p)} of {P.size} pair counts miss")
        assert (len(bad_s) == 0 and len(bad_p) == 0) == ok
        if not ok:
            assert len(bad_s) and len(bad_p)
    assert list(ST.misses([0, 1], 100, [0.0, 0.0])) == [1]                         # p == 0 must give X == 0
    # what the check resolves at the 200000 draws of the sharper GPU test: a structure that holds 30 % of the ensemble and is drawn
    # with 32 % instead does not pass (4000 draws too many, 1349 allowed); a bias of 2 % OF its 30 % (1200 draws) needs 260000 draws
    assert 0.02 * 200000 > ST.allowed(200000, 0.3) > 0.02 * 0.3 * 200000
    assert 0.02 * 0.3 * 260000 > ST.allowed(260000, 0.3)


# ---- 2. Philox4x32-10

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85                     # the published constants
MASK = 0xFFFFFFFF


def philox(key, ctr):
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


@pytest.fixture(scope="module")
def rng_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostcheck") / "rng_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "hostcheck", "rng_check.cpp"), "-o", exe])
    return exe


def test_philox_equals_its_restatement(rng_check):
    # the known answers of the generator's authors (Random123, kat_vectors): the restatement itself is right
    assert philox((0, 0), (0, 0, 0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox((MASK, MASK), (MASK,) * 4) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    rng = np.random.default_rng(5)
    cases = [(0, 0, 0), ((1 << 64) - 1, MASK, MASK), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1 << 32, 0, 0)]
    cases += [(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 14))) for _ in range(300)]
    cases += [(77, k, t) for k in range(12) for t in range(12)]
    text = "".join(f"{key} {k} {t}\n" for key, k, t in cases) + "raw 0 0 0 0 0 0\n" + f"raw {MASK} {MASK} {MASK} {MASK} {MASK} {MASK}\n"
    r = subprocess.run([rng_check], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases) + 2
    blocks = set()
    for (key, k, t), line in zip(cases, lines):
        f = line.split()
        want = philox((key & MASK, key >> 32), (k, t, 0, 0))
        assert tuple(int(x, 16) for x in f[:4]) == want, (key, k, t)
        bits = int(f[4])
        assert bits == (want[0] << 32 | want[1]) >> 11 and 0 <= bits < 1 << 53      # the uniform is bits * 2^-53: in [0, 1)
        blocks.add((key, want))
    assert len(blocks) == len(set(cases))                                           # distinct (k, t): distinct blocks
    assert [tuple(int(x, 16) for x in l.split()) for l in lines[-2:]] == [philox((0, 0), (0, 0, 0, 0)), philox((MASK, MASK), (MASK,) * 4)]


# ---- 3. header, binding, arguments

def test_sample_record_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*rafft_sample_seq;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for _, group in re.findall(r"\b(int32_t|double)\s+([\w, ]+);", body) for n in group.split(",")]
    assert names == [n for n, _ in _native.SampleSeq._fields_] == ["status", "length", "mfe_dcal", "n_samples", "energy"]
    assert ctypes.sizeof(_native.SampleSeq) == 24
    assert "#define RAFFT_SAMPLE_MAX (1 << 20)" in hdr and _native.SAMPLE_MAX == 1 << 20
    assert "rafft_sample_batch" in _native.EXPORTS
    proto = re.search(r"int rafft_sample_batch\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_sample_batch.argtypes) == 11
    assert "Two equal sequences with equal seeds get equal rows" in hdr
    assert rafft_amd.sample is not None and rafft_amd.sample_batch is not None


def test_bad_arguments_need_no_device():
    L = _native.lib()
    buf = ctypes.create_string_buffer(b"untouched!", 16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (_native.SampleSeq * 1)()
    rec[0].status, rec[0].energy = 77, 7.5
    seq = (ctypes.c_char_p * 1)(b"GGGAAACCC")
    ln = (ctypes.c_int * 1)(9)
    a = dict(n_seq=1, seqs=seq, lens=ln, temp=37.0, sf=0.0, ws=0, n=1, seeds=None, rec=rec, out=out, dcal=None)
    for change in (dict(rec=None), dict(out=None), dict(n_seq=-1), dict(n=-1), dict(sf=-1.0), dict(sf=float("nan")), dict(sf=float("inf")),
                   dict(n=_native.SAMPLE_MAX + 1), dict(seqs=None), dict(lens=None), dict(ws=-1), dict(n_seq=0, rec=None)):
        args = list({**a, **change}.values())
        assert L.rafft_sample_batch(*args) == _native.ERR_PARAM, change
        assert buf.value == b"untouched!" and rec[0].status == 77 and rec[0].energy == 7.5
    assert L.rafft_sample_batch(0, None, None, 37.0, 0.0, 0, 5, None, rec, out, None) == _native.OK
    assert L.rafft_sample_batch(0, None, None, 37.0, 0.0, 0, 0, None, rec, None, None) == _native.OK      # n_samples == 0: no rows wanted


def test_errors_of_a_sequence_without_a_device():
    from rafft_amd import mccaskill as M
    seqs = ["", "GGGTAACCC", "A" * (_native.PF_MAX_LEN + 1)]
    recs, rows, dcal = M.sample_batch_raw(seqs, 3, seeds=5)
    assert [r["status"] for r in recs] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR, _native.ERR_TOO_LONG]
    assert all(r["n_samples"] == 0 and r["energy"] == 0.0 and r["mfe_dcal"] == 0 for r in recs)
    assert [r.shape for r in rows] == [(3, 1), (3, 10), (3, _native.PF_MAX_LEN + 2)]
    assert rows[1].tobytes() == (b"." * 9 + b"\0") * 3 and not rows[0].any() and not any(d.any() for d in dcal)
    assert _native.lib().rafft_last_error().decode().startswith("sequence 0")
    recs, rows, dcal = M.sample_batch_raw(seqs[:2], 0)                                 # n_samples == 0: records only
    assert [r["status"] for r in recs] == [_native.ERR_EMPTY, _native.ERR_BAD_CHAR] and rows[1].shape == (0, 10)
    assert rafft_amd.sample_batch(seqs[:2], 2, raise_errors=False) == [None, None]
    with pytest.raises(KeyError):
        rafft_amd.sample("GGGTAACCC", 2)
    with pytest.raises(ValueError, match="4096 nt"):
        rafft_amd.sample(seqs[2], 1)
    with pytest.raises(_native.RafftError) as e:
        M.sample_batch_raw(["GGGXAACCC"], 2, temp=25.0)                             # the temperature is checked first
    assert e.value.code == _native.ERR_TEMP
    with pytest.raises(_native.RafftError) as e:
        M.sample_batch_raw(["GGGAAACCC"], _native.SAMPLE_MAX + 1)
    assert e.value.code == _native.ERR_PARAM
    with pytest.raises(ValueError):
        M.sample_batch_raw(["GGGAAACCC"], 2, seeds=[1, 2])
    with pytest.raises(ValueError):
        M.sample_batch_raw(["GGGAAACCC"], 2, seeds=-1)


# ---- 4. the command line

def _stub(calls):
    def stub(seqs, n, seed, temp):
        calls.append((list(seqs), n, seed, temp))
        out = []
        for s in seqs:
            L = len(s)
            a, b, c = "(" + "." * (L - 2) + ")", "." * L, ".(" + "." * (L - 4) + ")."
            picks = [(b, 0), (a, -120), (c, -120), (a, -120), (b, 0), (a, -120)]
            out.append([Structure(r, d) for r, d in picks][:n])
        return out
    return stub


def test_cli_sample_graph_text_scores_and_exclusions(tmp_path, capsys):
    calls = []
    stub = _stub(calls)
    a = cli.parse_arguments(["-s", "GGGAAACCC", "--sample", "6", "--seed", "3"])
    assert a.sample == 6 and a.seed == 3 and cli.parse_arguments(["-s", "GGGAAACCC"]).sample is None
    cli.main(["-s", "GGGAAACCC", "--sample", "6", "--seed", "3"], sample_batch=stub)
    text = capsys.readouterr().out
    assert calls[-1] == (["GGGAAACCC"], 6, 3, 37.0)
    # one step 0: the distinct structures, energy ascending, ties by row text
    assert text.splitlines() == ["GGGAAACCC", "# " + "{:-^20}".format(0), "(.......)   -1.2", ".(.....).   -1.2", ".........    0.0"]
    out = tmp_path / "one.txt"
    cli.main(["-s", "GGGAAACCC", "--sample", "6", "-o", str(out)], sample_batch=stub)
    assert out.read_text() == text and calls[-1][2] == 0
    steps, seq = parse_rafft_output(str(out))
    assert seq == "GGGAAACCC" and len(steps) == 1
    assert [(st.str_struct, st.dcal) for st in steps[0]] == [("(.......)", -120), (".(.....).", -120), (".........", 0)]
    fa = tmp_path / "s.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nACGUACGU\n")
    out2 = tmp_path / "two.txt"
    cli.main(["-sf", str(fa), "--batch", "--sample", "2", "-o", str(out2)], sample_batch=stub)
    assert out2.read_text().splitlines() == ["GGGAAACCC", "# " + "{:-^20}".format(0), "(.......)   -1.2", ".........    0.0",
                                             "ACGUACGU", "# " + "{:-^20}".format(0), "(......)   -1.2", "........    0.0"]
    csvf = tmp_path / "k.csv"
    csvf.write_text("GGGAAACCC,((.....)),x1\nACGUACGU,........,x2\n")
    seen = {}

    def scorer(beams, known):
        seen["beams"], seen["known"] = [[st.str_struct for st in b] for b in beams], list(known)
        z = np.zeros(2, dtype=np.int32)
        return dict(pick_ppv=np.array([1, 0]), pick_first=z, row0=np.array([0, 3]), n_known=np.array([2, 0]), seq_status=z,
                    n_pred=np.array([0, 1, 1, 0, 1, 1]), hit_pred=np.array([0, 1, 1, 0, 0, 0]), hit_known=np.array([0, 1, 1, 0, 0, 0]))

    sc = tmp_path / "scores.csv"
    cli.main(["-sf", str(csvf), "--batch", "--sample", "3", "--scores", str(sc)], sample_batch=stub, scorer=scorer)
    assert seen == {"beams": [[".........", "(.......)", ".(.....)."], ["........", "(......)", ".(....)."]], "known": ["((.....))", "........"]}
    assert sc.read_text().splitlines() == ["seq,len_seq,struct,nrj,nbp,pvv,sens,name", "GGGAAACCC,9,(.......),-1.2000000476837158,1,100.0,50.0,x1",
                                           "ACGUACGU,8,........,0.0,0,0.0,0.0,x2"]
    for extra in (["--mfe"], ["--pf"], ["--traj"], ["--kin", str(tmp_path / "kin.txt")]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-sf", str(fa), "--batch", "--sample", "2"] + extra, sample_batch=stub)
        assert str(e.value) == "--sample gives structures drawn from the ensemble of every sequence: no --mfe, no --pf, no --kin, no --traj"
    with pytest.raises(SystemExit, match="positive number"):
        cli.main(["-s", "GGGAAACCC", "--sample", "0"], sample_batch=stub)
    with pytest.raises(SystemExit, match="--scores needs -sf CSV --batch"):
        cli.main(["-s", "GGGAAACCC", "--sample", "2", "--scores", str(sc)], sample_batch=stub)
