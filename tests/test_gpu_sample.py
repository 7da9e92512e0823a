"""rafft_sample_batch on a real MI355X (`-m gpu`): the counts of every structure and of every pair of short sequences against the
exact Boltzmann weights of the enumerated ensemble, the multiloop derivations at ten times the draws, pair counts against
rafft_pf_batch's probabilities where enumeration cannot reach, another temperature, same input - same bits, errors that stay with
their sequence, and the command line as a process.  Every statistical comparison is tests/_sample_stats.py's: about 1e-9 a
comparison for a correct sampler, and - rows being a function of the seed - a pass is a pass for good."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, mccaskill, params, rafft as R
from rafft_amd.utils import parse_rafft_output
from conftest import ROOT
import _loops as LP
import _mfe_np as MF
import _par_reader as PR
import _pf_np as PF
import _sample_stats as ST

pytestmark = pytest.mark.gpu

TABLES = ("builtin", "multiloops_win")
MULTILOOP_SEQS = ["GAGAAACGAAACGAAACC", "GAGAAACGAAACGAAACAC", "GAAGAAACGAAACGAAACC", "GUGAAACGAAACGAAACAU", "GAGAAACGAAACGAAACCA"]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    idx.update(ml_closing=-700, ml_intern=-300)               # negative enough that multiloops hold most of Z at 16-20 nt
    out = dict(builtin=builtin, multiloops_win=idx, synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name, comment in (("multiloops_win", "index-sensitive, multiloops win"), ("synthetic", "made-up enthalpies")):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=comment)
    return out


def install(sets, which):
    if which == "builtin":
        params.reset_params()
    else:
        params.load_params(sets["paths"][which])


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()


def rand(rng, n, letters="ACGU", p=None):
    return "".join(rng.choice(list(letters), n, p=p))


def exhaustive_sequences():
    """the list of tests/test_gpu_pf.py, restated"""
    rng = np.random.default_rng(1971)
    seqs = ["A", "GC", "GAC", "GAAC"]                                              # lengths 1-4: the open chain alone
    seqs += [rand(rng, n) for n in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20, 20, 20)]
    seqs += [rand(rng, n, "GCU") for n in (14, 16, 17)]
    for name in LP.KINDS:                                                          # GC hairpins around the special loops
        for sp in LP.OWN_SPECIAL[name]:
            seqs.append("GG" + sp + "CC")
    seqs += ["GGGACACCCAGGACCACCC", "G" * 10 + "U" * 10, "GU" * 9, "GGGUUUGGGUUUCCC", "GCGCAAAGCGCAAAGCGC", "GGGAAACCCAGGGAAACCCA", "NGGGAAACCCN"]
    return seqs + LP.N_SEQS + MULTILOOP_SEQS


_ENUM = {}


def enumerated(seqs):
    for s in seqs:
        if s not in _ENUM:
            _ENUM[s] = MF.enumerate_structures(s)
    return [_ENUM[s] for s in seqs]


def distinct(rows):
    """(texts, counts, index of the first sample of each) of an (n, L + 1) uint8 array of rows"""
    assert not rows[:, -1].any()                                                   # NUL terminated
    body = np.ascontiguousarray(rows[:, :-1])
    if body.shape[1] == 0:
        return [""], np.array([len(body)]), np.array([0]), np.zeros(len(body), dtype=np.int64)
    key = body.view(np.dtype((np.void, body.shape[1]))).ravel()
    u, first, inv, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    return [body[f].tobytes().decode("ascii") for f in first], counts, first, inv.ravel()


def pair_counts(texts, counts, L):
    out = np.zeros((L, L))
    for r, c in zip(texts, counts):
        for i, j in PF.pairs_of(r):
            out[i, j] += c
    return out


def check_against_enumeration(seqs, recs, rows, dcal, n, temp=37.0):
    """every row a member of the ensemble, dcal_out the evaluation of the row, every structure count and every pair count within the
    check's bound of the exact Boltzmann share; returns (structures compared, pairs compared, largest |X - Np| / allowed)"""
    kt = PF.kt_of(temp)
    ens = enumerated(seqs)
    en, st = R.eval_structures([s for s, rr in zip(seqs, ens) for _ in rr], [r for rr in ens for r in rr], temp=temp)     # one call
    assert not any(st)
    at, n_struct, n_pair, worst = 0, 0, 0, 0.0
    flat_s, flat_r, flat_d = [], [], []
    for k, (s, rr) in enumerate(zip(seqs, ens)):
        e = np.array(en[at:at + len(rr)])
        at += len(rr)
        assert recs[k]["status"] == 0 and recs[k]["n_samples"] == n and rows[k].shape == (n, len(s) + 1)
        Z, P = PF.exact(rr, list(e), kt)
        p = np.exp(-e / (100.0 * kt)) / Z
        texts, counts, first, inv = distinct(rows[k])
        where = {r: x for x, r in enumerate(rr)}
        assert all(t in where for t in texts), s                                   # a sample never leaves the ensemble
        assert np.array_equal(dcal[k], dcal[k][first][inv]), s                    # one row, one energy
        assert [int(dcal[k][f]) for f in first] == [int(e[where[t]]) for t in texts], s
        flat_s += [s] * len(texts); flat_r += texts; flat_d += [int(dcal[k][f]) for f in first]
        X = np.zeros(len(rr))
        X[[where[t] for t in texts]] = counts
        assert len(ST.misses(X, n, p)) == 0, (s, [(rr[x], X[x], n * p[x]) for x in ST.misses(X, n, p)][:5])
        XP = pair_counts(texts, counts, len(s))
        assert len(ST.misses(XP, n, P)) == 0, (s, ST.misses(XP, n, P)[:5])
        worst = max(worst, float((np.abs(X - n * p) / ST.allowed(n, p)).max()), float((np.abs(XP - n * P) / ST.allowed(n, P)).max()))
        n_struct += len(rr); n_pair += P.size
        assert min(e) == recs[k]["mfe_dcal"]
    got, st = R.eval_structures(flat_s, flat_r, temp=temp)                         # dcal_out against rafft_eval_structures, one call
    assert not any(st) and list(got) == flat_d
    return n_struct, n_pair, worst


# ---- 1. every structure, short sequences

@pytest.mark.parametrize("which", TABLES)
def test_gpu_sample_counts_equal_the_boltzmann_shares_of_every_structure(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    assert 44 <= len(seqs) <= 59 and max(map(len, seqs)) == 20 and sum("N" in s for s in seqs) == 5
    n = 20000
    recs, rows, dcal = mccaskill.sample_batch_raw(seqs, n, seeds=list(range(100, 100 + len(seqs))))
    n_struct, n_pair, worst = check_against_enumeration(seqs, recs, rows, dcal, n)
    print(f"\n{which}: {n_struct} structure counts and {n_pair} pair counts compared, the largest deviation is {worst:.3f} of what the check allows")
    pf = mccaskill.pf_batch_raw(seqs, probs=False)[1]
    assert [(np.float64(r["energy"]).tobytes(), r["mfe_dcal"]) for r in recs] == [(np.float64(r["energy"]).tobytes(), r["mfe_dcal"]) for r in pf]
    for k in range(4):                                                             # 1-4 nt: only the open chain
        assert rows[k].tobytes() == (b"." * len(seqs[k]) + b"\0") * n and not dcal[k].any()


# ---- 2. multiloop derivations, sharper

def test_gpu_sample_multiloop_derivations_at_200000_draws(sets):
    """under `multiloops_win` the multiloop with an unpaired base before its first stem holds most of Z: a grammar that derives it
    twice, or a wrong power of pb, moves shares of tens of per cent by far more than the 1349 draws the check allows at 30 %"""
    install(sets, "multiloops_win")
    n = 200000
    recs, rows, dcal = mccaskill.sample_batch_raw(MULTILOOP_SEQS, n, seeds=7)
    n_struct, n_pair, worst = check_against_enumeration(MULTILOOP_SEQS, recs, rows, dcal, n)
    print(f"\n{n_struct} structure counts and {n_pair} pair counts compared, the largest deviation is {worst:.3f} of what the check allows")
    lead = 0
    for s, r in zip(MULTILOOP_SEQS, rows):
        texts, counts, _, _ = distinct(r)
        lead += sum(c for t, c in zip(texts, counts) if PF.has_leading_unpaired_multiloop(t)) > 0.001 * n
    assert lead >= 3                                                               # the derivations in question are drawn


# ---- 3. beyond enumeration

def loops_ok(seq, db):
    """balanced, canonical pairs (N pairs with nothing), hairpins of at least 3, interior loops of at most 30"""
    pt = LP.pair_table(db)
    for i, j in enumerate(pt):
        if j > i:
            if (seq[i] + seq[j]) not in MF.PAIRS:
                return False
            kids, x = [], i + 1
            while x < j:
                if pt[x] > x:
                    kids.append((x, pt[x])); x = pt[x] + 1
                else:
                    x += 1
            if not kids and j - i - 1 < 3:
                return False
            if len(kids) == 1 and (kids[0][0] - i - 1) + (j - kids[0][1] - 1) > MF.MAXLOOP:
                return False
    return True


def check_against_pf(seqs, n, seed):
    recs, rows, dcal = mccaskill.sample_batch_raw(seqs, n, seeds=seed)
    pf_rows, pf_recs, probs = mccaskill.pf_batch_raw(seqs)
    flat_s, flat_r, flat_d = [], [], []
    for k, s in enumerate(seqs):
        L = len(s)
        assert recs[k]["status"] == 0 and recs[k]["n_samples"] == n
        assert np.float64(recs[k]["energy"]).tobytes() == np.float64(pf_recs[k]["energy"]).tobytes() and recs[k]["mfe_dcal"] == pf_recs[k]["mfe_dcal"]
        texts, counts, first, inv = distinct(rows[k])
        assert all(loops_ok(s, t) for t in texts), s
        assert np.array_equal(dcal[k], dcal[k][first][inv])
        flat_s += [s] * len(texts); flat_r += texts; flat_d += [int(dcal[k][f]) for f in first]
        XP = pair_counts(texts, counts, L)
        bad = ST.misses(XP, n, probs[k])
        assert len(bad) == 0, (s[:20], [(divmod(int(b), L), XP.ravel()[b], n * probs[k].ravel()[b]) for b in bad[:5]])
        assert dcal[k].min() >= recs[k]["mfe_dcal"]
        print(f"\n{L} nt: {len(texts)} distinct structures in {n} draws, lowest energy {dcal[k].min()} dcal/mol (MFE {recs[k]['mfe_dcal']})")
    got, st = R.eval_structures(flat_s, flat_r)
    assert not any(st) and list(got) == flat_d
    return rows


def test_gpu_sample_pair_counts_equal_the_probabilities_at_60_to_90_nt():
    rng = np.random.default_rng(78)
    seqs = [rand(rng, n) for n in (60, 75, 90)]
    for run in (30, 31):          # one good helix pair separated by an A-run on one side: 30 is an allowed bulge, 31 is not
        seqs.append("GGGCG" + "A" * run + "GCGCG" + "GAAA" + "CGCGC" + "CGCCC")
    rows = check_against_pf(seqs, 5000, 21)
    body = rows[3][:, :-1].tobytes().decode("ascii")
    L = len(seqs[3])
    n30 = sum(body[r * L:(r + 1) * L].startswith("(((((" + "." * 30 + "(((((") for r in range(5000))
    assert n30 > 0                                   # the bulge of 30 is drawn (how often: the pair counts above); one of 31 never, by loops_ok


def test_gpu_sample_holds_1500_nt():
    rng = np.random.default_rng(1500)
    check_against_pf([rand(rng, 1500, "ACGU", [0.1, 0.4, 0.4, 0.1])], 500, 3)


# ---- 4. another temperature

def test_gpu_sample_at_another_temperature(sets):
    install(sets, "synthetic")
    seqs = MULTILOOP_SEQS[:2] + ["GGGACACCCAGGACCACCC", "GCGCAAAGCGCAAAGCGC", "GGGAAACCCAGGGAAACCCA", "GU" * 9]
    n = 20000
    recs, rows, dcal = mccaskill.sample_batch_raw(seqs, n, seeds=9, temp=60.0)
    n_struct, n_pair, worst = check_against_enumeration(seqs, recs, rows, dcal, n, temp=60.0)
    print(f"\n60 C: {n_struct} structure counts and {n_pair} pair counts compared, the largest deviation is {worst:.3f} of what the check allows")
    pf = mccaskill.pf_batch_raw(seqs, temp=60.0, probs=False)[1]
    assert [np.float64(r["energy"]).tobytes() for r in recs] == [np.float64(r["energy"]).tobytes() for r in pf]


# ---- 5. same input, same bits

def bits(recs, rows, dcal, k):
    r = recs[k]
    return (r["status"], r["length"], r["mfe_dcal"], r["n_samples"], np.float64(r["energy"]).tobytes(), rows[k].tobytes(), dcal[k].tobytes())


def test_gpu_sample_same_input_same_bits():
    rng = np.random.default_rng(6)
    seqs = [rand(rng, n) for n in (33, 58, 71, 20, 64, 45, 80, 9)]
    seeds = [1000 + k for k in range(len(seqs))]
    n = 300
    whole = mccaskill.sample_batch_raw(seqs, n, seeds=seeds)
    want = {s: bits(*whole, k) for k, s in enumerate(seqs)}
    assert all(whole[0][k]["status"] == 0 for k in range(len(seqs)))
    for k in (0, 3, len(seqs) - 1):                                                # alone
        assert bits(*mccaskill.sample_batch_raw([seqs[k]], n, seeds=[seeds[k]]), 0) == want[seqs[k]]
    got = mccaskill.sample_batch_raw(seqs[::-1], n, seeds=seeds[::-1])             # reversed: every sequence at another position
    assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs[::-1]]
    got = mccaskill.sample_batch_raw(seqs, n, seeds=seeds, workspace_bytes=1)      # one sequence per chunk
    assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs]
    got = mccaskill.sample_batch_raw(seqs, n, seeds=seeds, workspace_bytes=n * 100)    # the rows decide the chunks
    assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs]
    more = mccaskill.sample_batch_raw(seqs, 2 * n + 1, seeds=seeds)                # the prefix property
    for k in range(len(seqs)):
        assert more[1][k][:n].tobytes() == whole[1][k].tobytes() and more[2][k][:n].tobytes() == whole[2][k].tobytes()
        assert len(seqs[k]) < 30 or more[1][k][n:2 * n].tobytes() != whole[1][k].tobytes()
    other = mccaskill.sample_batch_raw(seqs, n, seeds=[x + 1 for x in seeds])      # another seed, other rows
    assert all(other[1][k].tobytes() != whole[1][k].tobytes() for k in range(len(seqs)) if len(seqs[k]) > 30)
    twice = mccaskill.sample_batch_raw([seqs[1], seqs[1], seqs[1]], n, seeds=[5, 5, 6])    # equal sequences: equal seeds, equal rows
    assert twice[1][0].tobytes() == twice[1][1].tobytes() != twice[1][2].tobytes()
    zero = mccaskill.sample_batch_raw(seqs[:2], n)                                 # seeds NULL: all 0
    assert [bits(*zero, k) for k in range(2)] == [bits(*mccaskill.sample_batch_raw(seqs[:2], n, seeds=0), k) for k in range(2)]
    none = mccaskill.sample_batch_raw(seqs[:2], 0, seeds=seeds[:2])                # n_samples == 0: the records
    assert [(r["status"], r["n_samples"], r["mfe_dcal"], r["energy"]) for r in none[0]] == [(0, 0, r["mfe_dcal"], r["energy"]) for r in whole[0][:2]]


def test_gpu_sample_does_not_depend_on_the_scale_in_distribution():
    seqs = ["GGGACACCCAGGACCACCC", "GCGCAAAGCGCAAAGCGC", MULTILOOP_SEQS[0]]
    n = 20000
    for sf in (0.5, 1.07, 1.5):
        recs, rows, dcal = mccaskill.sample_batch_raw(seqs, n, seeds=31, scale_factor=sf)
        check_against_enumeration(seqs, recs, rows, dcal, n)


# ---- 6. errors stay with their sequence

def test_gpu_sample_errors_stay_with_their_sequence():
    rng = np.random.default_rng(404)
    good = ["GGGGAAAACCCC", rand(rng, 40), "GCGCUUCGGCGC", rand(rng, 25), "ACGUACGUACGUACGUAGC"]
    big = "G" * 200 + "GAAA" + "C" * 200
    seqs = [good[0], "", good[1], "GGGXAAACCC", good[2], "A" * (N.PF_MAX_LEN + 1), good[3], big, good[4]]
    at = [0, 2, 4, 6, 8]
    seeds = list(range(50, 50 + len(seqs)))
    n = 40
    for sf in (1e-9, 0.0):
        alone = mccaskill.sample_batch_raw(good, n, seeds=[seeds[k] for k in at], scale_factor=sf)
        recs, rows, dcal = mccaskill.sample_batch_raw(seqs, n, seeds=seeds, scale_factor=sf)      # returns: the call is RAFFT_OK
        want_big = N.ERR_CAPACITY if sf else N.OK
        assert [r["status"] for r in recs] == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, 0, N.ERR_TOO_LONG, 0, want_big, 0]
        assert N.lib().rafft_last_error().decode().startswith("sequence 1")
        for k in (1, 3, 5) + ((7,) if sf else ()):
            assert recs[k]["n_samples"] == 0 and recs[k]["energy"] == 0.0 and not dcal[k].any()
            assert rows[k].tobytes() == (b"." * len(seqs[k]) + b"\0") * n
        assert [bits(recs, rows, dcal, k) for k in at] == [bits(*alone, k) for k in range(len(good))]
        if sf:
            only = mccaskill.sample_batch_raw([big], n, scale_factor=sf)
            assert only[0][0]["status"] == N.ERR_CAPACITY and N.lib().rafft_last_error().decode().startswith("sequence 0:")
            assert only[0][0]["mfe_dcal"] < -60000
        else:
            assert recs[7]["n_samples"] == n and dcal[7].min() >= recs[7]["mfe_dcal"] and math.isfinite(recs[7]["energy"])
            texts, counts, first, inv = distinct(rows[7])
            got, st = R.eval_structures([big] * len(texts), texts)
            assert not any(st) and list(got) == [int(dcal[7][f]) for f in first] and all(t.count("(") > 150 for t in texts)
    got = rafft_amd.sample_batch(seqs, 3, seeds=seeds, raise_errors=False)
    assert [g is None for g in got] == [False, True, False, True, False, True, False, False, False]
    assert [st.str_struct for st in got[0]] == [rows[0][r, :-1].tobytes().decode() for r in range(3)] and [st.dcal for st in got[0]] == list(dcal[0][:3])
    assert [st.str_struct for st in rafft_amd.sample(good[0], 3, seed=seeds[0])] == [st.str_struct for st in got[0]]
    # RAFFT_ERR_PARAM: the outputs are not touched, and the next call is exact
    L = N.lib()
    buf = ctypes.create_string_buffer(b"untouched!", 16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (N.SampleSeq * 1)()
    rec[0].status = 77
    seq = (ctypes.c_char_p * 1)(good[0].encode())
    ln = (ctypes.c_int * 1)(12)
    for args in ((1, seq, ln, 37.0, 0.0, 0, 1, None, None, out, None), (1, seq, ln, 37.0, 0.0, 0, 1, None, rec, None, None),
                 (1, seq, ln, 37.0, 0.0, 0, -1, None, rec, out, None), (1, seq, ln, 37.0, float("nan"), 0, 1, None, rec, out, None),
                 (1, seq, ln, 37.0, 0.0, 0, N.SAMPLE_MAX + 1, None, rec, out, None)):
        assert L.rafft_sample_batch(*args) == N.ERR_PARAM
        assert buf.value == b"untouched!" and rec[0].status == 77
    assert bits(*mccaskill.sample_batch_raw(good[:1], n, seeds=seeds[:1]), 0) == bits(*alone, 0)
    with pytest.raises(N.RafftError) as e:                                         # the built-in tables are 37 C only
        mccaskill.sample_batch_raw(good, 2, temp=25.0)
    assert e.value.code == N.ERR_TEMP


# ---- 7. the command line as a process

def test_gpu_cli_sample_writes_one_step_of_distinct_rows(tmp_path):
    seq = "GGGAAACCCAGGGAAACCCAGCGCAAAGCGC"
    f = tmp_path / "f"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-s", seq, "--sample", "200", "--seed", "3", "-o", str(f)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, got_seq = parse_rafft_output(str(f))
    assert got_seq == seq and len(steps) == 1
    texts = [st.str_struct for st in steps[0]]
    assert 1 < len(texts) == len(set(texts)) <= 200
    assert [(st.energy, st.str_struct) for st in steps[0]] == sorted((st.energy, st.str_struct) for st in steps[0])
    want = rafft_amd.sample(seq, 200, seed=3)
    assert set(texts) == {st.str_struct for st in want}
