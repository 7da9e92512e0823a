"""rafft_subopt_batch on a real MI355X (`-m gpu`): rows, energies and order equal the tests' own walk of the decision tree
(`_subopt_np.band`, which tests/test_subopt_host.py holds against the enumeration of every structure) on short sequences under four
table sets and at 60-90 nt, every row evaluates back to its energy, a 200-nt and a 1500-nt sequence side by side, Boltzmann samples
that fall into the band are members of it, same input - same bits across batch position, order, chunking and max_structs, capacity
and errors that stay with their sequence, other temperatures, and the command line as a process.  Integers and bytes: no tolerance."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, mccaskill, params, rafft as R, wuchty, zuker
from rafft_amd.utils import parse_rafft_output
from conftest import ROOT
import _loops as LP
import _mfe_np as MF
import _par_reader as PR
import _subopt_np as SB

pytestmark = pytest.mark.gpu

MULTILOOP_SEQS = ["GAGAAACGAAACGAAACC", "GAGAAACGAAACGAAACAC", "GAAGAAACGAAACGAAACC", "GUGAAACGAAACGAAACAU", "GAGAAACGAAACGAAACCA"]
DELTAS = (0, 150, 500, 100000)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    idx.update(ml_closing=-700, ml_intern=-300)
    out = dict(builtin=builtin, multiloops_win=idx, tie0=LP.tie_par(builtin, LP.TIE_ML[0]), tie1=LP.tie_par(builtin, LP.TIE_ML[1]),
               synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name, comment in (("multiloops_win", "index-sensitive, multiloops win"), ("tie0", "flat, multiloops cost nothing"),
                          ("tie1", "flat, multiloops win"), ("synthetic", "made-up enthalpies")):
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


def mirror_sequences():
    """the 60-90-nt list of tests/test_gpu_mfe.py, with the bulge of 30 that is allowed and the one of 31 that is not"""
    rng = np.random.default_rng(77)
    seqs = [rand(rng, n) for n in (60, 67, 75, 83, 90)]
    seqs.append(rand(rng, 64, "GC"))
    for run in (30, 31):
        seqs.append("GGGCG" + "A" * run + "GCGCG" + "GAAA" + "CGCGC" + "CGCCC")
    return seqs


def pairs_of(rows, dcal, k):
    return [(rows[k][r, :-1].tobytes().decode("ascii"), int(dcal[k][r])) for r in range(len(dcal[k]))]


def bits(recs, rows, dcal, k):
    r = recs[k]
    return (r["status"], r["length"], r["mfe_dcal"], r["n_structs"], r["n_reached"], rows[k].tobytes(), dcal[k].tobytes())


def evaluate_back(seqs, rows, dcal, temp=37.0):
    """every row's own energy (eval_kernel, one call) is the reported one"""
    flat_s, flat_r, want = [], [], []
    for k, s in enumerate(seqs):
        for text, e in pairs_of(rows, dcal, k):
            flat_s.append(s)
            flat_r.append(text)
            want.append(e)
    got, st = R.eval_structures(flat_s, flat_r, temp=temp)
    assert not any(st) and list(got) == want
    return len(want)


_BAND = {}


def mirror_band(sets, which, seqs, delta, temp=37.0):
    """band(...) of every sequence, computed once per (tables, temperature, sequence, delta)"""
    key = (which, temp)
    if key not in _BAND:
        _BAND[key] = (MF.Mirror(PR.tables_at(sets[which], temp)), {})
    mirror, done = _BAND[key]
    for s in seqs:
        if (s, delta) not in done:
            done[(s, delta)] = SB.band(mirror, s, delta)
    return [done[(s, delta)] for s in seqs]


# ---- 1. the symbol

def test_gpu_subopt_symbol_and_result():
    assert N.lib().rafft_subopt_batch is not None and N.lib().rafft_subopt_free is not None
    recs, rows, dcal = wuchty.subopt_batch_raw(["GGGGAAAACCCC", "GAAC"], 0)
    assert [r["status"] for r in recs] == [0, 0] and [r["n_structs"] for r in recs] == [1, 1]
    mfe = zuker.mfe_batch_raw(["GGGGAAAACCCC"])
    assert pairs_of(rows, dcal, 0) == [(mfe[0][0], mfe[1][0])] == [("((((....))))", recs[0]["mfe_dcal"])]
    assert pairs_of(rows, dcal, 1) == [("....", 0)]
    got = rafft_amd.subopt("GGGGAAAACCCC", delta=3.0)
    assert got[0].str_struct == "((((....))))" and len(got) > 1 and [st.dcal for st in got] == sorted(st.dcal for st in got)
    assert all(st.dcal <= got[0].dcal + 300 for st in got)


# ---- 2. every structure of short sequences

@pytest.mark.parametrize("which", ["builtin", "multiloops_win", "tie0", "tie1"])
def test_gpu_subopt_equals_the_walk_on_every_short_sequence(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    assert max(map(len, seqs)) == 20 and set(MULTILOOP_SEQS) <= set(seqs)
    n_rows = n_tied = 0
    for delta in DELTAS:
        recs, rows, dcal = wuchty.subopt_batch_raw(seqs, delta, max_structs=60000)
        assert not any(r["status"] for r in recs)
        want = mirror_band(sets, which, seqs, delta)
        for k, s in enumerate(seqs):
            got = pairs_of(rows, dcal, k)
            assert got == want[k], (which, s, delta)                               # rows, energies and order
            assert recs[k]["mfe_dcal"] == got[0][1] and recs[k]["n_structs"] == len(got)
            n_tied += sum(a[1] == b[1] for a, b in zip(got, got[1:]))
        n_rows += evaluate_back(seqs, rows, dcal)
        if delta == DELTAS[-1]:
            for k, s in enumerate(seqs):
                assert sorted(t for t, _ in pairs_of(rows, dcal, k)) == sorted(MF.enumerate_structures(s)), (which, s)
    print(f"\n{which}: {n_rows} rows compared, {n_tied} neighbours of equal energy whose order the walk decides")
    assert n_tied > 1000


# ---- 3. beyond enumeration

def test_gpu_subopt_equals_the_walk_at_60_to_90_nt(sets):
    seqs = mirror_sequences()
    recs, rows, dcal = wuchty.subopt_batch_raw(seqs, 300)
    want = mirror_band(sets, "builtin", seqs, 300)
    assert not any(r["status"] for r in recs)
    for k, s in enumerate(seqs):
        assert pairs_of(rows, dcal, k) == want[k], s
    assert evaluate_back(seqs, rows, dcal) == sum(map(len, want))
    print("\nstructures within 3 kcal/mol at 60-90 nt:", [r["n_structs"] for r in recs])
    # the bulge of 30 is in the ensemble, the one of 31 is not
    assert any(t.startswith("(((((" + "." * 30 + "(((((") for t, _ in pairs_of(rows, dcal, 6))
    assert not any(t.startswith("(((((" + "." * 31 + "(") for t, _ in pairs_of(rows, dcal, 7))


LONG_DELTA, LONG_MAX = 20, 50000
LONG_COUNTS = (12, 3216)    # structures within LONG_DELTA dcal of the 200-nt and the 1500-nt sequence (at 40 dcal: 24 and 17 024)


def test_gpu_subopt_200_nt_beside_1500_nt():
    rng = np.random.default_rng(1500)
    seqs = [rand(rng, 200), rand(rng, 1500, "ACGU", [0.1, 0.4, 0.4, 0.1])]
    recs, rows, dcal = wuchty.subopt_batch_raw(seqs, LONG_DELTA, max_structs=LONG_MAX)
    print("\nstructures within", LONG_DELTA, "dcal at 200 / 1500 nt:", [r["n_structs"] for r in recs], [r["status"] for r in recs])
    assert not any(r["status"] for r in recs)
    assert tuple(r["n_structs"] for r in recs) == LONG_COUNTS
    mfe = zuker.mfe_batch_raw(seqs)
    evaluate_back(seqs, rows, dcal)
    for k in range(2):
        got = pairs_of(rows, dcal, k)
        assert len(got) >= 2 and len({t for t, _ in got}) == len(got)
        assert got[0][1] == mfe[1][k] == recs[k]["mfe_dcal"] and all(e <= mfe[1][k] + LONG_DELTA for _, e in got)
        assert [e for _, e in got] == sorted(e for _, e in got)
        assert mfe[0][k] in [t for t, e in got if e == mfe[1][k]]


# ---- 4. samples that fall into the band are members of it

def test_gpu_samples_within_the_band_are_members_of_it():
    seqs = mirror_sequences()
    delta, n = 300, 2000
    recs, rows, dcal = wuchty.subopt_batch_raw(seqs, delta)
    srecs, srows, sdcal = mccaskill.sample_batch_raw(seqs, n, seeds=11)
    n_in = 0
    for k in range(len(seqs)):
        member = dict(pairs_of(rows, dcal, k))
        for r in np.nonzero(sdcal[k] <= recs[k]["mfe_dcal"] + delta)[0]:
            text = srows[k][r, :-1].tobytes().decode("ascii")
            assert member.get(text) == int(sdcal[k][r]), (seqs[k], text)
            n_in += 1
    print(f"\n{n_in} of {n * len(seqs)} samples lie within {delta} dcal of their minimum")
    assert n_in > n


# ---- 5. same input, same bits

def test_gpu_subopt_same_input_same_bits():
    rng = np.random.default_rng(6)
    seqs = [rand(rng, n) for n in (33, 58, 71, 20, 64, 45, 80, 9)]
    delta = 300
    whole = wuchty.subopt_batch_raw(seqs, delta)
    want = {s: bits(*whole, k) for k, s in enumerate(seqs)}
    counts = [r["n_structs"] for r in whole[0]]
    assert all(r["status"] == 0 for r in whole[0]) and max(counts) > 50
    for k in (0, 3, len(seqs) - 1):                                                # alone
        assert bits(*wuchty.subopt_batch_raw([seqs[k]], delta), 0) == want[seqs[k]]
    got = wuchty.subopt_batch_raw(seqs[::-1], delta)                               # reversed: every sequence at another position
    assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs[::-1]]
    got = wuchty.subopt_batch_raw(seqs, delta, workspace_bytes=1)                  # one sequence per chunk
    assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs]
    assert N_counters()[3] == len(seqs)
    got = wuchty.subopt_batch_raw(seqs, delta, max_structs=max(counts))            # max_structs just large enough ...
    assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs]
    for k in (1, 2):                                                               # ... for each sequence: exactly its count
        assert bits(*wuchty.subopt_batch_raw([seqs[k]], delta, max_structs=counts[k]), 0) == want[seqs[k]]
    got = wuchty.subopt_batch_raw(seqs[:3], delta, max_structs=2000000)            # ... and far above it
    assert [bits(*got, k) for k in range(3)] == [want[s] for s in seqs[:3]]


def N_counters():
    out = (ctypes.c_longlong * 7)()
    N.check(N.lib().rafft_subopt_counters(ctypes.byref(out)))
    return list(out)


# ---- 6. capacity

def test_gpu_subopt_capacity_stays_with_its_sequence():
    rng = np.random.default_rng(8)
    seqs = [rand(rng, 40), rand(rng, 70), rand(rng, 30)]
    delta = 400
    whole = wuchty.subopt_batch_raw(seqs, delta)
    counts = [r["n_structs"] for r in whole[0]]
    k = int(np.argmax(counts))
    assert counts[k] > max(c for x, c in enumerate(counts) if x != k) > 1
    recs, rows, dcal = wuchty.subopt_batch_raw(seqs, delta, max_structs=counts[k] - 1)       # returns: the call is RAFFT_OK
    assert [r["status"] for r in recs] == [N.ERR_CAPACITY if x == k else 0 for x in range(3)]
    assert recs[k]["n_structs"] == 0 and len(dcal[k]) == 0 and counts[k] - 1 < recs[k]["n_reached"] <= counts[k]
    assert recs[k]["mfe_dcal"] == whole[0][k]["mfe_dcal"]
    assert N.lib().rafft_last_error().decode().startswith(f"sequence {k}:")
    assert [bits(recs, rows, dcal, x) for x in range(3) if x != k] == [bits(*whole, x) for x in range(3) if x != k]
    exact = wuchty.subopt_batch_raw(seqs, delta, max_structs=counts[k])
    assert [bits(*exact, x) for x in range(3)] == [bits(*whole, x) for x in range(3)]
    with pytest.raises(N.RafftError) as e:
        wuchty.subopt_batch(seqs, delta / 100.0, max_structs=counts[k] - 1)
    assert e.value.code == N.ERR_CAPACITY
    assert [g is None for g in wuchty.subopt_batch(seqs, delta / 100.0, max_structs=counts[k] - 1, raise_errors=False)] == [x == k for x in range(3)]


# ---- 7. errors

def test_gpu_subopt_errors_stay_with_their_sequence():
    rng = np.random.default_rng(404)
    good = ["GGGGAAAACCCC", rand(rng, 40), "GCGCUUCGGCGC", rand(rng, 25)]
    seqs = [good[0], "", good[1], "GGGXAAACCC", good[2], "A" * (N.MFE_MAX_LEN + 1), good[3]]
    at = [0, 2, 4, 6]
    alone = wuchty.subopt_batch_raw(good, 200)
    recs, rows, dcal = wuchty.subopt_batch_raw(seqs, 200)
    assert [r["status"] for r in recs] == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, 0, N.ERR_TOO_LONG, 0]
    assert N.lib().rafft_last_error().decode().startswith("sequence 1")
    assert all(recs[k]["n_structs"] == 0 and len(dcal[k]) == 0 for k in (1, 3, 5))
    assert [bits(recs, rows, dcal, k) for k in at] == [bits(*alone, k) for k in range(len(good))]
    got = rafft_amd.subopt_batch(seqs, 2.0, raise_errors=False)
    assert [g is None for g in got] == [False, True, False, True, False, True, False]
    assert [(st.str_struct, st.dcal) for st in got[0]] == pairs_of(rows, dcal, 0)
    # RAFFT_ERR_PARAM: nothing is returned, and the next call is exact
    L = N.lib()
    seq = (ctypes.c_char_p * 1)(good[0].encode())
    ln = (ctypes.c_int * 1)(12)
    for args in ((-1, seq, ln, 37.0, 100, 10, 0), (1, None, ln, 37.0, 100, 10, 0), (1, seq, None, 37.0, 100, 10, 0), (1, seq, ln, 37.0, -1, 10, 0),
                 (1, seq, ln, 37.0, N.SUBOPT_MAX_DELTA + 1, 10, 0), (1, seq, ln, 37.0, 100, 0, 0), (1, seq, ln, 37.0, 100, N.SUBOPT_MAX_STRUCTS + 1, 0),
                 (1, seq, ln, 37.0, 100, 10, -1)):
        out = ctypes.POINTER(N.SuboptResult)()
        assert L.rafft_subopt_batch(*args, ctypes.byref(out)) == N.ERR_PARAM and not out
    assert L.rafft_subopt_batch(1, seq, ln, 37.0, 100, 10, 0, None) == N.ERR_PARAM
    assert bits(*wuchty.subopt_batch_raw(good[:1], 200), 0) == bits(*alone, 0)
    with pytest.raises(N.RafftError) as e:                                         # the built-in tables are 37 C only
        wuchty.subopt_batch_raw(good, 200, temp=25.0)
    assert e.value.code == N.ERR_TEMP


# ---- 8. other temperatures

def test_gpu_subopt_at_other_temperatures(sets):
    install(sets, "synthetic")
    seqs = exhaustive_sequences()
    at37 = wuchty.subopt_batch_raw(seqs, 150, max_structs=60000)
    for temp in (25.0, 60.0):
        for delta in (150, 500):
            recs, rows, dcal = wuchty.subopt_batch_raw(seqs, delta, max_structs=60000, temp=temp)
            want = mirror_band(sets, "synthetic", seqs, delta, temp)
            assert not any(r["status"] for r in recs)
            for k, s in enumerate(seqs):
                assert pairs_of(rows, dcal, k) == want[k], (temp, delta, s)
            evaluate_back(seqs, rows, dcal, temp)
    again = wuchty.subopt_batch_raw(seqs, 150, max_structs=60000)
    assert [bits(*again, k) for k in range(len(seqs))] == [bits(*at37, k) for k in range(len(seqs))]
    want = mirror_band(sets, "synthetic", seqs, 150)
    assert [pairs_of(again[1], again[2], k) for k in range(len(seqs))] == want


# ---- 9. the command line as a process

def test_gpu_cli_subopt_writes_one_step_in_the_librarys_order(tmp_path):
    seqs = ["GGGAAACCCAGGGAAACCCAGCGCAAAGCGC", "GCGCUUCGGCGCAAGGGAAACCC"]
    fa = tmp_path / "s.fa"
    fa.write_text("".join(f">s{k}\n{s}\n" for k, s in enumerate(seqs)))
    f = tmp_path / "f"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-sf", str(fa), "--batch", "--subopt", "1.5", "-o", str(f)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = rafft_amd.subopt_batch(seqs, 1.5)
    # one graph per sequence, back to back: cut the file at the sequence lines
    lines = f.read_text().splitlines(keepends=True)
    starts = [k for k, ln in enumerate(lines) if ln.strip() in seqs]
    assert len(starts) == len(seqs)
    blocks = ["".join(lines[a:b]) for a, b in zip(starts, starts[1:] + [len(lines)])]
    one = tmp_path / "one"
    for s, blk, w in zip(seqs, blocks, want):
        one.write_text(blk)
        steps, got_seq = parse_rafft_output(str(one))
        assert got_seq == s and len(steps) == 1
        assert [st.str_struct for st in steps[0]] == [st.str_struct for st in w] and len(w) > 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-s", seqs[0], "--subopt", "1.5", "--mfe"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--subopt gives every structure of every sequence within an energy band: no --mfe" in r.stderr
