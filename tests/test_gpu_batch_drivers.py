"""The five batch drivers (rafft_mfe_batch, rafft_pf_batch, rafft_sample_batch, rafft_subopt_batch, rafft_kin_batch) on a real
MI355X (`-m gpu`), where an offset out of the planning they share (rafft_hostpure.h: chunk planner, sequence pack, the layouts of the
sequence drivers, graph pack, solve order) would show and no other test looks: sequences with errors BETWEEN the good ones while the
good ones are cut into chunks of two, and a kinetics chunk that holds exactly two solvable graphs with an unsolved one between them.
Every comparison is bit for bit against the same call in one chunk."""
import ctypes

import numpy as np
import pytest

import _kin_graphs as K
import _loops as LP
import _mfe_np as MF
import _par_reader as PR
import _subopt_np as SB
from rafft_amd import _native as N, mccaskill, params, rafft_kin, wuchty, zuker

pytestmark = pytest.mark.gpu

GOOD_LENGTHS = (33, 58, 71, 20, 64, 45, 80, 9)           # as test_gpu_mfe_same_input_same_bits
BAD = ["", "GGGXAAACCC", "A" * (N.MFE_MAX_LEN + 1)]
BAD_STATUS = [N.ERR_EMPTY, N.ERR_BAD_CHAR, N.ERR_TOO_LONG]
BAD_AT = (2, 6, 9)
FEW_TIMES = np.array([0.05, 0.4, 3.0, 40.0, 1e4, 1e9])


def mixed():
    """(all eleven sequences, the eight good ones, where the good ones stand)"""
    rng = np.random.default_rng(55)
    good = ["".join(rng.choice(list("ACGU"), n)) for n in GOOD_LENGTHS]
    seqs = good[:2] + [BAD[0]] + good[2:5] + [BAD[1]] + good[5:7] + [BAD[2]] + good[7:]
    keep = [k for k in range(len(seqs)) if k not in BAD_AT]
    assert [seqs[k] for k in BAD_AT] == BAD and [seqs[k] for k in keep] == good
    return seqs, good, keep


def test_gpu_mfe_errors_between_chunks_of_two():
    """every good sequence in the device-memory class (max_lds_len=4); a budget for the tables of two 64-nt sequences cuts the eight
    into (33, 58) (71, 20) (64, 45) (80, 9) - 3 * 4 * (33^2 + 58^2 + 71^2) > 2 * 3 * 4 * 64^2 and so on - and a budget of 1 into eight"""
    seqs, good, keep = mixed()
    whole = zuker.mfe_batch_raw(seqs, max_lds_len=4)
    rows, dcal, n_pairs, status = whole
    assert status == [BAD_STATUS[BAD_AT.index(k)] if k in BAD_AT else N.OK for k in range(len(seqs))]
    assert [rows[k] for k in BAD_AT] == ["." * len(b) for b in BAD]
    alone = zuker.mfe_batch_raw(good, max_lds_len=4)
    assert ([rows[k] for k in keep], [dcal[k] for k in keep], [n_pairs[k] for k in keep], [status[k] for k in keep]) == alone
    for budget in (2 * 3 * 64 * 64 * 4, 1):
        assert zuker.mfe_batch_raw(seqs, max_lds_len=4, workspace_bytes=budget) == whole, budget
        assert zuker.mfe_batch_raw(good, max_lds_len=4, workspace_bytes=budget) == alone, budget


def pf_bits(rows, recs, probs, k):
    """everything rafft_pf_batch returns for sequence k, as bytes and integers (as bits() of tests/test_gpu_pf.py; a sequence above
    RAFFT_PF_MAX_LEN has no probability matrix)"""
    r = recs[k]
    return (rows[k], r["status"], r["length"], r["mfe_dcal"], r["n_pairs"], np.float64(r["energy"]).tobytes(), np.float64(r["mfe_frequency"]).tobytes(),
            None if probs[k] is None else probs[k].tobytes())


def test_gpu_pf_errors_between_chunks_of_two():
    """the same mix and the same cuts (six fp64 tables: 6 * 8 * (33^2 + 58^2 + 71^2) > 2 * 6 * 8 * 64^2 and so on); the budget is the
    MFE part's too.  One pack serves both parts: the MFE energy of every record is rafft_mfe_batch's"""
    seqs, good, keep = mixed()
    whole = mccaskill.pf_batch_raw(seqs, probs=True)
    n = len(seqs)
    assert [whole[1][k]["status"] for k in range(n)] == [BAD_STATUS[BAD_AT.index(k)] if k in BAD_AT else N.OK for k in range(n)]
    assert [whole[0][k] for k in BAD_AT] == ["." * len(b) for b in BAD]
    assert [whole[1][k]["mfe_dcal"] for k in range(n)] == zuker.mfe_batch_raw(seqs)[1]
    alone = mccaskill.pf_batch_raw(good, probs=True)
    assert [pf_bits(*whole, k) for k in keep] == [pf_bits(*alone, k) for k in range(len(good))]
    for budget in (2 * 6 * 64 * 64 * 8, 1):
        got = mccaskill.pf_batch_raw(seqs, workspace_bytes=budget, probs=True)
        assert [pf_bits(*got, k) for k in range(n)] == [pf_bits(*whole, k) for k in range(n)], budget
    rows, recs, probs = mccaskill.pf_batch_raw(BAD, probs=True)                    # nothing to fold: the call is RAFFT_OK
    assert rows == ["." * len(b) for b in BAD] and [r["status"] for r in recs] == BAD_STATUS
    assert all((r["mfe_dcal"], r["n_pairs"], r["energy"], r["mfe_frequency"]) == (0, 0, 0.0, 0.0) for r in recs)
    assert not probs[1].any()


def sample_bits(recs, rows, dcal, k):
    """everything rafft_sample_batch returns for sequence k, as bytes and integers"""
    r = recs[k]
    return (r["status"], r["length"], r["mfe_dcal"], r["n_samples"], np.float64(r["energy"]).tobytes(), rows[k].tobytes(), dcal[k].tobytes())


def test_gpu_sample_errors_between_chunks_of_two():
    """the same mix and the same cuts (three fp64 tables: 3 * 8 * (33^2 + 58^2 + 71^2) > 2 * 3 * 8 * 64^2 and so on; the rows of a
    chunk, 8 (L + 1) bytes a sequence, are far below the budget), eight samples a sequence, a seed of its own for each: rows and
    energies of a chunk come back from the chunk's own row and energy offsets, whatever stands between its sequences"""
    seqs, good, keep = mixed()
    n, seeds = len(seqs), [1000 + 17 * k for k in range(len(seqs))]
    whole = mccaskill.sample_batch_raw(seqs, 8, seeds)
    recs, rows, dcal = whole
    assert [recs[k]["status"] for k in range(n)] == [BAD_STATUS[BAD_AT.index(k)] if k in BAD_AT else N.OK for k in range(n)]
    assert [recs[k]["mfe_dcal"] for k in range(n)] == zuker.mfe_batch_raw(seqs)[1]
    for k, b in zip(BAD_AT, BAD):
        assert rows[k].shape == (8, len(b) + 1) and (rows[k][:, :-1] == ord(".")).all() and not rows[k][:, -1].any() and not dcal[k].any(), k
        assert (recs[k]["length"], recs[k]["mfe_dcal"], recs[k]["n_samples"], recs[k]["energy"]) == (len(b), 0, 0, 0.0), k
    for k in keep:
        assert recs[k]["n_samples"] == 8 and not rows[k][:, -1].any() and set(rows[k][:, :-1].tobytes()) <= set(b"(.)"), k
    alone = mccaskill.sample_batch_raw(good, 8, [seeds[k] for k in keep])
    assert [sample_bits(*whole, k) for k in keep] == [sample_bits(*alone, j) for j in range(len(good))]
    for budget in (2 * 3 * 64 * 64 * 8, 1):
        got = mccaskill.sample_batch_raw(seqs, 8, seeds, workspace_bytes=budget)
        assert [sample_bits(*got, k) for k in range(n)] == [sample_bits(*whole, k) for k in range(n)], budget


def subopt_bits(recs, rows, dcal, k):
    """everything rafft_subopt_batch returns for sequence k, as bytes and integers"""
    r = recs[k]
    return (r["status"], r["length"], r["mfe_dcal"], r["n_structs"], r["n_reached"], rows[k].tobytes(), dcal[k].tobytes())


def subopt_chunks():
    c = (ctypes.c_longlong * 7)()
    N.check(N.lib().rafft_subopt_counters(ctypes.byref(c)))
    return c[3]


def test_gpu_subopt_errors_between_chunks_of_two():
    """the same mix, max_structs 128 and a budget for the tables of two 64-nt sequences (three int32 tables, the cuts of the MFE
    test).  The frontiers do not cut earlier: two buffers of 128 states and 512 bytes of counts a sequence are 25088, 37376, 41472,
    20992, 41472, 29184, 49664 and 12800 bytes for the eight lengths (states of 96, 144, 160, 80, 160, 112, 192 and 48 bytes), at
    most 41472 + 29184 = 70656 for a pair, below the 98304 of the budget - so the counter of chunks is 4, and 8 with a budget of 1.
    delta is 150 dcal/mol: the walk of tests/_subopt_np.py finds 15, 13, 37, 2, 50, 2, 16 and 1 structures in that band, every
    count within max_structs and seven of them above 1, so that second states are read from their buffer offsets"""
    seqs, good, keep = mixed()
    n, delta, counts = len(seqs), 150, [15, 13, 37, 2, 50, 2, 16, 1]
    params.reset_params()                                       # the built-in tables, which the mirror reads
    mirror = MF.Mirror(PR.tables_at(LP.builtin_par(), 37.0))
    band = [SB.band(mirror, s, delta) for s in good]
    assert [len(b) for b in band] == counts and max(counts) <= 128 and sum(c > 1 for c in counts) == 7
    whole = wuchty.subopt_batch_raw(seqs, delta, max_structs=128)
    assert subopt_chunks() == 1
    recs, rows, dcal = whole
    assert [recs[k]["status"] for k in range(n)] == [BAD_STATUS[BAD_AT.index(k)] if k in BAD_AT else N.OK for k in range(n)]
    assert [recs[k]["n_structs"] for k in keep] == counts and all(recs[k]["n_structs"] == 0 and rows[k].shape[0] == 0 for k in BAD_AT)
    for j, k in enumerate(keep):
        assert [(rows[k][r, :-1].tobytes().decode("ascii"), int(dcal[k][r])) for r in range(counts[j])] == band[j], k
    alone = wuchty.subopt_batch_raw(good, delta, max_structs=128)
    assert [subopt_bits(*whole, k) for k in keep] == [subopt_bits(*alone, j) for j in range(len(good))]
    for budget, chunks in ((2 * 3 * 64 * 64 * 4, 4), (1, 8)):
        got = wuchty.subopt_batch_raw(seqs, delta, max_structs=128, workspace_bytes=budget)
        assert subopt_chunks() == chunks, budget
        assert "sequence 2" in N.lib().rafft_last_error().decode(), budget
        assert [subopt_bits(*got, k) for k in range(n)] == [subopt_bits(*whole, k) for k in range(n)], budget


def test_gpu_kin_batch_chunk_of_exactly_two():
    """a budget of exactly the matrices of the first two solvable graphs - one whose inverse fits LDS, one of 140 states that does
    not - with a malformed graph (no matrices, but rows) between them: the chunks are [0, 3) and [3, 4), the second solvable graph's
    blocks start behind the first's, and both integrate launches of the first chunk read their part of the solve order"""
    graphs = [K.facing_graph(), K.malformed_graphs()[0][1], K.star_graph(140), K.length_edge_graph(66)]
    call = lambda **kw: rafft_kin.kin_batch_call([rafft_kin._batch_graph(g)[:5] for g in graphs], FEW_TIMES, K.KT, 4, rates=True, **kw)
    whole = call()
    assert whole["status"] == [N.OK, N.ERR_STRUCT, N.OK, N.OK]
    S = whole["n_unique"]
    assert 0 < S[0] <= 128 and S[1] == 0 and S[2] == 140 and S[3] > 0
    budget = 3 * 8 * (S[0] * S[0] + S[2] * S[2])
    assert len(FEW_TIMES) * 8 * sum(whole["n_rows"][:3]) < budget          # the populations of the first chunk do not cut it earlier
    got = call(workspace_bytes=budget)
    assert got["status"] == whole["status"] and got["n_edges"] == whole["n_edges"] and got["n_unique"] == S
    assert "graph 1" in got["error"] and got["error"] == whole["error"]
    for k in range(4):
        assert np.array_equal(got["uid"][k], whole["uid"][k]) and np.array_equal(got["first_row"][k], whole["first_row"][k]), k
        if k == 1:
            assert got["pop"][k] is None and got["rate"][k] is None and (got["uid"][k] == -1).all() and len(got["uid"][k]) == whole["n_rows"][k] > 0
        else:
            assert got["pop"][k].tobytes() == whole["pop"][k].tobytes() and got["rate"][k].tobytes() == whole["rate"][k].tobytes(), k
            assert np.allclose(got["pop"][k].sum(axis=1), 1.0), k
