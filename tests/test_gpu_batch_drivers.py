"""The three batch drivers (rafft_mfe_batch, rafft_pf_batch, rafft_kin_batch) on a real MI355X (`-m gpu`), where an offset out of the
planning they share (rafft_hostpure.h: chunk planner, sequence pack, graph pack, solve order) would show and no other test looks:
sequences with errors BETWEEN the good ones while the good ones are cut into chunks of two, and a kinetics chunk that holds exactly
two solvable graphs with an unsolved one between them.  Every comparison is bit for bit against the same call in one chunk."""
import numpy as np
import pytest

import _kin_graphs as K
from rafft_amd import _native as N, mccaskill, rafft_kin, zuker

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
