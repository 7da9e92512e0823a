"""The beam step's `seen` tables with their occupancy in an LDS bitmap, on a real MI355X (`-m gpu`).

A table whose bitmap (one bit per slot) fits the beam-step launch's LDS budget is never zeroed: bit s set <=> slot s holds a key, the
bitmap travels between HBM and LDS once per step, lookups that find their home bit clear touch no HBM, inserts claim a slot with an
LDS atomic.  A table beyond the budget keeps the compare-and-swap protocol on a zeroed table.  What can go wrong is the protocol, not
arithmetic: a lookup that misses a key that is there (a duplicate structure in a beam), one that finds a key that is not (a structure
lost), a growth that drops or doubles keys, bits that outlive their table.  Every one of those changes a beam, so every test compares
whole trajectories - every step's beam, in order, with its energies - with the oracle's, and the runs of one input under both
protocols with each other.  Exact comparisons, no tolerance.

RAFFT_WIDE_BELOW=0 sends a small batch through the 256-thread kernel (the benchmark's bulk waves); by default a batch this small
takes the 1024-thread one.  RAFFT_SEEN_BM_MAX: the bitmap budget in bytes (0: compare-and-swap protocol throughout)."""
import numpy as np
import pytest

import rafft_amd

pytestmark = pytest.mark.gpu

_WANT = {}


def oracle_trajs(seqs, ms, mb):
    """the oracle's trajectories, computed once per (sequence, max_stack, max_branch) and shared by the tests"""
    from _oracle_pool import fold_many
    todo = [s for s in seqs if (s, ms, mb) not in _WANT]
    for s, t in zip(todo, fold_many([(s, 100, ms, mb, True) for s in todo])):
        _WANT[(s, ms, mb)] = t
    return [_WANT[(s, ms, mb)] for s in seqs]


def gpu_trajs(seqs, ms, mb):
    return [[[(x.str_struct, x.dcal) for x in st] for st in traj] for _, traj in rafft_amd.fold_batch(seqs, 100, ms, mb, traj=True)]


def kernel(monkeypatch, threads):
    if threads == 256:
        monkeypatch.setenv("RAFFT_WIDE_BELOW", "0")
    else:
        monkeypatch.delenv("RAFFT_WIDE_BELOW", raising=False)


def budget(monkeypatch, bm_max):
    if bm_max is None:
        monkeypatch.delenv("RAFFT_SEEN_BM_MAX", raising=False)
    else:
        monkeypatch.setenv("RAFFT_SEEN_BM_MAX", str(bm_max))


def rand(seed, L):
    return "".join(np.random.default_rng(seed).choice(list("ACGU"), L))


# ---- 1. lookups that hit: low-complexity sequences, where many combos of different parents give the same structure

REPEATS = ["GC" * 30, "GGGAAACCC" * 7, "GGGGCCCC" * 6]


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("mb", [1000, 7])
def test_gpu_bitmap_lookups_that_hit_vs_oracle(monkeypatch, threads, mb):
    """poly-GC, (GGGAAACCC)x7 and (GGGGCCCC)x6 at max_stack 50: max_branch 1000, and 7 - the cut-off falls inside a pass, so the
    keys of the pass beyond it must not be inserted"""
    kernel(monkeypatch, threads)
    want = oracle_trajs(REPEATS, 50, mb)
    got = gpu_trajs(REPEATS, 50, mb)
    budget(monkeypatch, 0)
    legacy = gpu_trajs(REPEATS, 50, mb)
    for k in range(len(REPEATS)):
        assert got[k] == want[k], (k, mb)
        assert legacy[k] == want[k], (k, mb)
        for st in got[k]:
            assert len({db for db, _ in st}) == len(st), (k, mb)


# ---- 2. and 3. growth: inside bitmap mode, across the budget, and without a bitmap

GROW_SEQS = [rand(120, 120), rand(300, 300)]
GROW_MS, GROW_MB = 600, 6000


@pytest.mark.parametrize("threads", [256, 1024])
def test_gpu_bitmap_growth_inside_and_across_the_budget_vs_oracle(monkeypatch, threads):
    """RAFFT_SEEN_FIXED=1: both tables start at 8192 slots (1 KiB of bitmap).  At max_stack 600, max_branch 6000 the 120-nt sequence
    accepts 8863 structures and the 300-nt sequence 26 216 (the oracle's count of children): their tables double twice, to 32 768
    slots, and three times, to 65 536 (RAFFT_TRACE=2 on the GPU prints the sizes).  Default budget: every doubling under the
    1024-thread kernel (32 KiB) and the first two under the 256-thread kernel (4 KiB) rebuild the bitmap in LDS, the third under the
    256-thread kernel leaves bitmap mode.  RAFFT_SEEN_BM_MAX=2048: the second doubling leaves it (bitmap -> compare-and-swap in the
    middle of a fold); 0: never a bitmap.  All three equal each other and the oracle."""
    kernel(monkeypatch, threads)
    monkeypatch.setenv("RAFFT_SEEN_FIXED", "1")
    want = oracle_trajs(GROW_SEQS, GROW_MS, GROW_MB)
    for bm_max in (None, 2048, 0):
        budget(monkeypatch, bm_max)
        got = gpu_trajs(GROW_SEQS, GROW_MS, GROW_MB)
        for k in range(len(GROW_SEQS)):
            assert got[k] == want[k], (bm_max, k)


# ---- 4. regrow: the wave is folded again, stale bits must not survive into the second attempt

@pytest.mark.parametrize("threads", [256, 1024])
def test_gpu_bitmap_regrow_starts_from_clean_bitmaps_vs_oracle(monkeypatch, threads):
    """RAFFT_TEST_OVF_AT=2: the first attempt is abandoned after two steps - its keys are in the tables and their bits in the bitmap
    arena - and the wave is folded again on the same workspace"""
    kernel(monkeypatch, threads)
    seqs = [rand(1000 + k, 48 + 7 * k) for k in range(8)]
    want = oracle_trajs(seqs, 20, 1000)
    monkeypatch.setenv("RAFFT_SPLIT", "0")
    monkeypatch.setenv("RAFFT_TEST_OVF_AT", "2")
    got = gpu_trajs(seqs, 20, 1000)
    assert rafft_amd.last_stats()["n_regrows"] == 1
    for k in range(len(seqs)):
        assert got[k] == want[k], k


# ---- 5. the 1024-thread variant on an ordinary batch, with the bitmap and without

def test_gpu_bitmap_1024_thread_kernel_vs_oracle(monkeypatch):
    """a batch below RAFFT_WIDE_BELOW (twelve random sequences of 40-260 nt, max_stack 50): tables sized from the lengths"""
    monkeypatch.delenv("RAFFT_WIDE_BELOW", raising=False)
    seqs = [rand(2000 + k, 40 + 20 * k) for k in range(12)]
    want = oracle_trajs(seqs, 50, 1000)
    for bm_max in (None, 0):
        budget(monkeypatch, bm_max)
        got = gpu_trajs(seqs, 50, 1000)
        for k in range(len(seqs)):
            assert got[k] == want[k], (bm_max, k)


# ---- 6. a beam wider than the workgroup: the lookups and inserts of the parents that only replay their first combo

def test_gpu_bitmap_beam_wider_than_the_workgroup_vs_oracle(monkeypatch):
    """max_stack 300, max_branch 50 on 60 nt through the 256-thread kernel: after 50 children every later parent is in "one combo,
    then break" mode - more of them than the workgroup has threads"""
    kernel(monkeypatch, 256)
    seqs = [rand(60, 60), "GGGAAACCC" * 6 + "GGGAAA"]
    want = oracle_trajs(seqs, 300, 50)
    for bm_max in (None, 0):
        budget(monkeypatch, bm_max)
        got = gpu_trajs(seqs, 300, 50)
        for k in range(len(seqs)):
            assert got[k] == want[k], (bm_max, k)
    assert max(len(st) for t in want for st in t) > 256
