"""Tie-heavy, low-complexity sequences (repeats) on the CPU: the oracle against fixtures made by the reference's own
Python (tools/make_golden_ties.py), and the conditions that make those fixtures worth having.

On i.i.d. sequences hardly any decision of a fold is a tie; on repeats nearly every one is, and the reference defines
the outcome only implicitly: lags are ranked by value descending, then lag descending; the best stem of a lag is a
`>=` arg-max; the beam is a children-before-parents stable merge.  tests/test_gpu_ties.py holds the GPU side."""
import numpy as np
import pytest

import oracle
from conftest import load_json_gz


@pytest.fixture(scope="module")
def tie_cases():
    return load_json_gz("fold_traj_ties.json.gz")


@pytest.fixture(scope="module")
def tie_records():
    return load_json_gz("node_expand_ties.json.gz")


def noncontiguous(pos):
    return any(b - a != 1 for a, b in zip(pos, pos[1:]))


def cut_ties(cor, lags):
    """(lags of the whole profile that carry the value of the last ranked lag, how many of them were ranked)"""
    cut = cor[lags[-1]]
    return sum(1 for v in cor if v == cut), sum(1 for k in lags if cor[k] == cut)


def test_fold_trajectories_match_reference_python(tie_cases):
    assert len(tie_cases) >= 8 * 4 + 6 + 2
    for case in tie_cases:
        _, traj = oracle.fold(case["seq"], traj=True, **case["params"])
        got = [[[s.str_struct, s.dcal] for s in st] for st in traj]
        assert got == case["traj"], (case["family"], len(case["seq"]), case["params"])


def test_node_expansion_matches_reference_python(tie_records):
    for r in tie_records:
        cor = oracle.autocor(r["seq"], r["pos"], r["gc"], r["au"], r["gu"])
        np.testing.assert_array_equal(cor, np.array(r["cor"]))  # exact: integer weights, direct convolution
        ex = oracle.expand_node(r["seq"], r["db"], r["pos"], r["nb_mode"], r["min_hp"], r["min_nrj"],
                                r["gc"], r["au"], r["gu"])
        assert ex["lag"] == r["lags"]                           # value descending, then lag descending
        assert ex["cor"] == [r["cor"][k] for k in r["lags"]]
        ws = [[a, b, c, d] for a, b, c, d in zip(ex["nb"], ex["mi"], ex["mj"], ex["score"])]
        assert ws == r["ws"]                                    # the `>=` arg-max of every ranked lag
        sol = [[ex["nb"][k], ex["score"][k], ex["mi"][k], ex["mj"][k], ex["ddcal"][k]] for k in ex["kept"]]
        assert sol == r["sol"]


def test_long_fixture_is_the_oracles(tie_cases):
    """fold_ties_long.json.gz is the oracle's own output (the reference's Python is too slow there): the cheapest case is
    folded again here, so that the file cannot drift from the oracle unnoticed; all of it is what the GPU test compares with"""
    longs = load_json_gz("fold_ties_long.json.gz")
    assert [(c["family"], len(c["seq"]), c["params"]["max_stack"]) for c in longs] == \
        [(f, L, 4) for f in ("GC", "CUG", "GGGGCCCC") for L in (1100, 1500)] + [("GC", 4200, 2)]
    c = longs[4]
    _, traj = oracle.fold(c["seq"], traj=True, **c["params"])
    assert [[[s.str_struct, s.dcal] for s in st] for st in traj] == c["traj"]
    for c in longs:
        for st in c["traj"]:
            assert len({db for db, _ in st}) == len(st) <= c["params"]["max_stack"]


# ---- the fixtures are what they claim to be: conditions, so that a regenerated fixture cannot lose its point silently

def test_fixture_covers_every_family(tie_cases, tie_records):
    fams = {"GC", "AU", "GU", "CUG", "GGGAAACCC", "GGGGCCCC", "GC+A", "GC+N5"}
    base = dict(nb_mode=100, max_stack=20, max_branch=1000)
    have = {(c["family"], len(c["seq"])) for c in tie_cases if c["params"] == base}
    assert have == {(f, L) for f in fams for L in (33, 130, 257, 600)}
    for f in ("CUG", "GGGAAACCC"):
        for ms, mb in ((1, 1000), (7, 7), (50, 3)):
            assert any(c["family"] == f and len(c["seq"]) == 130 and c["params"] == dict(nb_mode=100, max_stack=ms, max_branch=mb)
                       for c in tie_cases), (f, ms, mb)
    assert any(c["params"].get("gc_wei") == c["params"].get("au_wei") == c["params"].get("gu_wei") == 1.0 for c in tie_cases)
    assert any(c["params"].get("min_hp") == 1 for c in tie_cases)
    assert len(tie_records) >= 150
    assert sum(noncontiguous(r["pos"]) for r in tie_records) >= 40
    for f in fams:
        mine = [r for r in tie_records if r["family"] == f]
        assert any(r["pos"] == list(range(len(r["seq"]))) for r in mine), f                # root regions
        # (nothing forms on the GU repeat; the GC and AU repeats zip up into ONE hairpin from end to end, which leaves contiguous
        #  regions only - their split regions are made by hand in tests/test_gpu_ties.py)
        if f not in ("GU", "GC", "AU"):
            assert any(noncontiguous(r["pos"]) for r in mine), f
            assert any(not noncontiguous(r["pos"]) and len(r["pos"]) < len(r["seq"]) for r in mine), f


def test_roots_of_pure_repeats_are_one_big_tie(tie_records):
    """GC, AU and GU roots of 130 nt and more: the 100 ranked values are ONE value, carried by more than 100 lags"""
    seen = set()
    for r in tie_records:
        n = len(r["pos"])
        if r["family"] in ("GC", "AU", "GU") and n >= 130 and r["pos"] == list(range(len(r["seq"]))) and r["nb_mode"] == 100:
            top = {r["cor"][k] for k in r["lags"]}
            assert len(r["lags"]) == 100 and len(top) == 1, (r["family"], n)
            cor = oracle.autocor(r["seq"], r["pos"], r["gc"], r["au"], r["gu"])
            assert int((cor == top.pop()).sum()) > 100, (r["family"], n)
            seen.add((r["family"], n))
    assert seen == {(f, n) for f in ("GC", "AU", "GU") for n in (130, 257, 600)}


def test_the_cut_falls_inside_tie_groups(tie_records):
    inside = 0
    for r in tie_records:
        tied, taken = cut_ties(r["cor"], r["lags"])
        inside += tied > taken
    assert inside >= 30, inside


def test_beams_are_full_of_equal_energies(tie_cases):
    c, = [c for c in tie_cases if c["family"] == "CUG" and len(c["seq"]) == 130
          and c["params"] == dict(nb_mode=100, max_stack=20, max_branch=1000)]
    pairs = sum(a[1] == b[1] for st in c["traj"] for a, b in zip(st, st[1:]))
    assert pairs >= 100, pairs                    # (347 when the fixture was made)


def test_no_step_lists_a_structure_twice(tie_cases):
    for c in tie_cases:
        for k, st in enumerate(c["traj"]):
            assert len({db for db, _ in st}) == len(st), (c["family"], len(c["seq"]), c["params"], k)
