"""The expand classes at their span and branch-count edges, on a real MI355X (`-m gpu`): the constructed parents of
tests/_class_edges.py through the expand seam, and whole folds forced through a loop on each span edge, under the three routings of
tests/test_gpu_ties.py.  tests/test_class_edges.py (CPU) shows that every parent lands in the class it is built for and that every
fold visits its loop.  Expected values: the oracle.  Integers and bit-equal fp64 throughout: no tolerance."""
import pytest

import oracle
import rafft_amd
from rafft_amd import _native as N, rafft as R
import _class_edges as CE
import _loops as LP

pytestmark = pytest.mark.gpu

KEYS = ("lag", "cor", "nb", "mi", "mj", "score", "ddcal", "kept")
SETTINGS = ((100, 3, 0.0), (100, 0, LP.HIGH_NRJ))            # (nb_mode, min_hp, min_nrj)
SMALL = ("16,32", "16,16", "0,0")                            # RAFFT_SMALL: both small teams, the 16-lane one alone, neither


@pytest.fixture(autouse=True, params=["classes_by_size", "classes_merged", "general_builds"])
def expand_class_routing(request, monkeypatch):
    """the three routings of tests/test_gpu_ties.py"""
    if request.param in ("classes_by_size", "general_builds"):
        monkeypatch.setenv("RAFFT_MERGE_BELOW", "0")
        monkeypatch.setenv("RAFFT_MERGE2_BELOW", "0")
    if request.param == "general_builds":
        monkeypatch.setenv("RAFFT_PROD", "0")
    yield


# the oracle's answers are computed once and shared by the three routings
_ORACLE_NODES, _ORACLE_FOLDS = {}, {}


def oracle_node(name, seq, db, pos, setting):
    key = (name, setting)
    if key not in _ORACLE_NODES:
        _ORACLE_NODES[key] = oracle.expand_node(seq, db, pos, *setting)
    return _ORACLE_NODES[key]


def check_parents(parents, monkeypatch, smalls):
    for name, seq, db, pos, _ in parents:
        for setting in SETTINGS:
            o = oracle_node(name, seq, db, pos, setting)
            assert o["kept"], (name, setting)
            for small in smalls:
                if small is not None:
                    monkeypatch.setenv("RAFFT_SMALL", small)
                g = R.expand_node(seq, db, pos, *setting)
                for key in KEYS:
                    assert g[key] == o[key], (name, setting, small, key)


@pytest.mark.parametrize("span", CE.SMALL_SPANS + CE.WAVE_SPANS)
def test_gpu_span_parents_vs_oracle(monkeypatch, span):
    """one loop of exactly `span` nt from closing pair to closing pair - 448 | 449: the window of the small-region kernel, 1280 | 1281:
    the staged bases of the one-wavefront class - at every ci mod 4 (how far the word-wise copy of the bases starts before the loop),
    at the 5' end, at the 3' end of a 4096-nt sequence (the copy reads up to the sequence's last base) and of a 4097-nt one (no copy)"""
    check_parents(CE.span_parents((span,)), monkeypatch, SMALL)


def test_gpu_small_loops_behind_position_4000_vs_oracle(monkeypatch):
    """the staged bases are addressed by sequence position through a pointer shifted back by ci: ci >= 4000 of a 4096-nt sequence,
    in both small teams and in the one-wavefront class"""
    check_parents(CE.tail_parents(), monkeypatch, SMALL)


@pytest.mark.parametrize("k", CE.BRANCH_K)
def test_gpu_many_branch_parents_vs_oracle(monkeypatch, k):
    """k hairpins in one loop: the full 1024-entry branch list of the wide classes, the class for the biggest regions entered through
    the branch count alone (k >= 1025), and its 4096-word list and the 12-bit cut points of a candidate at their last value (4095)"""
    check_parents(CE.branch_parents((k,)), monkeypatch, (None,))


def test_gpu_a_loop_of_4096_helices_is_refused_and_the_next_call_is_exact(monkeypatch):
    for name, seq, db, pos, want in CE.branch_parents((CE.BIG_BR + 1,)):
        assert want is None
        with pytest.raises(N.RafftError) as e:
            R.expand_node(seq, db, pos, 100, 3, 0.0)
        assert e.value.code == N.ERR_PARAM, name
    check_parents(list(CE.branch_parents((255,), (2,))) + list(CE.tail_parents())[:2], monkeypatch, (None,))


@pytest.mark.parametrize("params", CE.ONION_PARAMS)
def test_gpu_folds_through_a_loop_on_every_span_edge_vs_oracle(params):
    """production builds (the seam only runs the general ones): every onion of tests/_class_edges.py in one batch, whole trajectories"""
    cases = list(CE.onions())
    seqs = [c[1] for c in cases]
    for s in seqs:
        if (s, params) not in _ORACLE_FOLDS:
            _ORACLE_FOLDS[(s, params)] = [[(x.str_struct, x.dcal) for x in st] for st in oracle.fold(s, *params, traj=True)[1]]
    got = rafft_amd.fold_batch(seqs, *params, traj=True)
    for c, (fin, traj) in zip(cases, got):
        assert [[(x.str_struct, x.dcal) for x in st] for st in traj] == _ORACLE_FOLDS[(c[1], params)], c[0]
