"""The constructed parents and folds of tests/_class_edges.py do what they are built for (CPU only: the product's own node_class()
compiled for the host, and the oracle): every parent lands in its class, the two sides of every edge land in different ones, every
onion's fold visits its loop, every parent is a structure the oracle evaluates and expands with stems where they are wanted - and
rafft_expand_node refuses a loop of more than 4095 helices before it touches a device."""
import os
import subprocess

import pytest

import oracle
from rafft_amd import _native as N, rafft as R
import _class_edges as CE
import _loops as LP
from conftest import ROOT

SEAM = dict(cls1_P=512, cls1_br=256, K=100, sm=(16, 32))         # what rafft_expand_node runs with (general builds, FFT buffers)
PRODUCTION = dict(cls1_P=512, cls1_br=128, K=100, sm=(16, 32))   # a fold at nb_mode 100 (the one-wavefront class without FFT buffers)
SETTINGS = ((100, 3, 0.0), (100, 0, LP.HIGH_NRJ))


@pytest.fixture(scope="module")
def node_class(tmp_path_factory):
    """-> (constants of rafft_kernels.h, classify(list of (n, span, nbr), limits) -> list of classes)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "node_class_check")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-Wno-unused-function", "-Wno-missing-braces",
                           os.path.join(ROOT, "tests", "hostcheck", "node_class_check.cpp"), "-o", exe])

    def run(triples, lim, merge=0):
        text = "".join(f"{n} {span} {nbr} {merge} {lim['cls1_P']} {lim['cls1_br']} {lim['K']} {lim['sm'][0]} {lim['sm'][1]}\n" for n, span, nbr in triples)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split("\n")
        words = lines[0].split()
        got = [int(x) for x in lines[1:] if x]
        assert len(got) == len(triples)
        return dict(zip(words[0::2], map(int, words[1::2]))), got

    return run((), SEAM)[0], lambda triples, lim=SEAM, merge=0: run(triples, lim, merge)[1]


def triple(seq, db, pos):
    """(n, span, branches) of the region as the product classifies it: the span of a loop under a pair is closing pair to closing
    pair; the exterior loop's, and every loop's of a sequence beyond LDS_SEQ, is the sequence"""
    pt = LP.pair_table(db)
    br = LP.branches_of(db, pos)
    ci = max([i for i in range(pos[0]) if pt[i] > pos[0]], default=-1)      # the innermost pair around the region
    L = len(seq)
    span = L if (ci < 0 or L > CE.LDS_SEQ) else pt[ci] + 1 - ci
    return len(pos), span, len(br)


@pytest.fixture(scope="module")
def parents():
    return list(CE.span_parents()) + list(CE.tail_parents()) + list(CE.branch_parents())


def test_constants_are_the_products(node_class):
    c = node_class[0]
    assert (c["SM_SPAN"], c["CLS01_L"], c["MAX_BR"], c["BIG_BR"], c["LDS_SEQ"]) == (CE.SM_SPAN, CE.CLS01_L, CE.MAX_BR, CE.BIG_BR, CE.LDS_SEQ)
    assert (c["CLS1_P"], c["CLS1_BR"], c["CLS2_P"], c["MAX_P"]) == (512, 256, 2048, 8192)


def test_every_parent_lands_in_the_class_it_is_built_for(node_class, parents):
    names = [p[0] for p in parents]
    assert len(set(names)) == len(names) == 144 + 16 + 32 + 2
    t = [triple(s, d, pos) for _, s, d, pos, _ in parents]
    for lim in (SEAM, PRODUCTION):
        got = node_class[1](t, lim)
        wrong = [(p[0], tr, g, p[4]) for p, tr, g in zip(parents, t, got) if g != p[4]]
        assert not wrong, wrong[:8]
    assert {p[4] for p in parents} == {0, 1, 2, 3, 4, 5}
    # the shapes are the ones asked for
    for (name, s, d, pos, want), (n, span, nbr) in zip(parents, t):
        f = name.split("/")
        if f[0] == "span":
            assert n == int(f[2][1:]) and nbr == 1 + (int(f[3][2:]) & 1)
            ci = pos[0] - 1
            assert ci % 4 == int(f[3][2:]) and LP.pair_table(d)[ci] + 1 - ci == int(f[1])
            assert len(s) == {"5p": int(f[1]) + ci, "3p4096": 4096, "3p4097": 4097}[f[4]]
            assert span == (4097 if f[4] == "3p4097" else int(f[1]))
            if f[4] != "5p":
                assert len(s) - 1 - LP.pair_table(d)[ci] <= 3           # the loop ends within three bases of the 3' end
        elif f[0] == "tail":
            assert len(s) == 4096 and pos[0] - 1 >= 4000 and (pos[0] - 1) % 4 == int(f[3][2:]) and span == int(f[1]) and n == int(f[2][1:])
        else:
            k, g = int(f[1][1:]), int(f[2][1:])
            assert nbr == k and n == (k if f[-1] == "full_list" else k + 1) * g and span == len(s) > CE.LDS_SEQ // 4


def test_the_two_sides_of_every_edge_land_in_different_classes(node_class, parents):
    by = {p[0]: c for p, c in zip(parents, node_class[1]([triple(s, d, pos) for _, s, d, pos, _ in parents]))}
    for n in CE.SMALL_N + CE.WAVE_N:
        lo, at, up = CE.SMALL_SPANS if n in CE.SMALL_N else CE.WAVE_SPANS
        for r in range(4):
            for where in ("5p", "3p4096"):
                a, b, c = (by[f"span/{s}/n{n}/ci{r}/{where}"] for s in (lo, at, up))
                assert a == b != c, (n, r, where, a, b, c)
            # ... and at 4097 nt the span is the sequence: the edge is gone, and with it the classes below it
            assert {by[f"span/{s}/n{n}/ci{r}/3p4097"] for s in (lo, at, up)} == {2}
            assert by[f"span/{at}/n{n}/ci{r}/3p4096"] != 2
    for g in CE.BRANCH_G:
        for where in ("ext", "GC"):
            assert by[f"branches/k1024/g{g}/{where}"] == 3 and by[f"branches/k1025/g{g}/{where}"] == 0
    # the branch limit of the one-wavefront class needs 257 helices within 1280 nt - five bases each at the least, 1285: no loop has
    # them, the parents of 255-257 helices go by their span; on bare numbers the edge is where CLS1_BR puts it
    assert node_class[1]([(256, 1280, 256), (256, 1280, 257)], SEAM) == [1, 2]
    assert node_class[1]([(200, 1280, 128), (200, 1280, 129)], PRODUCTION) == [1, 2]
    # merged steps have no small teams and no one-wavefront class
    assert node_class[1]([(16, 448, 1), (40, 1280, 1)], SEAM, merge=2) == [2, 2] and node_class[1]([(16, 448, 1)], SEAM, merge=3) == [3]


def test_class_0_is_reached_through_the_branch_count_alone(node_class, parents):
    seen = set()
    for name, s, d, pos, want in parents:
        if not name.startswith("branches/"):
            continue
        n, span, nbr = triple(s, d, pos)
        if nbr <= CE.MAX_BR:
            continue
        assert want == 0
        if 2 * n - 1 <= node_class[0]["MAX_P"]:              # the FFT plan would hold its lags: only the branch list does not fit
            assert node_class[1]([(n, span, nbr), (n, span, CE.MAX_BR)]) == [0, 2 if 2 * n - 1 <= 2048 else 3], name
            seen.add(nbr)
    assert seen == {1025, 4094, 4095}


@pytest.mark.parametrize("family", ["span", "tail"])
def test_span_parents_keep_stems_that_touch_both_ends_of_the_staged_bases(family):
    """every span parent is a structure the oracle evaluates; under both settings of the GPU test a kept stem has its outermost pair
    within two positions of ci and one within two of cj, so dE reads the first and the last staged base"""
    for name, seq, db, pos, _ in (CE.span_parents() if family == "span" else CE.tail_parents()):
        oracle.eval_structure(seq, db)
        ci = pos[0] - 1
        cj = LP.pair_table(db)[ci]
        assert cj > pos[-1]
        for setting in SETTINGS:
            o = oracle.expand_node(seq, db, pos, *setting)
            outer = [(pos[o["mi"][k] - o["nb"][k] + 1], pos[o["mj"][k] + o["nb"][k] - 1]) for k in o["kept"]]
            assert any(a - ci <= 2 for a, b in outer) and any(cj - b <= 2 for a, b in outer), (name, setting)


@pytest.mark.parametrize("k", CE.BRANCH_K)
def test_branch_parents_keep_stems_over_no_one_and_nearly_all_branches(k):
    """valid structures with k branches in the loop; with every ranked stem kept (min_nrj 1e6) there are stems that enclose one branch,
    k - 1 and all k - the 12-bit cut points of a candidate see the values at their upper end - and, where a segment has two bases,
    none"""
    for name, seq, db, pos, _ in CE.branch_parents((k,)):
        oracle.eval_structure(seq, db)
        assert len(LP.branches_of(db, pos)) == k and len(seq) <= 32768
        o = oracle.expand_node(seq, db, pos, 100, 0, LP.HIGH_NRJ)
        counts = CE.stem_branch_counts(db, pos, o)
        kept = {counts[x] for x in o["kept"]}
        g = len(pos) // k
        assert {1, k - 1} <= kept and (k in kept or name.endswith("full_list")) and (g == 1 or 0 in kept), (name, sorted(kept))
        assert len(kept) >= 30                               # ... and the counts between are spread out
        assert oracle.expand_node(seq, db, pos, 100, 3, 0.0)["kept"], name


@pytest.mark.parametrize("params", CE.ONION_PARAMS)
def test_every_onion_fold_visits_its_loop(params):
    """the oracle's trajectory of every onion holds a structure with a loop of exactly the (n, span, branches) it is built for, and
    goes on from there: a sequence that stops visiting its edge fails here"""
    cases = list(CE.onions())
    assert len(cases) == 48
    for name, seq, want in cases:
        _, traj = oracle.fold(seq, *params, traj=True)
        hit = [k for k, st in enumerate(traj) if any(want in CE.loops_of(s.str_struct) for s in st)]
        assert hit and hit[0] < len(traj) - 1, (name, len(traj))
        assert traj[-1][0].str_struct.count("(") > traj[hit[0]][0].str_struct.count("("), name       # the edge region kept a stem


def test_loop_walker_on_hand_made_rows():
    assert CE.loops_of("....") == {(4, 4, 0)}
    assert CE.loops_of("(...)") == {(0, 5, 1), (3, 5, 0)}
    assert CE.loops_of(".((..(...)..(...).)).") == {(2, 21, 1), (0, 19, 1), (5, 17, 2), (3, 5, 0)}


@pytest.mark.parametrize("g", CE.BRANCH_G)
def test_expand_node_refuses_a_loop_of_4096_helices_before_touching_a_device(g):
    """(the check precedes the call's first use of the device: it is reached here, with or without one)"""
    for name, seq, db, pos, want in CE.branch_parents((CE.BIG_BR + 1,), (g,)):
        assert want is None and len(LP.branches_of(db, pos)) == 4096 and len(seq) <= 32768
        oracle.eval_structure(seq, db)                       # a well-formed structure: only the number of helices is refused
        with pytest.raises(N.RafftError) as e:
            R.expand_node(seq, db, pos, 100, 3, 0.0)
        assert e.value.code == N.ERR_PARAM and "4095" in str(e.value) and "4096" in str(e.value), name
