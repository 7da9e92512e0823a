"""rafft_kin_batch / rafft_kin.kinetics_batch on the GPU: structure identity, rate matrices and populations of many graphs in one
call, on the constructed graphs of tests/_kin_graphs.py, the closed forms, the reference's examples against 60-digit arithmetic,
and end to end behind a fold.

The call has ONE kt.  Where a set of cases holds graphs built for other kt (the `energies` family), every graph goes through one
batch at kt 0.61 for what does not depend on kt (identity), and the rates of the graphs of each kt are checked in that kt's batch."""
import os

import numpy as np
import pytest

import _kin_graphs as K
from rafft_amd import _native as N
from rafft_amd import cli, rafft_kin, utils
from conftest import GOLD, load_json_gz

pytestmark = pytest.mark.gpu

CASES = K.well_formed_cases()
MALFORMED = dict(K.malformed_graphs())
FEW_TIMES = np.array([0.05, 0.4, 3.0, 40.0, 1e4, 1e9])
_cache = {}


def arrays(graph):
    return rafft_kin._batch_graph(graph)[:5]


def call(graphs, times, kt=K.KT, substeps=4, **kw):
    return rafft_kin.kin_batch_call([arrays(g) for g in graphs], times, kt, substeps, **kw)


def flat_rows(graph):
    return [st for step in graph for st in step]


def reference_rate(name):
    if name not in _cache:
        graph, kt = next((g, kt) for n, g, kt in CASES if n == name)
        _cache[name] = K.reference_rate_matrix(graph, kt)
        _cache[name].setflags(write=False)
    return _cache[name]


# ---------------------------------------------------------------- 1. identity and rates

def test_gpu_identity_and_rates_of_all_constructed_graphs_in_one_batch():
    res = call([g for _, g, _ in CASES], FEW_TIMES[:2], rates=True, substeps=1)
    assert res["status"] == [N.OK] * len(CASES), res["error"]
    row0 = 0
    for k, (name, graph, kt) in enumerate(CASES):
        ordered, index = K.unique_rows(graph)
        flat = flat_rows(graph)
        assert (res["n_rows"][k], res["row0"][k], res["n_unique"][k]) == (len(flat), row0, len(ordered)), name
        row0 += len(flat)
        assert res["uid"][k].tolist() == [index[st.str_struct] for st in flat], name
        assert res["first_row"][k].tolist() == [next(r for r, st in enumerate(flat) if st.str_struct == u.str_struct) for u in ordered], name
    for kt in sorted({kt for _, _, kt in CASES}):
        ks = [k for k, c in enumerate(CASES) if c[2] == kt]
        sub = res if kt == K.KT else call([CASES[k][1] for k in ks], FEW_TIMES[:2], kt=kt, rates=True, substeps=1)
        for at, k in enumerate(ks):
            name, at = CASES[k][0], k if kt == K.KT else at
            want, got = reference_rate(name), sub["rate"][at]
            assert np.array_equal(got != 0, want != 0), name
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=name)
            assert sub["n_edges"][at] == int(np.count_nonzero(want - np.diag(np.diag(want)))), name
            P = sub["pop"][at]
            # (one sub-step per interval: h times the hub's exit rate is 13 on the stars, where TR-BDF2 - L-stable, not positive -
            #  dips below 0 as solve_master_equation does; positivity is asked at the step sizes of tests 2 and 3)
            assert np.isfinite(P).all() and np.allclose(P.sum(axis=1), 1.0), name


# ---------------------------------------------------------------- 2. closed forms

def test_gpu_batch_populations_against_closed_forms(m=4):
    """the two-state and the star case of _kin_graphs.solver_cases() in one batch, on one time list, against their closed forms, held
    to what tests/test_gpu_kin_graphs.py asks of method="implicit" on them: non-negative, normalised, an error above round-off that
    falls to between 1/5 and 1/3 when the steps are halved (second order)"""
    times = K.solver_times(-9.0)
    graphs = [K.two_state_graph(-1.0), K.star_graph(K.SOLVER_STAR_LEAVES + 1, K.SOLVER_STAR_ENERGY)]
    exact = [K.two_state_populations(-1.0, K.KT, times), K.star_populations(K.SOLVER_STAR_LEAVES, K.SOLVER_STAR_ENERGY, K.KT, times)]
    a, b = call(graphs, times, substeps=m), call(graphs, times, substeps=2 * m)
    for k, name in enumerate(("two_state", "star")):
        for P in (a["pop"][k], b["pop"][k]):
            assert P.shape == exact[k].shape and P.min() > -1e-9 and np.allclose(P.sum(axis=1), 1.0)
        ea, eb = np.abs(a["pop"][k] - exact[k]).max(), np.abs(b["pop"][k] - exact[k]).max()
        print(f"{name}: error {ea:.3e} at substeps {m}, {eb:.3e} at {2 * m}, ratio {eb / ea:.4f}")
        assert ea > 1e-8 and eb > 1e-8
        assert 1 / 5 < eb / ea < 1 / 3


# ---------------------------------------------------------------- 3. the reference's examples

def test_gpu_batch_reference_examples_against_60_digit_truth():
    """both examples and an 8-nt two-state graph in one batch, on the union of the examples' own sample times (kinetics.json.gz; the
    call has one time list), each compared at its own times: the bounds tests/test_gpu_kinetics.py applies to the integrator.  The
    test after this one solves each example on its own times."""
    names = ["example_rafft_20.out", "example_rafft.out"]
    gold, truth = load_json_gz("kinetics.json.gz"), load_json_gz("kinetics_truth.json.gz")
    graphs = [utils.parse_rafft_output(os.path.join(GOLD, n))[0] for n in names] + [K.two_state_graph(-1.0, 8)]
    own = [np.array(gold[n]["times"][1:], dtype=np.float64) for n in names]
    times = np.unique(np.concatenate(own))
    res = call(graphs, times, substeps=32)
    assert res["status"] == [N.OK] * 3
    for k, n in enumerate(names):
        g, tr = gold[n], truth[n]
        flat = flat_rows(graphs[k])
        assert [flat[r].str_struct for r in res["first_row"][k]] == g["struct_list"]
        at = np.searchsorted(times, own[k])
        assert np.array_equal(times[at], own[k])
        P = res["pop"][k][at]
        ks, want = tr["sample_index"], np.array(tr["populations"])
        early = [i for i, s in enumerate(ks) if s <= 0.6 * tr["n_steps"]]
        e_early, e_all = np.abs(P[ks][early] - want[early]).max(), np.abs(P[ks] - want).max()
        print(f"{n}: {res['n_unique'][k]} states, error {e_early:.3e} over the first 60 %, {e_all:.3e} everywhere")
        assert e_early < 5e-6
        assert e_all < 2e-2
        assert int(np.argmax(P[-1])) == int(np.argmax(want[-1]))
        assert P.min() > -1e-9 and np.allclose(P.sum(axis=1), 1.0)
    assert np.abs(res["pop"][2] - K.two_state_populations(-1.0, K.KT, times)).max() < 5e-6


@pytest.mark.parametrize("name", ["example_rafft_20.out", "example_rafft.out"])
def test_gpu_batch_reference_example_on_its_own_schedule(name):
    """each example with the two-state graph on the example's OWN sample times - the schedule kinetics_batch(-mt, -ns) gives a user,
    coarser for the 68-state example than the union above - held to the same bounds"""
    g, tr = load_json_gz("kinetics.json.gz")[name], load_json_gz("kinetics_truth.json.gz")[name]
    graph = utils.parse_rafft_output(os.path.join(GOLD, name))[0]
    times = np.array(g["times"][1:], dtype=np.float64)
    res = call([graph, K.two_state_graph(-1.0, 8)], times, substeps=32)
    assert res["status"] == [N.OK] * 2
    flat = flat_rows(graph)
    assert [flat[r].str_struct for r in res["first_row"][0]] == g["struct_list"]
    P = res["pop"][0]
    ks, want = tr["sample_index"], np.array(tr["populations"])
    early = [i for i, s in enumerate(ks) if s <= 0.6 * tr["n_steps"]]
    e_early, e_all = np.abs(P[ks][early] - want[early]).max(), np.abs(P[ks] - want).max()
    print(f"{name} on its own times: {res['n_unique'][0]} states, error {e_early:.3e} over the first 60 %, {e_all:.3e} everywhere")
    assert e_early < 5e-6
    assert e_all < 2e-2
    assert int(np.argmax(P[-1])) == int(np.argmax(want[-1]))
    assert P.min() > -1e-9 and np.allclose(P.sum(axis=1), 1.0)
    assert np.abs(res["pop"][1] - K.two_state_populations(-1.0, K.KT, times)).max() < 5e-6


# ---------------------------------------------------------------- 4. independence

def others():
    return [K.facing_graph(), K.star_graph(140), K.length_edge_graph(129)]


@pytest.mark.parametrize("which", ["lds_68_states", "global_257_states"])
def test_gpu_batch_result_does_not_depend_on_the_batch(which):
    """alone, first of four, last of four, and with every graph in a workspace chunk of its own (workspace_bytes=1): the same bits"""
    graph = utils.parse_rafft_output(os.path.join(GOLD, "example_rafft_20.out"))[0] if which.startswith("lds") else K.star_graph(257, -3.05)
    alone = call([graph], FEW_TIMES, rates=True)
    assert alone["status"] == [N.OK] and alone["n_unique"][0] == int(which.split("_")[1])
    for label, graphs, at, ws in (("first", [graph] + others(), 0, 0), ("last", others() + [graph], 3, 0),
                                  ("first, chunked", [graph] + others(), 0, 1), ("last, chunked", others() + [graph], 3, 1)):
        res = call(graphs, FEW_TIMES, rates=True, workspace_bytes=ws)
        assert res["status"] == [N.OK] * 4, label
        assert np.array_equal(res["pop"][at], alone["pop"][0]), label
        assert np.array_equal(res["rate"][at], alone["rate"][0]) and res["n_edges"][at] == alone["n_edges"][0], label
        assert np.array_equal(res["uid"][at], alone["uid"][0]), label
    chunked, whole = call(others(), FEW_TIMES, workspace_bytes=1), call(others(), FEW_TIMES)
    assert all(np.array_equal(a, b) for a, b in zip(chunked["pop"], whole["pop"]))


# ---------------------------------------------------------------- 5. errors are local

def neighbours():
    if "neighbours" not in _cache:
        pair = [K.length_edge_graph(66), K.star_graph(200)]
        _cache["neighbours"] = (pair, call(pair, FEW_TIMES))
    return _cache["neighbours"]


def check_neighbours(res, code, word):
    pair, base = neighbours()
    assert res["status"] == [N.OK, code, N.OK]
    assert word in res["error"] and "graph 1" in res["error"]
    assert res["pop"][1] is None and (res["uid"][1] == -1).all()
    for at, k in ((0, 0), (2, 1)):
        assert np.array_equal(res["pop"][at], base["pop"][k]) and np.array_equal(res["uid"][at], base["uid"][k])
        assert (res["n_unique"][at], res["n_edges"][at]) == (base["n_unique"][k], base["n_edges"][k])


@pytest.mark.parametrize("name", list(MALFORMED))
def test_gpu_batch_malformed_graph_fails_alone(name):
    pair, _ = neighbours()
    check_neighbours(call([pair[0], MALFORMED[name], pair[1]], FEW_TIMES), N.ERR_STRUCT, "malformed")


def test_gpu_batch_graph_over_the_cap_fails_alone():
    pair, _ = neighbours()
    res = call([pair[0], K.star_graph(N.KIN_BATCH_MAX_STATES + 1), pair[1]], FEW_TIMES)
    check_neighbours(res, N.ERR_CAPACITY, "single-graph")
    assert res["n_unique"][1] == N.KIN_BATCH_MAX_STATES + 1
    at_cap = call([K.star_graph(N.KIN_BATCH_MAX_STATES)], FEW_TIMES[:2], substeps=1)          # the cap itself is solved
    assert at_cap["status"] == [N.OK] and np.allclose(at_cap["pop"][0].sum(axis=1), 1.0)


def test_gpu_kinetics_batch_keeps_the_other_graphs_when_one_fails():
    """kinetics_batch: the graph over the cap goes through kinetics_gpu(method="implicit"), the malformed one gives None, the two
    good graphs keep the bits of a batch without them, and a warning carries the library's message"""
    pair, _ = neighbours()
    max_time, n_steps, m = 10, 4, 2
    base = rafft_kin.kinetics_batch(pair, max_time, n_steps, substeps=m)
    over = K.star_graph(N.KIN_BATCH_MAX_STATES + 1)
    with pytest.warns(RuntimeWarning, match="single-graph"):
        got = rafft_kin.kinetics_batch([pair[0], over, next(iter(MALFORMED.values())), pair[1]], max_time, n_steps, substeps=m)
    assert got[2] is None
    for at, k in ((0, 0), (3, 1)):
        assert np.array_equal(np.array(got[at][0]), np.array(base[k][0])) and got[at][3] == base[k][3]
    one = rafft_kin.kinetics_gpu(over, max_time, n_steps, method="implicit", substeps=m)
    assert len(got[1][2]) == N.KIN_BATCH_MAX_STATES + 1 and got[1][1] == one[1]
    assert np.array_equal(np.array(got[1][0]), np.array(one[0]))


def bad_calls():
    good = arrays(K.length_edge_graph(66))
    L, sizes, rows, stride, en = good
    neg = sizes.copy()
    neg[1] = -1
    sched = lambda m, h: (FEW_TIMES, [m] + [4] * 5, [h] + [1.0] * 5)
    return {"kt_0": dict(kt=0.0), "kt_nan": dict(kt=float("nan")),
            "times_descend": dict(times=FEW_TIMES[::-1]), "times_repeat": dict(times=np.array([1.0, 1.0])), "time_0": dict(times=np.array([0.0, 1.0])),
            "no_times": dict(times=np.zeros(0)),
            "m_0": dict(schedule=sched(0, 1.0)), "h_0": dict(schedule=sched(4, 0.0)), "h_negative": dict(schedule=sched(4, -1.0)),
            "length_32768": dict(graph=(32768, np.zeros(0, np.int32), b"", 32768, np.zeros(0))),
            "stride_below_length": dict(graph=(L, sizes, rows, L - 1, en)),
            "negative_step_size": dict(graph=(L, neg, rows, stride, en[:int(neg.sum())])),
            "negative_budget": dict(workspace_bytes=-1)}


@pytest.mark.parametrize("what", list(bad_calls()))
def test_gpu_batch_bad_argument_is_refused(what):
    kw = bad_calls()[what]
    pair, base = neighbours()
    graphs = [arrays(pair[0]), kw.pop("graph", arrays(pair[1]))]
    times = kw.pop("times", FEW_TIMES)
    with pytest.raises(N.RafftError) as err:
        rafft_kin.kin_batch_call(graphs, times, kw.pop("kt", K.KT), 4, **kw)
    assert err.value.code == N.ERR_PARAM
    again = call(pair, FEW_TIMES)
    assert all(np.array_equal(a, b) for a, b in zip(again["pop"], base["pop"]))


# ---------------------------------------------------------------- 6. end to end

def test_gpu_fold_then_kinetics_batch_end_to_end(tmp_path):
    import rafft_amd
    rng = np.random.default_rng(6)
    seqs = ["GGGGCGCAAAAGCGCCCCAU"] + ["".join(rng.choice(list("ACGU"), n)) for n in (35, 50, 65, 80)]
    max_time, n_steps, coarse = 30, 20, 8
    folded = rafft_amd.fold_batch(seqs, max_stack=5, traj=True)
    got = rafft_amd.kinetics_batch(folded, max_time, n_steps)
    parsed = []
    for k, s in enumerate(seqs):                                   # the same graphs through the text format
        path = tmp_path / f"g{k}.out"
        with open(path, "wb") as fh:
            utils.write_result_text(fh, s, folded.raw(k), traj=True)
        fp, seq = utils.parse_rafft_output(str(path))
        assert seq == s
        parsed.append(fp)
    from_text = rafft_amd.kinetics_batch(parsed, max_time, n_steps)
    # (against the per-graph route with 8 sub-steps per e^0.3 on both sides: its host solves are what this test's time goes to)
    got8 = rafft_amd.kinetics_batch(folded, max_time, n_steps, substeps=coarse)
    early = int(0.6 * n_steps) + 1
    for k in range(len(seqs)):
        traj, times, sl, eq = got[k]
        traj2, times2, sl2, eq2 = from_text[k]
        assert np.array_equal(np.array(traj), np.array(traj2)) and times == times2
        assert [(s.str_struct, s.energy) for s in sl] == [(s.str_struct, s.energy) for s in sl2] and eq == eq2
        one, t1, sl1, eq1 = rafft_kin.kinetics_gpu(parsed[k], max_time, n_steps, method="implicit", substeps=coarse)
        assert [s.str_struct for s in sl1] == [s.str_struct for s in sl]
        np.testing.assert_allclose(np.array(times, dtype=float), np.array(t1, dtype=float), rtol=0, atol=0)
        d = np.abs(np.array(got8[k][0]) - np.array(one))
        print(f"sequence {k}: {len(sl)} states, against kinetics_gpu {d[:early].max():.3e} early, {d.max():.3e} overall")
        assert d[:early].max() < 5e-6 and d.max() < 2e-2
    fa, out = tmp_path / "s.fa", tmp_path / "kin.txt"
    fa.write_text("".join(f">s{k}\n{s}\n" for k, s in enumerate(seqs)))
    cli.main(["-sf", str(fa), "--batch", "-ms", "5", "--kin", str(out), "-mt", str(max_time), "-ns", str(n_steps)])
    blocks = out.read_text().split("> ")[1:]
    assert len(blocks) == len(seqs)
    for k, block in enumerate(blocks):
        lines = block.splitlines()
        assert lines[0] == f"{k} {seqs[k]}" and len(lines) - 1 == len(got[k][2])
        want = sorted(got[k][3], key=lambda el: el[2])
        assert lines[1:] == ["{} {:6.3f} {:5.1f} {:d}".format(st, fp, nrj, si) for st, nrj, fp, si in want]
