"""rafft_kinfold_batch on a real MI355X (`-m gpu`): on a slice of the starts of tests/_descend_np.py every trajectory is, bit for bit,
that of the tests' own restatement (tests/_kinfold_np.py: whole-structure oracle energies, brute-force neighbours, its own Philox) -
end row, steps, flags, stop index, energies, every move, every sample record; the times agree to the last places of a logarithm -
under the built-in tables and an index-sensitive set; at 60-120, 300 and 1000 nt every row of every logged path evaluates back
(eval_kernel) and on sampled steps the sum of the weights and the move are those of neighbours generated a third way; 20 000
trajectories a sequence against the exact master equation on the full enumeration, occupancy, survival and equilibrium, judged
by _sample_stats (no tolerance to tune); the edges of the definition; same input - same bits across batch position, order,
duplicates, chunking, logs and strides; errors that stay with their item; other temperatures; the command line."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from rafft_amd import _native as N, kinfold as KFm, findpath as FPm, mccaskill, params, rafft as R, zuker
from conftest import ROOT
import _descend_np as DS
from _descend_np import all_neighbours, move_row
import _kinfold_np as KF
import _loops as LP
import _par_reader as PR
import _sample_stats as SS

pytestmark = pytest.mark.gpu

GRID = [3.7, 41.3, 171.3, 433.7]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    out = dict(builtin=builtin, index=LP.index_sensitive_par(builtin), synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name in ("index", "synthetic"):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=name)
    return out


def install(sets, which):
    if which == "builtin":
        params.reset_params()
        oracle.reset_tables()
    else:
        params.load_params(sets["paths"][which])
        oracle.set_tables(PR.tables_at(sets[which], 37.0))


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()
    oracle.reset_tables()


def rand(rng, n, letters="ACGU"):
    return "".join(rng.choice(list(letters), n))


def run(seqs, rows, t_max, **kw):
    """per sequence a list of trajectories as dicts in the shape of the mirror's"""
    log = kw.pop("log", True)
    srec, trec, ends, samples, mv, tm = KFm.kinfold_batch_raw(list(seqs), rows, t_max, log=log, **kw)
    out = []
    for s in range(len(seqs)):
        rws = KFm.end_rows(ends[s], srec[s]["length"])
        out.append([dict(seq_status=srec[s]["status"], status=int(t["status"]), flags=int(t["flags"]), n_steps=int(t["n_steps"]),
                         start_dcal=int(t["start_dcal"]), end_dcal=int(t["end_dcal"]), stop_index=int(t["stop_index"]), time=float(t["time"]),
                         end=rws[k], samples=[tuple(x) for x in samples[s][k].tolist()],
                         moves=[tuple(m) for m in mv[s][k].tolist()] if log else None, times=tm[s][k].tolist() if log else None)
                    for k, t in enumerate(trec[s])])
    return out


EXACT = ("status", "flags", "n_steps", "start_dcal", "end_dcal", "stop_index", "end", "moves", "samples")


def same_as_mirror(got, want, what):
    assert want["near"] == 0, what
    for f in EXACT:
        assert got[f] == want[f], (what, f, got[f], want[f])
    # a time is a sum of n_steps terms, each a logarithm of the device (the last place may differ from math.log's) times exact
    # factors: relative 1e-12 a step holds 4500 ulp a step
    tol = 1e-12 * max(want["n_steps"], 1)
    assert len(got["times"]) == len(want["times"])
    for a, b in zip(got["times"] + [got["time"]], want["times"] + [want["time"]]):
        assert abs(a - b) <= tol * abs(b), (what, a, b)


def watch_of(rows, en):
    """the watched rows of an enumeration in the tests: the MFE row (the stop row), the open chain, three more"""
    mfe = int(np.argmin(en))
    return [rows[mfe], "." * len(rows[0])] + [rows[k] for k in (len(rows) // 3, len(rows) // 2, len(rows) - 1) if k != mfe]


# ---- 1. bit equality with the restatement

@pytest.mark.parametrize("which", ["builtin", "index"])
def test_trajectories_are_the_restatements_bit_for_bit(sets, which):
    install(sets, which)
    W = KFm.kinfold_weights()
    M = KF.Mirror(W)
    grid = GRID if which == "builtin" else GRID[:3]         # (the index-sensitive set moves faster: the same steps in less time)
    seqs, rows, watch, want = [], [], [], []
    for s, (seq, all_rows) in enumerate(DS.start_sequences()):
        w = watch_of(all_rows, [M.energy(seq, r) for r in all_rows])
        picks = all_rows[s % 13::13]
        seqs.append(seq); rows.append(picks); watch.append(w)
        want.append([M.trajectory(seq, r, k * 2 + rep, 4242 + s, grid[-1], 1000, w, 1, grid) for k, r in enumerate(picks) for rep in range(2)])
    n = sum(len(w) for w in want)
    steps = [t["n_steps"] for w in want for t in w]
    print(f"\n{which}: {n} trajectories, {sum(steps) / n:.1f} steps each, {max(steps)} at most, "
          f"{sum(t['flags'] == KF.KF_STOP for w in want for t in w)} arrive, near {sum(t['near'] for w in want for t in w)}")
    assert 500 <= n <= 700 and 15 <= sum(steps) / n <= 80
    assert {t["flags"] for w in want for t in w} == {KF.KF_STOP, KF.KF_TIME}
    got = run(seqs, rows, grid[-1], n_rep=2, watch=watch, n_stop=1, seeds=[4242 + s for s in range(len(seqs))], sample_times=grid, max_steps=1000)
    for s in range(len(seqs)):
        assert len(got[s]) == len(want[s])
        for k, (g, w) in enumerate(zip(got[s], want[s])):
            same_as_mirror(g, w, (which, s, k))
    cnt = (ctypes.c_longlong * 4)()
    assert N.lib().rafft_kinfold_counters(ctypes.byref(cnt)) == 0 and list(cnt) == [1, 1, n, sum(steps)]


# ---- 2. larger sizes: the same equality where the restatement is affordable, and what can be checked beyond it

def path_checks(items, W, seed_of, sampled_steps=3, temp=37.0, seed=5):
    """items: (seq, start row, k, trajectory).  Every row of every logged path evaluates back with the running energy; on up to
    `sampled_steps` steps per trajectory the sum of the weights (through the jump time) and the move are what the neighbours of
    all_neighbours give, energies from rafft_eval_structures.  One eval call."""
    rng = np.random.default_rng(seed)
    q_seq, q_row, plan = [], [], []

    def ask(seq, row):
        q_seq.append(seq)
        q_row.append(row)
        return len(q_row) - 1

    for seq, row, k, g in items:
        assert len(g["moves"]) == g["n_steps"]
        path = FPm.path_rows(row, np.array(g["moves"], dtype=np.int64).reshape(-1, 2))
        assert path[-1] == g["end"]
        at = [ask(seq, r) for r in path]
        look = sorted(set(rng.choice(g["n_steps"], min(sampled_steps, g["n_steps"]), replace=False).tolist())) if g["n_steps"] else []
        probes = []
        for t in look:
            nb = all_neighbours(seq, path[t])
            probes.append((t, nb, [ask(seq, move_row(path[t], i, j, rem)) for i, j, rem in nb]))
        plan.append((seq, k, g, at, probes))
    en, st = R.eval_structures(q_seq, q_row, temp=temp)
    assert not any(st)
    n_probes = 0
    for seq, k, g, at, probes in plan:
        run_e = [en[a] for a in at]
        assert run_e[0] == g["start_dcal"] and run_e[-1] == g["end_dcal"]
        for t, nb, idx in probes:
            w = [KF.weight(W, en[a] - run_e[t]) for a in idx]
            wtot = sum(w)
            o = KF.philox((seed_of & KF.MASK, seed_of >> 32), (k, t, 0, 0))
            u = float((o[0] << 32 | o[1]) >> 11) * 2.0 ** -53
            dt = -math.log(1.0 - u) * 4294967296.0 / float(wtot)
            before = g["times"][t - 1] if t else 0.0
            assert abs(g["times"][t] - (before + dt)) <= 1e-12 * (t + 1) * g["times"][t], (seq, k, t)
            r = ((o[2] << 32 | o[3]) * wtot) >> 64
            acc = 0
            for (i, j, rem), wi in zip(nb, w):
                acc += wi
                if acc > r:
                    break
            assert g["moves"][t] == ((-i - 1, -j - 1) if rem else (i, j)), (seq, k, t)
            n_probes += 1
    return n_probes


def test_longer_sequences_equal_the_restatement_and_evaluate_back():
    rng = np.random.default_rng(20261101)
    seqs = [rand(rng, n) for n in (60, 77, 96, 120)]
    sampled = mccaskill.sample_batch(seqs, 2, seeds=11)
    rows = [[None] + [st.str_struct for st in sm] for sm in sampled]
    mfe = [m.str_struct for m in zuker.mfe_batch(seqs)]
    W = KFm.kinfold_weights()
    t_max = 20.9173
    grid = [0.0713, 0.9177, 20.9173]
    got = run(seqs, rows, t_max, n_rep=2, watch=[[m, "." * len(s)] for m, s in zip(mfe, seqs)], n_stop=1, seeds=77, sample_times=grid, max_steps=600)
    M = KF.Mirror(W)
    items = []
    for s, seq in enumerate(seqs):
        for k, g in enumerate(got[s]):
            row = rows[s][k // 2] or "." * len(seq)
            items.append((seq, row, k, g))
            same_as_mirror(g, M.trajectory(seq, row, k, 77, t_max, 600, [mfe[s], "." * len(seq)], 1, grid), (seq, k))
    steps = [g["n_steps"] for _, _, _, g in items]
    print(f"\n{len(items)} trajectories, {sum(steps)} steps, {max(steps)} at most")
    assert all(g["status"] == 0 for _, _, _, g in items) and sum(steps) >= 10 * len(items)
    assert path_checks(items, W, 77) >= 2 * len(items)


@pytest.mark.parametrize("L", DS.STRIDE_LENGTHS)
def test_lengths_where_the_lanes_stride(L):
    """63, 64, 65 and 129 positions, where a lane's share x = lane, lane + 64, ... gains a position and the lane that owns the drawn
    position, xs & 63, is no longer xs: four trajectories of 32 steps from random rows, exactly the restatement's"""
    seq, rows = DS.stride_rows(L)
    watch, grid = [rows[2], "." * L], [1e-3, 1.0, 1e9]
    M = KF.Mirror(KFm.kinfold_weights())
    want = [M.trajectory(seq, r, k, 900 + L, 1e9, 32, watch, 0, grid) for k, r in enumerate(rows)]
    assert all(w["n_steps"] == 32 and w["flags"] == KF.KF_MORE for w in want)
    top = max(max(-a - 1 if a < 0 else a, -b - 1 if b < 0 else b) for w in want for a, b in w["moves"])
    assert top >= (64 if L == 129 else L - 4), top            # (moves reach the last positions, those of the second share at 129)
    got = run([seq], [rows], 1e9, watch=[watch], n_stop=0, seeds=[900 + L], sample_times=grid, max_steps=32)[0]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        same_as_mirror(g, w, (L, k))


def test_300_and_1000_nt():
    """300 nt from the open chain (several positions a lane, a scan beyond 64 entries), 1000 nt from its MFE row (the loops of a
    folded row keep the neighbours of the three probed steps affordable): 200 steps each, the bound ends them"""
    rng = np.random.default_rng(20261102)
    seqs = [rand(rng, 300), rand(rng, 1000)]
    starts = ["." * 300, zuker.mfe_batch(seqs[1:])[0].str_struct]
    W = KFm.kinfold_weights()
    got = run(seqs, [[r] for r in starts], 1e9, seeds=[5, 6], max_steps=200, sample_times=[1e-5, 1e9])
    items = []
    for s, seq in enumerate(seqs):
        g = got[s][0]
        assert g["flags"] == KF.KF_MORE and g["status"] == N.ERR_CAPACITY and g["n_steps"] == 200 and g["time"] == g["times"][-1] < 1e9
        assert g["samples"][1] == KF.INVALID and g["samples"][0][1] == -1
        assert all(a < b for a, b in zip(g["times"], g["times"][1:]))
        n_before = sum(1 for T in g["times"] if T <= 1e-5)
        items.append((seq, starts[s], 0, g))
        path = FPm.path_rows(starts[s], np.array(g["moves"][:n_before], dtype=np.int64).reshape(-1, 2))
        en, st = R.eval_structures([seq], [path[-1]])
        assert g["samples"][0][0] == en[0]
    assert path_checks(items[:1], W, 5) == 3 and path_checks(items[1:], W, 6) == 3


# ---- 3. statistics against the exact master equation

STAT_TIMES = [2.3, 11.7, 53.9, 247.1, 1131.7, 5179.3]
N_STAT = 20000


@pytest.mark.parametrize("case", [0, 1])
def test_occupancy_survival_and_equilibrium_against_the_master_equation(case):
    seq, rows = [(s, r) for s, r in DS.start_sequences() if len(r) <= 300][case]
    W = KFm.kinfold_weights()
    en, st = R.eval_structures([seq] * len(rows), rows)
    assert not any(st)
    Q, en2 = KF.generator(seq, rows, W, energy=lambda s, r: en[rows.index(r)])
    assert en2 == list(en)
    boltz = np.exp(-(np.array(en) - min(en)) / (100.0 * KF.GAS * 310.15))
    boltz /= boltz.sum()
    mfe = int(np.argmin(en))
    # a start that is no minimum: the row with the highest energy
    for start in ("." * len(seq), rows[int(np.argmax(en))]):
        p0 = np.zeros(len(rows))
        p0[rows.index(start)] = 1.0
        P = np.clip(KF.propagate(Q, p0, STAT_TIMES), 0.0, 1.0)
        assert np.abs(P[-1] - boltz).max() < 1e-3           # the last time is equilibrium: the counts are checked against exp(-E/kT)/Z too
        top = np.argsort(-P[-1], kind="stable")[:63]
        watch = [rows[k] for k in top]
        counts = KFm.occupancy([seq], [start], [watch], N_STAT, STAT_TIMES, seeds=900 + case)[0]
        assert counts.shape == (len(STAT_TIMES), len(watch) + 1) and (counts.sum(axis=1) == N_STAT).all()
        want = np.concatenate([P[:, top], 1.0 - P[:, top].sum(axis=1, keepdims=True)], axis=1)
        bad = SS.misses(counts, N_STAT, np.clip(want, 0.0, 1.0))
        assert len(bad) == 0, (seq, start, bad, counts.ravel()[bad], (N_STAT * want).ravel()[bad])
        # survival: the MFE row absorbing
        Qa = Q.copy()
        Qa[:, mfe] = 0.0
        arrived = np.clip(KF.propagate(Qa, p0, STAT_TIMES)[:, mfe], 0.0, 1.0)
        times, missing = KFm.first_passage(seq, start, rows[mfe], N_STAT, STAT_TIMES[-1], seed=1900 + case)
        got = np.array([(times <= tau).sum() for tau in STAT_TIMES])
        assert abs((1.0 - missing) * N_STAT - got[-1]) < 0.5
        assert len(SS.misses(got, N_STAT, arrived)) == 0, (seq, start, got, N_STAT * arrived)


# ---- 4. the edges of the definition

def one(seq, row, t_max, **kw):
    kw.setdefault("seeds", 3)
    return run([seq], [[row]], t_max, **kw)[0][0]


def test_edges_of_the_process(sets):
    # nothing can pair: absorbed at once, the time is t_max
    for seq in ("A", "GC", "GAC", "GAAC", "A" * 40, "N" * 12, "GGGGNNNNNNNN"):
        g = one(seq, None, 7.5, sample_times=[0.0, 7.5])
        assert (g["flags"], g["n_steps"], g["time"], g["end"], g["stop_index"]) == (KF.KF_ABSORBED, 0, 7.5, "." * len(seq), -1), seq
        assert g["samples"] == [(0, -1)] * 2
    seq = "GGGGAAAACCCC"
    M = KF.Mirror(KFm.kinfold_weights())
    # t_max = 0: no step unless u is 0
    g = one(seq, None, 0.0, sample_times=[0.0])
    assert (g["flags"], g["n_steps"], g["time"]) == (KF.KF_TIME, 0, 0.0) and g["samples"] == [(0, -1)]
    # a start that is a stop row; the second of two stop rows, reached by its index; watched rows that are not stop rows do not end it
    hp = "((((....))))"
    g = one(seq, hp, 5.0, watch=[["." * 12, hp]], n_stop=2, sample_times=[1.0])
    assert (g["flags"], g["n_steps"], g["time"], g["stop_index"], g["end"]) == (KF.KF_STOP, 0, 0.0, 1, hp) and g["samples"] == [(M.energy(seq, hp), 1)]
    stops = ["(((......)))", ".(((....))).", hp]
    got = run([seq], [[None]], 400.0, n_rep=64, watch=[stops], n_stop=2, seeds=8, sample_times=[0.5, 400.0], max_steps=4000)[0]
    for k, g in enumerate(got):
        same_as_mirror(g, M.trajectory(seq, "." * 12, k, 8, 400.0, 4000, stops, 2, [0.5, 400.0]), k)
    assert {g["stop_index"] for g in got} - {-1} == {0, 1} and all(g["end"] == stops[g["stop_index"]] for g in got if g["flags"] == KF.KF_STOP)
    assert any(g["samples"][0][1] == -1 for g in got)
    # 64 watched rows, the last one the state; none; no sample times
    many = [move_row("." * 12, i, j, False) for i in range(12) for j in range(i + 4, 12) if seq[i] + seq[j] in DS.CANONICAL]
    many = (many * 4)[:63] + [hp]
    g = one(seq, hp, 0.01, watch=[many], n_stop=0, sample_times=[0.0])
    assert g["samples"] == [(M.energy(seq, hp), 63)] and g["flags"] == KF.KF_TIME
    g0 = one(seq, None, 30.0, max_steps=500)
    gw = one(seq, None, 30.0, max_steps=500, watch=[many], n_stop=0, sample_times=[1.1, 29.3])
    assert g0["samples"] == [] and all(g0[f] == gw[f] for f in EXACT if f != "samples") and g0["times"] == gw["times"]
    same_as_mirror(gw, M.trajectory(seq, "." * 12, 0, 3, 30.0, 500, many, 0, [1.1, 29.3]), "64 watched")
    # max_steps = 3: CAPACITY, the later samples invalid, the neighbours untouched
    alone = run([seq], [[None, hp]], 1e5, seeds=3, sample_times=[1e-3, 1e5], max_steps=3000)[0]
    three = run([seq, seq], [[None, hp], [None]], 1e5, seeds=3, sample_times=[1e-3, 1e5], max_steps=3)
    for g in three[0] + three[1]:
        assert (g["flags"], g["status"], g["n_steps"]) == (KF.KF_MORE, N.ERR_CAPACITY, 3) and g["samples"][1] == KF.INVALID and g["time"] == g["times"][2]
    assert three[0][0]["moves"] == alone[0]["moves"][:3] and three[0][1]["times"] == alone[1]["times"][:3] and three[1][0] == three[0][0]
    assert "trajectory 0: not ended after 3 steps" in N.lib().rafft_last_error().decode()
    with pytest.raises(N.RafftError, match="max_steps"):
        KFm.kinfold_batch([seq], [[None]], 1e5, max_steps=3)
    # a kt at which every uphill move has weight 0: from the open chain of a sequence whose every first pair costs energy, absorbed
    g = one(seq, None, 50.0, kt=1e-4)
    assert g["flags"] == KF.KF_ABSORBED and g["n_steps"] == 0 and M.moves(seq, "." * 12) and min(c[4] for c in M.moves(seq, "." * 12)) > 0
    cold = KF.Mirror(KFm.kinfold_weights(37.0, 1e-4))
    same_as_mirror(one(seq, "(((......)))", 50.0, kt=1e-4, max_steps=50), cold.trajectory(seq, "(((......)))", 0, 3, 50.0, 50), "cold")
    hot = KF.Mirror(KFm.kinfold_weights(37.0, 2.5))
    same_as_mirror(one(seq, None, 20.0, kt=2.5, max_steps=500), hot.trajectory(seq, "." * 12, 0, 3, 20.0, 500), "hot")


def test_loops_of_every_kind_on_the_way(sets):
    """a lonely pair removed, a multiloop closing and opening, a hairpin of 34, interior loops above 30, N bases: constructed starts,
    short trajectories, equal to the restatement"""
    M = KF.Mirror(KFm.kinfold_weights())
    hp = "GGGAAAACCC"
    ml = "GGGA" + hp + "A" + hp + "ACCC"
    cases = [("GAAAAA" + hp + "AAAAAC", "(....." + "(((....)))" + ".....)", 300.0),                 # a lonely pair around a helix
             (ml, "...." + "(((....)))" + "." + "(((....)))" + "....", 300.0), (ml, "(((." + "(((....)))" + "." + "(((....)))" + ".)))", 300.0),
             ("GGG" + "A" * 34 + "CCC", "(((" + "." * 34 + ")))", 300.0),
             ("GG" + "A" * 17 + "GGGAAAACCC" + "A" * 16 + "CC", "((" + "." * 17 + "(((....)))" + "." * 16 + "))", 300.0),
             ("GGNGAANACNCC", "((.(....).))", 6.0), ("NGGGAAAACCCN", None, 40.0)]
    seqs = [c[0] for c in cases]
    assert all(r is None or DS.parse_status(s, r) == 0 for s, r, _ in cases)
    kinds = set()
    for s, (seq, row, t_max) in enumerate(cases):
        got = run([seq], [[row]], t_max, n_rep=6, seeds=31 + s, max_steps=300, sample_times=[t_max * 0.37])[0]
        for k, g in enumerate(got):
            same_as_mirror(g, M.trajectory(seq, row or "." * len(seq), k, 31 + s, t_max, 300, grid=[t_max * 0.37]), (seq, k))
            kinds |= {m[0] < 0 for m in g["moves"]}
        assert sum(g["n_steps"] for g in got) >= 20, seq
        if s == 1:          # the multiloop closes in some of them ... and in the next case it opens and closes again
            assert any(g["end"].startswith("((") for g in got)
    assert kinds == {True, False}


def test_other_temperatures_with_a_loaded_parameter_file(sets):
    params.load_params(sets["paths"]["synthetic"])
    seq, rows = DS.start_sequences()[0]
    ends = {}
    for temp in (25.0, 60.0):
        oracle.set_tables(PR.tables_at(sets["synthetic"], temp))
        W = KFm.kinfold_weights(temp)
        assert max(abs(int(a) - b) for a, b in zip(W, KF.formula_weights(KF.GAS * (temp + 273.15)))) <= 1
        M = KF.Mirror(W)
        got = run([seq], [rows[::29]], 120.0, n_rep=2, seeds=61, temp=temp, max_steps=400, sample_times=[13.7])[0]
        for k, g in enumerate(got):
            same_as_mirror(g, M.trajectory(seq, rows[::29][k // 2], k, 61, 120.0, 400, grid=[13.7]), (temp, k))
        ends[temp] = [(g["end"], g["n_steps"]) for g in got]
    assert ends[25.0] != ends[60.0]


# ---- 5. same input, same bits; errors stay with their item

def test_same_input_same_bits():
    groups = DS.start_sequences()[:3]
    seqs = [g[0] for g in groups]
    rows = [g[1][3::41] for g in groups]
    watch = [g[1][:2] for g in groups]
    kw = dict(n_rep=3, watch=watch, n_stop=1, seeds=[5, 6, 7], sample_times=[7.7, 99.1], max_steps=300)
    base = run(seqs, rows, 99.1, **kw)
    assert sum(len(b) for b in base) > 30 and any(g["n_steps"] > 10 for b in base for g in b)
    # alone, reversed, duplicated with equal seeds
    for s in range(3):
        assert run(seqs[s:s + 1], rows[s:s + 1], 99.1, **dict(kw, watch=watch[s:s + 1], seeds=[5 + s]))[0] == base[s]
    assert run(seqs[::-1], rows[::-1], 99.1, **dict(kw, watch=watch[::-1], seeds=[7, 6, 5]))[::-1] == base
    twice = run(seqs + seqs, rows + rows, 99.1, **dict(kw, watch=watch + watch, seeds=[5, 6, 7] * 2))
    assert twice[:3] == base and twice[3:] == base
    # one trajectory per chunk
    assert run(seqs, rows, 99.1, workspace_bytes=1, **kw) == base
    cnt = (ctypes.c_longlong * 4)()
    N.lib().rafft_kinfold_counters(ctypes.byref(cnt))
    n = sum(len(b) for b in base)
    assert list(cnt) == [n, n, n, sum(g["n_steps"] for b in base for g in b)]
    # without logs; logs for one sequence only; a stride of L + 1
    strip = lambda b: [[dict(g, moves=None, times=None) for g in per] for per in b]
    assert run(seqs, rows, 99.1, log=False, **kw) == strip(base)
    arr = [np.frombuffer(b"".join(r.encode() + b"\0" for r in rws), dtype=np.uint8).reshape(len(rws), -1) for rws in rows]
    assert all(a.shape[1] == len(s) + 1 for a, s in zip(arr, seqs)) and run(seqs, arr, 99.1, **kw) == base
    L = N.lib()
    enc, sarr, lens = N.seq_arrays(seqs)
    blocks = [KFm._row_block(r, len(s))[0] for r, s in zip(rows, seqs)]
    wblocks = [KFm._row_block(w, len(s))[0] for w, s in zip(watch, seqs)]
    n_traj = [3 * len(r) for r in rows]
    ends = [np.zeros((n_traj[s], len(seqs[s]) + 1), dtype=np.uint8) for s in range(3)]
    smp = [np.zeros((n_traj[s], 2, 2), dtype=np.int32) for s in range(3)]
    mv1, tm1 = np.zeros((n_traj[1], 300, 2), dtype=np.int32), np.zeros((n_traj[1], 300), dtype=np.float64)
    srec, trec = (N.KinfoldSeq * 3)(), np.zeros(sum(n_traj), dtype=KFm.TRAJ_DTYPE)
    ints = lambda v: (ctypes.c_int * 3)(*v)
    voids = lambda v: (ctypes.c_void_p * 3)(*[a if a is None else a.ctypes.data for a in v])
    grid = (ctypes.c_double * 2)(7.7, 99.1)
    assert L.rafft_kinfold_batch(3, sarr, lens, ints([len(r) for r in rows]), voids(blocks), ints([len(s) for s in seqs]), 3, ints([2] * 3), ints([1] * 3),
                                 voids(wblocks), ints([len(s) for s in seqs]), (ctypes.c_ulonglong * 3)(5, 6, 7), 37.0, 0.0, 99.1, 300, 2, grid, 0, srec,
                                 trec.ctypes.data, voids(ends), voids(smp), voids([None, mv1, None]), voids([None, tm1, None])) == 0
    for s in range(3):
        part = trec[srec[s].traj0:srec[s].traj0 + srec[s].n_traj]
        assert part["n_steps"].tolist() == [g["n_steps"] for g in base[s]] and part["time"].tolist() == [g["time"] for g in base[s]]
        assert KFm.end_rows(ends[s], len(seqs[s])) == [g["end"] for g in base[s]] and smp[s].tolist() == [[list(x) for x in g["samples"]] for g in base[s]]
    for k, g in enumerate(base[1]):
        assert [tuple(m) for m in mv1[k, :g["n_steps"]].tolist()] == g["moves"] and tm1[k, :g["n_steps"]].tolist() == g["times"]
    # the first n trajectories of n_rep = m > n are those of n_rep = n, for one start row
    five = run(seqs[:1], [rows[0][:1]], 99.1, **dict(kw, n_rep=5, watch=watch[:1], seeds=[5]))[0]
    assert five[:3] == base[0][:3] and len(five) == 5 and five[3] != five[4]


def test_errors_stay_with_their_item():
    good, rows = DS.start_sequences()[0]
    target = rows[len(rows) // 2]
    seqs = [good, "", good, "GGGTAAAACCC", good, "A" * 4097, good]
    start = [[rows[3]], [None], [rows[3], rows[3][:-1], rows[3]], [None], [rows[3]], [None], [rows[3]]]
    watch = [[target], [], [target], [], [target, "(" + "." * (len(good) - 1)], [], [target]]
    got = run(seqs, start, 50.0, n_rep=2, watch=watch, n_stop=[1, 0, 1, 0, 1, 0, 1], seeds=12, sample_times=[5.5], max_steps=6)
    ref = got[0]
    assert [g["seq_status"] for per in got for g in per[:1]] == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, N.ERR_STRUCT, N.ERR_TOO_LONG, 0]
    assert got[6] == ref and got[2][:2] == ref and len(ref) == 2
    assert [g["status"] for g in got[2][2:4]] == [N.ERR_STRUCT] * 2 and [g["end"] for g in got[2][2:4]] == [rows[3][:-1] + "\0"] * 2      # (as it went in: its NUL where the row ended)
    # trajectories 4 and 5 of the sequence start from its third row: their numbers, not the first row's
    M = KF.Mirror(KFm.kinfold_weights())
    for k in (4, 5):
        same_as_mirror(got[2][k], M.trajectory(good, rows[3], k, 12, 50.0, 6, [target], 1, [5.5]), k)
    assert {g["status"] for g in ref + got[2][4:]} <= {0, N.ERR_CAPACITY} and N.ERR_CAPACITY in {g["status"] for g in ref + got[2][4:]}
    assert all(g["status"] == N.ERR_STRUCT and g["end"] == "." * len(good) and g["samples"] == [KF.INVALID] for g in got[4])
    # the first erroneous item in input order is the call's error text: here the first trajectory, which the bound ended
    assert ref[0]["status"] == N.ERR_CAPACITY and N.lib().rafft_last_error().decode().startswith("sequence 0 trajectory 0: not ended after 6 steps")
    run(seqs[1:], start[1:], 50.0, n_rep=2, watch=watch[1:], n_stop=[0, 1, 0, 1, 0, 1], seeds=12, sample_times=[5.5], max_steps=6)
    assert N.lib().rafft_last_error().decode().startswith("sequence 0: empty")


# ---- 6. the command line

def test_command_line_as_a_process(tmp_path):
    groups = DS.start_sequences()[:2]
    seqs = [g[0] for g in groups]
    f = tmp_path / "seqs.fa"
    f.write_text(f">first\n{seqs[0]}\n>second\n{seqs[1]}\n")          # (names are a CSV's: a FASTA's are not printed)
    exe = [sys.executable, os.path.join(ROOT, "bin", "rafft")]
    r = subprocess.run(exe + ["-sf", str(f), "--batch", "--kinfold", "200", "--tmax", "500", "--stop", "mfe", "--times", "4", "--seed", "9"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    mfe = [m.str_struct for m in zuker.mfe_batch(seqs)]
    lines = r.stdout.splitlines()
    blocks = [lines[:len(lines) // 2], lines[len(lines) // 2:]]
    for s, b in enumerate(blocks):
        times, missing = KFm.first_passage(seqs[s], None, mfe[s], 200, 500.0, seed=9)
        assert len(b) == 7 and b[0] == seqs[s] and b[1].split()[0] == mfe[s]
        f3 = b[2].split()
        assert f3[0] == "arrived" and float(f3[1]) == pytest.approx(1.0 - missing, abs=5e-5)
        if len(times):
            assert float(f3[3]) == pytest.approx(float(np.median(times)), rel=1e-4) and float(f3[5]) == pytest.approx(float(times.mean()), rel=1e-4)
        table = [ln.split() for ln in b[3:]]
        assert len(table) == 4 and float(table[-1][0]) == pytest.approx(500.0) and all(len(t) == 3 for t in table)
        assert float(table[-1][2]) == pytest.approx(1.0 - missing, abs=5e-5)
    # a stop structure from a file; without --stop nothing arrives and the summary says so
    sf = tmp_path / "stop.txt"
    sf.write_text(mfe[0] + "\n")
    one = tmp_path / "one.fa"
    one.write_text(seqs[0] + "\n")
    r2 = subprocess.run(exe + ["-sf", str(one), "--batch", "--kinfold", "200", "--tmax", "500", "--stop", str(sf), "--seed", "9"], capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout.splitlines()[1:3] == blocks[0][1:3], r2.stderr
    r3 = subprocess.run(exe + ["-sf", str(one), "--batch", "--kinfold", "50", "--tmax", "5"], capture_output=True, text=True, timeout=120)
    assert r3.returncode == 0 and r3.stdout.splitlines()[1].split()[:2] == ["arrived", "0.0000"], r3.stderr
    r4 = subprocess.run(exe + ["-sf", str(one), "--batch", "--kinfold", "50", "--tmax", "1e6", "--max-steps", "2"], capture_output=True, text=True, timeout=120)
    assert r4.returncode != 0 and "max_steps" in r4.stderr
    r5 = subprocess.run(exe + ["-sf", str(one), "--batch", "--kinfold", "50"], capture_output=True, text=True, timeout=120)
    assert r5.returncode != 0 and "--tmax" in r5.stderr
