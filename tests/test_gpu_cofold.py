"""rafft_cofold_batch on a real MI355X (`-m gpu`): the minimum of the definition over every structure of
the host test's dimers, several times each in one batch mixed with single strands, under two table sets; the tests' mirror of the
recurrences - energy, row and n_inter - at 60-105 nt and on the 133- and 197-nt sequences of _lane_rounds cut near the middle,
where the 64-lane loops over the splits and the exterior loop, which span the dimer, are past their second round (the loops over
one strand end, FA and FB, are not: tests/test_gpu_cofold_edges.py); strands of one nt, the adjacent pair across the nick, a perfect duplex, strands
that cannot meet; swap symmetry; the same bytes in both size classes, per chunk, in another order and alone; the bytes of
rafft_mfe_batch without a cut; another DuplexInit and other temperatures; the limits of length; a bad cut; the command line.
Integers and bytes: no tolerance."""
import importlib

import numpy as np
import pytest

from rafft_amd import _native as N, cli, params, zuker
import rafft_amd
import _cofold_np as CF
import _lane_rounds as LR
import _loops as LP
import _par_reader as PR

cofold = importlib.import_module("rafft_amd.cofold")        # (the package's attribute `cofold` is the function)

pytestmark = pytest.mark.gpu

SEED = 1                        # of the drawn dimers, as tests/test_cofold_host.py
DINIT = 410


def par_of(which, **over):
    par = dict(LR.par_sets()[which])
    par.update(duplex_init=DINIT, duplex_init_dH=3 * DINIT + 70)
    par.update(over)
    return par


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("par")
    out = {}
    for name, par in (("multiloops_win", par_of("multiloops_win")), ("synthetic", par_of("synthetic", duplex_init=360, duplex_init_dH=900))):
        out[name] = d / (name + ".par")
        PR.write_par(par, out[name], comment=name)
    return out


def install(paths, which):
    if which == "builtin":
        params.reset_params()
    else:
        params.load_params(paths[which])


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()


_MIRROR = {}


def mirror(which, temp=37.0, dinit=DINIT):
    if (which, temp, dinit) not in _MIRROR:
        par = par_of("synthetic", duplex_init=360, duplex_init_dH=900) if which == "synthetic" else par_of(which)
        _MIRROR[which, temp, dinit] = CF.CutMirror(PR.tables_at(par, temp), dinit)
    return _MIRROR[which, temp, dinit]


def run(dimers, **kw):
    """cofold_batch_raw of a list of (seq, cut)"""
    return cofold.cofold_batch_raw([d[0] for d in dimers], [d[1] for d in dimers], **kw)


def swapped(dimers):
    return [(s[c:] + s[:c], len(s) - c) if c else (s, 0) for s, c in dimers]


def check_against_mirror(dimers, raw, m):
    rows, dcal, n_pairs, n_inter, cut, status = raw
    assert status == [0] * len(dimers) and cut == [c for _, c in dimers]
    for k, (s, c) in enumerate(dimers):
        want = m.fold_cut(s, c)
        assert (dcal[k], rows[k], n_inter[k]) == want and n_pairs[k] == rows[k].count("("), (k, s, c, rows[k], dcal[k], want)
        if c:
            assert CF.dimer_energy(m, s, c, rows[k], m.dinit) == dcal[k], (k, s, c)


# ---- 1. the exhaustive minimum

@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_gpu_cofold_is_the_minimum_of_the_definition_over_every_structure(paths, which):
    install(paths, which)
    m = mirror(which)
    cases = CF.draw_dimers(SEED, 40, n_hairpin=8, n_two=4)
    best = {(s, c): min(CF.dimer_energy(m, s, c, r, DINIT) for r in CF.enumerate_dimer(s, c)) for s, c in cases}
    batch = []
    for k, (s, c) in enumerate(cases):                  # each case three times, single strands between them: ONE batch
        batch += [(s, c), (s, 0), (s, c)]
    batch += cases[::-1]
    raw = run(batch)
    rows, dcal, n_pairs, n_inter, cut, status = raw
    assert status == [0] * len(batch)
    free = zuker.mfe_batch_raw([s for s, _ in cases])
    for k, (s, c) in enumerate(batch):
        if c:
            assert dcal[k] == best[s, c] and CF.dimer_energy(m, s, c, rows[k], DINIT) == dcal[k], (k, s, c, rows[k])
            assert n_inter[k] == sum(1 for x, y in enumerate(CF.pair_table(rows[k])) if x < c <= y) and n_pairs[k] == rows[k].count("(")
        else:
            j = k // 3
            assert (rows[k], dcal[k], n_pairs[k], n_inter[k], cut[k]) == (free[0][j], free[1][j], free[2][j], 0, 0)
    check_against_mirror(batch, raw, m)
    assert sum(x > 0 for x in n_inter) >= 3 * (15 if which == "builtin" else 25)
    sw = run(swapped(batch))
    assert sw[1] == dcal                                # the exterior loop and the loop with the nick trade places


# ---- 2. against the mirror where enumeration cannot reach

def long_dimers():
    rng = np.random.default_rng(SEED + 1)
    mid = [("".join(rng.choice(list("ACGU"), n)), c) for n, c in ((60, 21), (77, 40), (105, 64))]
    return mid + [(LR.RANDOM_SEQS[0], 66), (LR.RANDOM_SEQS[1], 99)]


def edge_dimers():
    dup = "GGCAUCGGAUCC"
    rc = "".join({"A": "U", "U": "A", "G": "C", "C": "G"}[x] for x in reversed(dup))
    rng = np.random.default_rng(SEED + 2)
    s70 = "".join(rng.choice(list("ACGU"), 70))
    apart_a, apart_b = "A" * 30, "".join(rng.choice(list("ACG"), 50))
    return dict(one_nt_a=(s70, 1), one_nt_b=(s70, 69), adjacent=("GGGGGGCCCCCC", 6), adjacent_short=("GC", 1), duplex=(dup + rc, len(dup)),
                apart=(apart_a + apart_b, 30))


def test_gpu_cofold_equals_the_mirror_at_60_to_197_nt_and_on_the_edge_cuts(paths):
    install(paths, "builtin")
    m = mirror("builtin")
    edges = edge_dimers()
    dimers = long_dimers() + list(edges.values())
    raw = run(dimers)
    check_against_mirror(dimers, raw, m)
    rows, dcal, n_pairs, n_inter, _, _ = raw
    by = {k: i + len(long_dimers()) for i, k in enumerate(edges)}
    # the adjacent pair (c-1, c): the optimum of G6 C6 stacks it, and the shortest dimer is that pair alone or nothing
    k = by["adjacent"]
    assert rows[k] == "(((((())))))" and n_inter[k] == 6
    assert rows[by["adjacent_short"]] in ("()", "..")
    # a perfect duplex: every position paired with the other strand
    k = by["duplex"]
    assert rows[k] == "(" * 12 + ")" * 12 and n_inter[k] == 12 and dcal[k] < -1000
    # an A-only strand beside a strand without U: the two single-strand folds side by side
    k = by["apart"]
    a, b = zuker.mfe_batch_raw(["A" * 30, edges["apart"][0][30:]])[:2]
    assert rows[k] == a[0] + a[1] and dcal[k] == b[0] + b[1] and n_inter[k] == 0
    assert sum(x > 0 for x in n_inter[:5]) >= 3
    assert run(swapped(dimers))[1] == dcal
    # the same bytes in the HBM class, with one sequence per chunk, in another order and alone
    assert run(dimers, max_lds_len=40) == raw and run(dimers, max_lds_len=1) == raw and run(dimers, max_lds_len=1, workspace_bytes=1) == raw
    back = run(dimers[::-1], max_lds_len=40)
    assert tuple(x[::-1] for x in back) == raw
    for k in (1, 4, by["duplex"]):
        assert tuple(x[0] for x in run(dimers[k:k + 1])) == tuple(x[k] for x in raw)


def test_gpu_cofold_equals_the_mirror_where_multiloops_win(paths):
    install(paths, "multiloops_win")
    dimers = long_dimers()[:3]
    raw = run(dimers)
    check_against_mirror(dimers, raw, mirror("multiloops_win"))
    assert run(dimers, max_lds_len=1) == raw and run(swapped(dimers))[1] == raw[1]
    assert any(CF.multiloop_with_cross_branch(r, c) for r, (_, c) in zip(raw[0], dimers))


def test_gpu_cofold_without_a_cut_is_rafft_mfe_batch():
    rng = np.random.default_rng(SEED + 3)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (60, 75, 90, 200)]
    free = zuker.mfe_batch_raw(seqs)
    for cuts in (None, [0] * 4):
        for kw in ({}, dict(max_lds_len=70)):
            rows, dcal, n_pairs, n_inter, cut, status = cofold.cofold_batch_raw(seqs, cuts, **kw)
            assert (rows, dcal, n_pairs, status) == free and n_inter == cut == [0] * 4


# ---- 3. duplex_init and the temperature

def test_gpu_cofold_takes_the_loaded_duplex_init_and_other_temperatures(paths):
    install(paths, "synthetic")
    dimers = long_dimers()[:2] + [edge_dimers()["duplex"]]
    tempf = lambda t: (t + 273.15) / (37.0 + 273.15)
    for temp in (37.0, 25.0, 60.0):
        want = 360 if temp == 37.0 else int(900 - (900 - 360) * tempf(temp))
        assert rafft_amd.cofold_duplex_init(temp) == want and want != DINIT
        raw = run(dimers, temp=temp)
        check_against_mirror(dimers, raw, mirror("synthetic", temp, want))
        assert raw[1][2] != mirror("synthetic", temp, want + 10).mfe_cut(*dimers[2])        # the value counts


# ---- 4. limits and errors

def test_gpu_cofold_limits_of_length_and_a_bad_cut():
    rng = np.random.default_rng(SEED + 4)
    s = "".join(rng.choice(list("ACGU"), 4097))
    rows, dcal, n_pairs, n_inter, cut, status = run([(s[:4096], 2048), (s, 2048), ("GGGAAACCC", 9), ("GGGG" + "CCCC", 4), ("GGGAAACCC", -1)])
    assert status == [0, N.ERR_TOO_LONG, N.ERR_STRUCT, 0, N.ERR_STRUCT]
    assert N.lib().rafft_last_error().decode() == "sequence 1: longer than RAFFT_MFE_MAX_LEN"
    assert rows[1] == "." * 4097 and rows[2] == rows[4] == "." * 9 and dcal[1] == dcal[2] == dcal[4] == 0 and cut == [2048, 0, 0, 4, 0]
    assert rows[3] == "(((())))" and n_inter[3] == 4
    # 4096 nt, cut 2048: the row is a structure of the dimer, it spans the nick, swapping the strands gives the same energy, and
    # the dimer lies at or below its two strands
    assert len(rows[0]) == 4096 and n_pairs[0] == rows[0].count("(") == rows[0].count(")") and n_inter[0] > 0
    pt = CF.pair_table(rows[0])
    assert n_inter[0] == sum(1 for x, y in enumerate(pt) if x < 2048 <= y)
    assert all(y < 0 or s[x] + s[y] in CF.PAIRS or s[y] + s[x] in CF.PAIRS for x, y in enumerate(pt))
    mono = zuker.mfe_batch_raw([s[:2048], s[2048:4096]])[1]
    assert dcal[0] <= mono[0] + mono[1] and run([(s[2048:4096] + s[:2048], 2048)])[1][0] == dcal[0]


# ---- 5. the Python surface and the command line

def test_gpu_cofold_python_and_cli(capsys):
    r = rafft_amd.cofold("GGCAUCGGAUCC", "GGAUCCGAUGCC", monomers=True)
    assert r.row == "(" * 12 + "&" + ")" * 12 and r.n_inter == 12
    mono = zuker.mfe_batch_raw(["GGCAUCGGAUCC", "GGAUCCGAUGCC"])[1]
    assert r.binding_dcal == r.dcal - mono[0] - mono[1] and r.binding < 0 and r.energy == rafft_amd.Structure("", r.dcal).energy
    cli.main(["-s", "GGCAUCGGAUCC&GGAUCCGAUGCC", "--cofold", "--binding"])
    out = capsys.readouterr().out.split()
    assert out[:3] == ["GGCAUCGGAUCC&GGAUCCGAUGCC", "24", r.row] and out[4] == "12" and len(out) == 9
    assert [float(x) for x in out[5:]] == [r.energy, r.energy_a, r.energy_b, r.binding] and float(out[3]) == r.energy
