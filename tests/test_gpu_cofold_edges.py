"""rafft_cofold_batch on a real MI355X (`-m gpu`) where tests/test_gpu_cofold.py does not take it, on the
case sets of _cofold_cases (tests/test_cofold_cases.py shows with the mirror alone that they can fail):
the third round of the 64-lane loops over a strand end, FA and FB, in the fill and in the traceback, in both size classes;
the candidate order of the dimer traceback under the flat tables tie0 and tie1 - the row is the mirror's "first" row and, where the
two differ, not its "last" one - at every kind of decision, FA, FB and nick loop against interior loop and split included;
every cut of a 48-nt dimer, and the cuts around 64 and 128 of a 133-nt one; dimers of RAFFT_MFE_LDS_LEN nt and one more under the
default class switch; two dimers of 4096 nt whose rows evaluate back to their energies.
Against the numpy mirror `CutMirror` (energy, row, n_inter) and the definition `dimer_energy`.  Integers and bytes: no tolerance."""
import importlib

import numpy as np
import pytest

from rafft_amd import _native as N, params, zuker
import _cofold_cases as CC
import _cofold_np as CF
import _par_reader as PR

cofold = importlib.import_module("rafft_amd.cofold")        # (the package's attribute `cofold` is the function)

pytestmark = pytest.mark.gpu

DINIT = CC.DINIT


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("par")
    out = {}
    for name in ("multiloops_win", "tie0", "tie1"):
        out[name] = d / (name + ".par")
        PR.write_par(CC.par_of(name), out[name], comment=name)
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


def run(dimers, **kw):
    """cofold_batch_raw of a list of (seq, cut)"""
    return cofold.cofold_batch_raw([d[0] for d in dimers], [d[1] for d in dimers], **kw)


def inter_of(row, c):
    return sum(1 for x, y in enumerate(CF.pair_table(row)) if x < c <= y)


def check_against_mirror(which, dimers, raw):
    rows, dcal, n_pairs, n_inter, cut, status = raw
    assert status == [0] * len(dimers) and cut == [c for _, c in dimers]
    for k, (s, c) in enumerate(dimers):
        want, _ = CC.fold(which, s, c)
        assert (dcal[k], rows[k], n_inter[k]) == want and n_pairs[k] == rows[k].count("("), (which, k, s, c, rows[k], dcal[k], want)
        assert CF.dimer_energy(CC.mirror(which), s, c, rows[k], DINIT) == dcal[k], (which, k, s, c)


# ---- 1. the third round of FA and FB

@pytest.mark.parametrize("which", ["builtin", "multiloops_win"])
def test_gpu_cofold_strand_end_loops_past_their_second_round(paths, which):
    install(paths, which)
    cases = [k for k in CC.third_round_cases() if k[1] == which]
    dimers = [(seq, c) for _, _, seq, c, _ in cases]
    raw = run(dimers)
    check_against_mirror(which, dimers, raw)
    assert all(x > 0 for x in raw[3])
    # the classes differ in where G lives (LDS behind the bases / cofold_ends_kernel's copy in device memory), not in the bytes
    assert run(dimers, max_lds_len=1) == raw and run(dimers, max_lds_len=1, workspace_bytes=1) == raw
    assert run(CC.swapped(dimers))[1] == raw[1]


# ---- 2. the candidate order

@pytest.mark.parametrize("which", ["tie0", "tie1"])
def test_gpu_cofold_takes_the_first_candidate_where_the_tables_tie(paths, which):
    install(paths, which)
    cases = CC.tie_cases()
    names, dimers = list(cases), list(cases.values())
    raw = run(dimers)
    check_against_mirror(which, dimers, raw)
    two_rows = 0
    for k, (s, c) in enumerate(dimers):
        last, _ = CC.fold(which, s, c, "last")
        if last[1] != CC.fold(which, s, c)[0][1]:
            two_rows += 1
            assert raw[0][k] != last[1], (which, names[k])
    assert two_rows >= 10
    assert run(dimers, max_lds_len=1) == raw                    # the same ballots over tables in device memory
    sw = run(CC.swapped(dimers))
    assert sw[1] == raw[1]
    # a homodimer swapped is the same input; two different strands both ways round are not
    assert raw[1][names.index("het_ab")] == raw[1][names.index("het_ba")] == sw[1][names.index("het_ba")]


# ---- 3. every cut

@pytest.mark.parametrize("which", ["builtin", "tie1"])
def test_gpu_cofold_at_every_cut_of_48_nt_and_around_the_lane_rounds_of_133_nt(paths, which):
    install(paths, which)
    dimers = CC.sweep_cases()
    raw = run(dimers)
    check_against_mirror(which, dimers, raw)
    assert run(dimers, max_lds_len=1) == raw
    for c in (1, 24, 47):
        assert dimers[c - 1][1] == c and tuple(x[0] for x in run(dimers[c - 1:c])) == tuple(x[c - 1] for x in raw)


# ---- 4. the limit of the LDS class

def test_gpu_cofold_at_the_limit_of_the_lds_class_and_one_above(paths):
    install(paths, "builtin")
    dimers = CC.limit_cases()
    assert N.lib().rafft_mfe_lds_len() == CC.LDS_LEN and [len(s) for s, _ in dimers] == [CC.LDS_LEN] * 3 + [CC.LDS_LEN + 1] * 2
    raw = run(dimers)                                           # the default switch: three in LDS with G at the top of it, two in device memory
    check_against_mirror("builtin", dimers, raw)
    assert run(dimers[:3], max_lds_len=CC.LDS_LEN - 1) == tuple(x[:3] for x in raw)
    assert run(dimers, max_lds_len=CC.LDS_LEN - 1) == raw


# ---- 5. 4096 nt

def nick_loop_of(row, c):
    """what holds the nick in the row of a single strand: "exterior", or the kind of the loop the innermost pair around it closes"""
    pt = CF.pair_table(row)
    around = [x for x, y in enumerate(pt) if x < c <= y]
    if not around:
        return "exterior"
    i = max(around)
    return ("hairpin", "interior", "multiloop")[min(len(CF.branches(pt, i + 1, pt[i] - 1)), 2)]


def test_gpu_cofold_rows_of_4096_nt_evaluate_back_to_their_energies(paths):
    """cut at 2048, and cut at 130: strand A takes three rounds of the FA loops, strand B 62 of FB's.  No mirror reaches this
    length; the definition does, loop by loop over the row"""
    install(paths, "builtin")
    rng = np.random.default_rng(CC.SEED + 3)
    dimers = [("".join(rng.choice(list("ACGU"), 4096)), c) for c in (2048, 130)]
    rows, dcal, n_pairs, n_inter, cut, status = run(dimers)
    assert status == [0, 0] and cut == [2048, 130]
    m = CC.mirror("builtin")
    free = zuker.mfe_batch_raw([x for s, c in dimers for x in (s[:c], s[c:], s)])
    assert free[3] == [0] * 6
    for k, (s, c) in enumerate(dimers):
        assert len(rows[k]) == 4096 and CF.dimer_energy(m, s, c, rows[k], DINIT) == dcal[k], k
        assert n_inter[k] == inter_of(rows[k], c) and n_pairs[k] == rows[k].count("(")
        assert dcal[k] <= free[1][3 * k] + free[1][3 * k + 1]
        # the fold of the concatenation is a structure of the dimer too; where the nick falls into its exterior loop or into an
        # interior loop, the dimer's minimum lies at or below what the definition gives that row
        whole = free[0][3 * k + 2]
        kind = nick_loop_of(whole, c)
        print(f"\n4096 nt cut {c}: dcal {dcal[k]}, strands {free[1][3 * k]} + {free[1][3 * k + 1]}, n_inter {n_inter[k]}; the nick of the single-strand row lies in: {kind}")
        if kind in ("exterior", "interior"):
            assert dcal[k] <= CF.dimer_energy(m, s, c, whole, DINIT), k
