"""The case sets of _cofold_cases do what tests/test_gpu_cofold_edges.py needs them for, shown with the numpy mirror alone: the
third-round dimers tell a strand-end loop of two rounds from the right one, each its own; the tie set ties at every kind of
decision of the dimer traceback, the two that only dimers have included, and at least ten of its dimers have one row per
candidate order; every mirror row has the energy the definition gives it; swapping the strands changes no energy.  And the five
long dimers of tests/test_gpu_cofold.py tie nowhere under the tables they run with: no test on them can see the candidate order.
Integers and strings: no tolerance.  No GPU."""
import pytest

import _cofold_cases as CC
import _cofold_np as CF
import test_gpu_cofold as TG


def energy(which, seq, c, row):
    return CF.dimer_energy(CC.mirror(which), seq, c, row, CC.DINIT)


def test_third_round_cases_tell_a_loop_of_two_rounds_from_the_right_one():
    cases = CC.third_round_cases()
    assert [k[4] for k in cases].count("fa") == [k[4] for k in cases].count("fb") == 3
    for kind, small in (("fa", True), ("fa", False), ("fb", True), ("fb", False)):      # both size classes, both loops
        assert any(k[4] == kind and k[1] == "builtin" and (len(k[2]) <= CC.LDS_LEN) == small for k in cases)
        assert any(k[4] == kind and k[1] == "multiloops_win" for k in cases)
    for name, which, seq, c, kind in cases:
        assert min(c, len(seq) - c) >= 133 or kind, name
        (dcal, row, n_inter), _ = CC.fold(which, seq, c)
        assert energy(which, seq, c, row) == dcal and n_inter > 0, name
        if kind is None:
            continue
        two = {d: CC.mirror(which, d + "_two_rounds").mfe_cut(seq, c) for d in ("fa", "fb")}
        other = "fb" if kind == "fa" else "fa"
        print(f"\n{name}: L {len(seq)} cut {c} dcal {dcal} fa_two_rounds {two['fa']} fb_two_rounds {two['fb']}")
        assert two[kind] > dcal and two[other] == dcal, (name, dcal, two)
        # the stem that makes the difference lies in the loop with the nick, on the strand the case is meant for
        pt = CF.pair_table(row)
        i = max(x for x, y in enumerate(pt) if x < c <= y)
        inside = CF.branches(pt, i + 1, pt[i] - 1)
        if kind == "fa":
            assert any(q < c and q - p >= 4 + 128 for p, q in inside), (name, row)
        else:
            assert any(p >= c + 128 for p, q in inside), (name, row)
        s, k = CC.swapped([(seq, c)])[0]
        assert CC.mirror(which).mfe_cut(s, k) == dcal, name


@pytest.fixture(scope="module")
def tie_counts():
    """{table set: (ties summed over the set, names whose "last" row differs)}"""
    out = {}
    for which in ("tie0", "tie1"):
        total, differ = dict.fromkeys(CF.TIE_KINDS + CF.TIE_NICK, 0), []
        for name, (seq, c) in CC.tie_cases().items():
            (dcal, row, n_inter), ties = CC.fold(which, seq, c)
            last, _ = CC.fold(which, seq, c, "last")
            assert last[0] == dcal == energy(which, seq, c, row) == energy(which, seq, c, last[1]), (which, name)
            assert n_inter == sum(1 for x, y in enumerate(CF.pair_table(row)) if x < c <= y)
            assert ties["C_cross"] >= max(ties["C_cross_nick_interior"], ties["C_cross_nick_split"])
            if last[1] != row:
                differ.append(name)
                assert sum(ties[k] for k in CF.TIE_KINDS) > 0, (which, name)
            for k, v in ties.items():
                total[k] += v
        out[which] = (total, differ)
        print(f"\n{which}: {total}; {len(differ)} of {len(CC.tie_cases())} dimers with two rows")
    return out


def test_tie_set_ties_at_every_kind_of_decision(tie_counts):
    cases = CC.tie_cases()
    assert all(40 <= len(cases["random%d" % n][0]) <= 150 for n in (40, 56, 72, 90, 110, 150))
    for k in range(CC.HOMO):
        s, c = cases["homo%d" % k]
        assert s[:c] == s[c:]
    assert CC.swapped([cases["het_ab"]]) == [cases["het_ba"]] and cases["het_ab"] != cases["het_ba"]
    total = {k: tie_counts["tie0"][0][k] + tie_counts["tie1"][0][k] for k in CF.TIE_KINDS + CF.TIE_NICK}
    for kind in CF.TIE_KINDS:
        assert total[kind] >= 3, (kind, total)
    assert total["FA"] >= 2 and total["FB"] >= 2
    assert total["C_cross_nick_interior"] >= 1 and total["C_cross_nick_split"] >= 1
    for which in ("tie0", "tie1"):
        assert len(tie_counts[which][1]) >= 10, which
    # the constructed dimers tie where they were built to
    for name, kind in (("fa_two_stems", "FA"), ("fa_unpaired", "FA"), ("fb_two_stems", "FB"), ("fb_unpaired", "FB"), ("nick_or_split", "C_cross_nick_split"),
                       ("nick_or_split_backwards", "C_cross_nick_split")):
        assert CC.fold("tie0", *cases[name])[1][kind] >= 1, name
    # "unpaired" against a stem, and two stems: the two orders of the FA / FB step that a kernel could get wrong
    for name in ("fa_unpaired", "fb_unpaired"):
        first, last = CC.fold("tie0", *cases[name])[0][1], CC.fold("tie0", *cases[name], "last")[0][1]
        assert first.count("(") + 4 == last.count("("), name
    for name in ("fa_two_stems", "fb_two_stems"):
        first, last = CC.fold("tie0", *cases[name])[0][1], CC.fold("tie0", *cases[name], "last")[0][1]
        assert first.count("(") == last.count("(") and first != last, name


def test_swapped_tie_dimers_have_equal_energies():
    for name, (seq, c) in CC.tie_cases().items():
        if len(seq) > 64:
            continue
        s, k = CC.swapped([(seq, c)])[0]
        for which in ("tie0", "tie1"):
            assert CC.mirror(which).mfe_cut(s, k) == CC.fold(which, seq, c)[0][0], (which, name)


def test_sweep_and_limit_cases():
    sweep, limit = CC.sweep_cases(), CC.limit_cases()
    assert [c for s, c in sweep if len(s) == 48] == list(range(1, 48)) and len({s for s, _ in sweep}) == 2
    assert [(len(s), c) for s, c in sweep[47:]] == [(133, c) for c in (1, 63, 64, 65, 127, 128, 129, 132)]
    assert [(len(s), c) for s, c in limit] == [(146, 4), (146, 73), (146, 142), (147, 4), (147, 73)]
    for which in ("builtin", "tie1"):                           # the 48-nt dimers; the long ones are folded by the GPU test's mirror
        inter = 0
        for seq, c in sweep[:47]:
            (dcal, row, n_inter), _ = CC.fold(which, seq, c)
            assert energy(which, seq, c, row) == dcal
            assert c % 6 or CC.mirror(which).mfe_cut(seq[c:] + seq[:c], 48 - c) == dcal, (which, c)
            inter += n_inter > 0
        assert inter >= 36, (which, inter)                      # three cuts in four leave pairs between the strands


def test_the_long_dimers_of_test_gpu_cofold_tie_nowhere():
    """why this file exists: on the mirror cases of test_gpu_cofold the first and the last reproducing candidate give the same
    row, and no decision but M has two candidates at all.  M has, on the 197-nt dimer: an unpaired position before the stems of
    a multiloop is taken by "i unpaired" or left to the first part of a split, two derivations of one structure"""
    for seq, c in TG.long_dimers():
        first, ties = CC.fold("builtin", seq, c)
        assert CC.fold("builtin", seq, c, "last")[0] == first, (len(seq), c)
        assert not any(v for k, v in ties.items() if k != "M"), (len(seq), c, ties)
    assert len(TG.long_dimers()) == 5
