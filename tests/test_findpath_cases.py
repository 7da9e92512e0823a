"""The problems of _findpath_cases do what tests/test_gpu_findpath_edges.py needs them for, shown with the Python mirrors alone:
the search in the kernels' scheme (duplicates marked against the lower ranks, all unmarked candidates sorted, the first W kept -
the claim of rafft_findpath.hip's header) returns the moves and energies of the definition on the short problems and on every
case; each case takes the loops as far as it was built to (mask words, marks at moves >= 64 and >= 128, additions kept back by
removals numbered >= 64 alone, ranks >= 64 that are the first to form a duplicate, beams above 64 and above 512 states); and each
error a kernel could make there - conflicts read in word 0 only, the duplicate's bit taken modulo 64, a duplicate test or an
offer of moves that stops after one or two rounds of 64 - changes the result of the case built for it, the duplicate test's the
RETURNED PATH, not just the beam.  The full beams at width 1024 find the exact saddle.  Integers and strings: no tolerance.  No GPU.
The file takes about 30 s, all of it the mirrors (whole-structure oracle energies, one store a problem); it prints its slowest
mirrors and fails above a minute.  tests/test_gpu_findpath_edges.py reads the same cache."""
import time

import pytest

import oracle
import _findpath_cases as FC
import _findpath_np as FP


@pytest.fixture(autouse=True)
def clean_tables():
    yield
    oracle.reset_tables()


@pytest.fixture(scope="module", autouse=True)
def under_a_minute():
    t0 = time.perf_counter()
    yield
    took = time.perf_counter() - t0
    for key, t in sorted(FC.TIMES.items(), key=lambda kv: -kv[1])[:12]:
        print(f"\n{t:6.2f} s  {key[0]} {key[1]} d {FC.dist(key[2])[0]} width {key[3]} {key[4] if len(key) > 4 else ''}", end="")
    print(f"\nthe file: {took:.1f} s")
    assert took < 60.0, took


def both_mirrors(name, prob, width):
    """search_marked without a defect == search; (result, stats)"""
    want = FC.mirror("builtin", prob, width)
    got, stats = FC.marked("builtin", prob, width)
    assert got == want, (name, width)
    d, n_rem = FC.dist(prob)
    took = [FC.TIMES.get(("findpath " + kind, "builtin", prob, width) + rest, 0.0) for kind, rest in (("search", ()), ("marked", (None,)))]
    print(f"\n{name}: L {len(prob[0])} d {d} n_rem {n_rem} W {width} saddle {want['saddle_dcal']} {stats} search {took[0]:.2f} s marked {took[1]:.2f} s", end="")
    return want, stats


def changed(name, prob, width, defect):
    """what the defect returns, which is not what the definition returns: None (no candidate left), "invalid", or another path"""
    right = FC.mirror("builtin", prob, width)
    wrong, _ = FC.marked("builtin", prob, width, defect)
    what = wrong if wrong in (None, "invalid") else "other moves" if wrong["moves"] != right["moves"] else "the same moves"
    print(f"\n    {defect}: {what}", end="")
    assert wrong != right, (name, width, defect)
    return wrong


def test_marked_search_is_the_definition_on_the_short_problems():
    for k, prob in enumerate(FP.host_problems()):
        for width in (256, 3):
            stats = {}
            assert FP.search_marked(*prob, width, stats=stats) == FP.search(*prob, width), (k, width)
            assert stats["max_live"] <= min(width, 252) and stats["marks_ge64"] == 0


def test_removals_across_the_word_edge():
    cases = FC.removal_cases()
    assert [FC.dist(p) for _, p, _ in cases] == [(64, 64), (65, 65), (66, 66), (70, 70)]
    assert [FC.mask_words(FC.dist(p)[0]) for _, p, _ in cases] == [1, 2, 2, 2] and all(w <= 130 for _, _, w in cases)
    for name, prob, width in cases:
        assert set(prob[0]) == set("ACGU") and prob[1].count("(") == FC.dist(prob)[0] and set(prob[2]) == {"."}, name
        _, stats = both_mirrors(name, prob, width)
        d = FC.dist(prob)[0]
        assert stats["max_live"] == stats["max_k"] == width and stats["marks_ge128"] == 0
        if d == 64:
            assert stats["marks_ge64"] == 0     # move 63 is the last bit of the only word: nothing of a second round exists
        else:
            assert stats["marks_ge64"] > 0, name
            changed(name, prob, width, "dup_bit_word0")
            if d == 65:                         # (one move of a second round is as good as six: the search is stuck at level 64)
                assert changed(name, prob, width, "moves_rounds:1") is None
        if width > 65:                          # (rank 64 of 65 is the last: it forms no duplicate for a higher one)
            assert stats["max_first_rank"] >= 64, name


def test_additions_across_the_word_edge():
    cases = FC.addition_cases()
    assert [FC.dist(p) for _, p, _ in cases] == [(128, 68), (129, 68), (144, 72), (135, 99)]
    assert [FC.mask_words(FC.dist(p)[0]) for _, p, _ in cases] == [2, 3, 3, 3] and all(w <= 8 for _, _, w in cases)
    for name, prob, width in cases:
        mv, n_rem = FP.move_list(prob[1], prob[2])
        conf = FP.conflict_masks(mv, n_rem)[n_rem:]
        assert all(conf) and sum(1 for c in conf if c >> 64) >= 4, name
        _, stats = both_mirrors(name, prob, width)
        assert stats["marks_ge64"] > 0 and stats["refused_high"] > 0, name
        # an addition that does not wait for its removals numbered 64 and above leaves the structures
        assert changed(name, prob, width, "conf_word0") == "invalid"
        changed(name, prob, width, "dup_bit_word0")
        assert changed(name, prob, width, "moves_rounds:1") is None
        if len(mv) > 128:
            assert stats["marks_ge128"] > 0, name
            assert changed(name, prob, width, "moves_rounds:2") is None
    # half_opened: the seven opened units hold the removals 0-62, so every addition but the first (removals 63 and 64) waits for nothing in word 0
    mv, n_rem = FP.move_list(*cases[3][1][1:])
    conf = FP.conflict_masks(mv, n_rem)[n_rem:]
    assert len(conf) == 36 and sum(1 for c in conf if not c & FP.WORD and c >> 64) == 35 and conf[0] == 3 << 63


def test_a_duplicate_test_of_one_round_or_two_returns_another_path():
    (name1, prob1, width1, defect1), (name2, prob2, width2, defect2) = FC.dedup_cases()
    assert 65 <= FC.dist(prob1)[0] <= 70 and 65 <= width1 <= 130 and defect1 == "dedup_rounds:1"
    assert 65 <= FC.dist(prob2)[0] <= 70 and width2 >= 129 and defect2 == "dedup_rounds:2"
    for name, prob, width, defect in FC.dedup_cases():
        right, stats = both_mirrors(name, prob, width)
        assert stats["max_live"] == width and stats["max_first_rank"] >= 64 * int(defect[-1]) and stats["marks_ge64"] > 0, name
        wrong = changed(name, prob, width, defect)
        assert wrong["moves"] != right["moves"] or wrong["dcal"] != right["dcal"], name

def test_full_beams_at_the_largest_width_are_exact():
    cases = FC.full_beam_cases()
    assert FC.FULL_WIDTH == 1024 and [FC.dist(p)[0] for _, p, _ in cases] == [12] * 4 and len(cases[0][1][0]) == 40
    assert cases[1][1] == (cases[0][1][0], cases[0][1][2], cases[0][1][1])
    for name, prob, live in cases:
        mv, n_rem = FP.move_list(prob[1], prob[2])
        assert any(FP.conflict_masks(mv, n_rem)) == (live < 924), name
        want, stats = both_mirrors(name, prob, FC.FULL_WIDTH)
        assert stats["max_live"] == stats["max_k"] == live > 512 and stats["max_first_rank"] >= 512, name
        assert want["saddle_dcal"] == FP.exact_saddle(*prob), name


def test_mixed_chunk_holds_every_number_of_words():
    chunk = FC.mixed_chunk()
    assert [FC.mask_words(FC.dist(p)[0]) for p, _ in chunk] == [1, 3, 2, 3] and [FC.dist(p)[0] for p, _ in chunk] == [12, 144, 65, 135]
    lens = [len(p[0]) for p, _ in chunk]
    assert lens[0] == 40 and max(lens) == lens[3] and FC.dist(chunk[3][0])[0] < 144
