"""rafft_findpath_batch past 64 moves and past 64 beam states, on a real MI355X (`-m gpu`), against the definition
(`_findpath_np.search` over whole-structure oracle energies) on the problems of tests/_findpath_cases.py - what each is built for,
and that it gets there, is shown on the CPU by tests/test_findpath_cases.py:
 (a) hairpins opened with d = 64, 65, 66, 70: removals across the edge of the first mask word, beams of 64-80 states;
 (b) slipping helices with d = 128, 129, 144 and 135: additions that wait for removals numbered 64 and above, masks of two and three
     words, conflict masks that are 0 in word 0;
 (c) d = 66 at width 100 and d = 65 at width 160, where a duplicate test that stops after one round of 64 ranks, or after two,
     returns another path;
 (d) d = 12 at width 1024 with 924 and 672 live states: the record, moves and energies of the definition, and its saddle is the exact
     one (dynamic programming over all subsets).  That is equality and exactness only: no test here claims to see the beam's tail
     past rank 512 - on such problems a select that dropped it would return the same path;
 (e) one chunk of four problems with one, three, two and three mask words, the longest not the one of the largest d: the same bits
     whole, reversed, one problem a chunk, and each alone.
(a) and (b) also at widths 1, 2, 7 and once under an index-sensitive table set; every row of every path evaluates back (eval_kernel).
Integers and bytes: no tolerance.  Measured on the MI355X machine: the file alone 13.3 s (5.5, 4.0, 3.5, 0.1, 0.1 s a test), nearly
all of it the Python mirrors of the host, each computed once a process (the cache of _findpath_cases); every device call is under a
second."""
import pytest

import _findpath_cases as FC
import _findpath_np as FP
from test_gpu_findpath import back_to_builtin, bits, evaluate_back, install, run, same_as_mirror, sets       # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def against_the_mirror(which, probs, widths):
    """one call; record, moves and energies of every problem are those of FP.search under the tables `which` (computed once a
    process: the cache of _findpath_cases)"""
    recs, moves, dcal = run(probs, widths)
    for k, prob in enumerate(probs):
        same_as_mirror(prob, widths[k], recs[k], moves[k], dcal[k], want=FC.mirror(which, prob, widths[k]))
    return recs, moves, dcal


def word_edge_batch(small=True):
    cases = FC.removal_cases() + FC.addition_cases()
    probs = [p for _, p, w in cases for _ in range(1 + 3 * small)]
    widths = [x for _, p, w in cases for x in ((w,) + FC.SMALL_WIDTHS if small else (w,))]
    return probs, widths


def test_word_edge_problems_equal_the_mirror_at_their_width_and_at_1_2_7():
    probs, widths = word_edge_batch()
    assert len(probs) == 32 and sorted({FC.mask_words(FC.dist(p)[0]) for p in probs}) == [1, 2, 3]
    recs, moves, dcal = against_the_mirror("builtin", probs, widths)
    assert evaluate_back(probs, recs, moves, dcal) == sum(FC.dist(p)[0] + 1 for p in probs)
    # the width matters on these landscapes: were every saddle the same at 1 and at W, a beam of one state would pass as well
    assert sum(recs[4 * k]["saddle_dcal"] < recs[4 * k + 1]["saddle_dcal"] for k in range(8)) >= 2


def test_word_edge_problems_under_index_sensitive_tables(sets):
    probs, widths = word_edge_batch(small=False)
    for prob, width in zip(probs, widths):      # the mirrors first: forming their tables (_loops.builtin_par) resets the library's
        FC.mirror("index", prob, width)
    install(sets, "index")
    recs, moves, dcal = against_the_mirror("index", probs, widths)
    evaluate_back(probs, recs, moves, dcal)
    install(sets, "builtin")
    assert [r["start_dcal"] for r in recs] != [FC.mirror("builtin", p, w)["start_dcal"] for p, w in zip(probs, widths)]


def test_dedup_sensitive_problems_equal_the_mirror():
    cases = FC.dedup_cases()
    probs, widths = [p for _, p, _, _ in cases], [w for _, _, w, _ in cases]
    assert widths == [100, 160]
    recs, moves, dcal = against_the_mirror("builtin", probs, widths)
    evaluate_back(probs, recs, moves, dcal)
    # ... which is not what a duplicate test of one round, or of two, returns (CPU: tests/test_findpath_cases.py)
    for k, (_, prob, width, defect) in enumerate(cases):
        wrong = FC.marked("builtin", prob, width, defect)[0]
        assert [tuple(m) for m in moves[k].tolist()] != wrong["moves"]


def test_full_beams_at_width_1024_equal_the_mirror_and_are_exact():
    cases = FC.full_beam_cases()
    probs = [p for _, p, _ in cases]
    recs, moves, dcal = against_the_mirror("builtin", probs, [FC.FULL_WIDTH] * len(probs))
    evaluate_back(probs, recs, moves, dcal)
    for rec, prob in zip(recs, probs):
        assert rec["saddle_dcal"] == FP.exact_saddle(*prob)


def test_mixed_chunk_same_bits_whole_reversed_chunked_and_alone():
    chunk = FC.mixed_chunk()
    probs, widths = [p for p, _ in chunk], [w for _, w in chunk]
    whole = against_the_mirror("builtin", probs, widths)
    want = [bits(*whole, k) for k in range(len(probs))]
    back = run(probs[::-1], widths[::-1])
    assert [bits(*back, k) for k in range(len(probs))] == want[::-1]
    apart = run(probs, widths, workspace_bytes=1)
    assert [bits(*apart, k) for k in range(len(probs))] == want
    for k in range(len(probs)):
        alone = run([probs[k]], [widths[k]])
        assert bits(*alone, 0) == want[k]
