"""rafft_mfe_span_batch on a real MI355X (`-m gpu`): the minimum over every structure that obeys the span of short sequences, the
bits of rafft_mfe_batch where the span does not bind - on bands wide enough for every round count of the exterior loop and its
tail as well -, the rows of the tests' span mirror in the documented candidate order, other
temperatures, sequences of up to 32 768 nt whose fold is known exactly, same input - same bits, the errors, the command line.
Integers and bytes: no tolerance."""
import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, params, rafft as R, zuker
import _loops as LP
import _mfe_span_np as MS
import _par_reader as PR
from test_gpu_mfe import sets, install, check_rows, exhaustive_sequences, enumerated, mirror_sequences, multiloops  # noqa: F401 (sets: a fixture)

pytestmark = pytest.mark.gpu

TABLES = ("builtin", "multiloops_win")
FIXED_SPANS = (1, 4, 5, 6, 8, 12, 4096)


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()


def triples(raw):
    return list(zip(raw[0], raw[1], raw[2]))


def check_span_rows(seqs, raw, span, temp=37.0):
    check_rows(seqs, raw, temp)
    assert all(MS.obeys(r, span) for r in raw[0])


_MIRRORS = {}


def span_mirror(sets, which, temp=37.0):
    key = (which, temp)
    if key not in _MIRRORS:
        _MIRRORS[key] = MS.SpanMirror(PR.tables_at(sets[which], temp))
    return _MIRRORS[key]


# ---- 1. the exhaustive minimum under the span

@pytest.mark.parametrize("which", TABLES)
def test_gpu_mfe_span_is_the_minimum_over_every_structure_that_obeys_the_span(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    assert 40 <= len(seqs) <= 49 and max(map(len, seqs)) == 20
    rows = enumerated(seqs)
    flat_s = [s for s, rr in zip(seqs, rows) for _ in rr]
    flat_r = [r for rr in rows for r in rr]
    en, st = R.eval_structures(flat_s, flat_r)                                     # every structure once, whatever the span
    assert not any(st)
    widest = [max((j - i + 1 for i, j in MS.pairs_of(r)), default=0) for r in flat_r]
    at, per_seq = 0, []
    for rr in rows:
        per_seq.append((en[at:at + len(rr)], widest[at:at + len(rr)]))
        at += len(rr)
    want = lambda k, span: min(e for e, w in zip(*per_seq[k]) if w <= span)
    n_bound = 0
    for span in FIXED_SPANS:
        raw = zuker.mfe_span_batch_raw(seqs, span)
        assert raw[1] == [want(k, span) for k in range(len(seqs))], span
        check_span_rows(seqs, raw, span)
        n_bound += sum(d > want(k, 4096) for k, d in enumerate(raw[1]))
        if span <= 4:
            assert raw[0] == ["." * len(s) for s in seqs] and raw[1] == [0] * len(seqs) and raw[2] == [0] * len(seqs)
    assert n_bound >= 20                                                           # the span binds
    for length in sorted(set(map(len, seqs))):                                     # spans L - 1 and L
        ks = [k for k, s in enumerate(seqs) if len(s) == length]
        for span in {max(length - 1, 1), length}:
            raw = zuker.mfe_span_batch_raw([seqs[k] for k in ks], span)
            assert raw[1] == [want(k, span) for k in ks], (length, span)
            check_span_rows([seqs[k] for k in ks], raw, span)
    free = zuker.mfe_span_batch_raw(seqs, 4096)
    assert free == zuker.mfe_batch_raw(seqs)
    if which == "multiloops_win":
        assert sum(multiloops(r) > 0 for s, r in zip(seqs, free[0]) if 16 <= len(s) <= 20) >= 3


# ---- 2. the bits of rafft_mfe_batch where the span does not bind

@pytest.mark.parametrize("which", ["builtin", "multiloops_win", "tie0", "tie1"])
def test_gpu_mfe_span_equals_mfe_batch_at_span_of_the_length_and_more(sets, which):
    install(sets, which)
    seqs = mirror_sequences() if which in TABLES else LP.tie_short_sequences() + LP.tie_long_sequences()
    lds = zuker.mfe_batch_raw(seqs)
    hbm = zuker.mfe_batch_raw(seqs, max_lds_len=4)
    assert lds == hbm
    longest = max(map(len, seqs))
    for span in (longest, 4096):
        assert zuker.mfe_span_batch_raw(seqs, span) == lds, span
    for length in sorted(set(map(len, seqs))):                                     # span = L exactly
        ks = [k for k, s in enumerate(seqs) if len(s) == length]
        got = zuker.mfe_span_batch_raw([seqs[k] for k in ks], length)
        assert triples(got) == [triples(lds)[k] for k in ks], length


# ---- 2b. wide bands: every round count of the exterior loop and its tail

WIDE_LENGTHS = (150, 300, 450, 530, 700, 1200)     # W = L: 3, 5, 7 and 8 rounds fetched ahead; beyond 516 the tail loop as well


def wide_sequences():
    rng = np.random.default_rng(516)
    return ["".join(rng.choice(list("ACGU"), n)) for n in WIDE_LENGTHS]


def test_gpu_mfe_span_equals_mfe_batch_on_wide_bands():
    """W = L from 150 to 1200: the exterior loop fetches (W - 4 + 63) / 64 rounds ahead, eight at most, and reads a wider band's
    rest in its tail loop; the exterior stems of these folds lie anywhere in the window"""
    seqs = wide_sequences()
    assert sorted({min(8, (n - 4 + 63) // 64) for n in WIDE_LENGTHS + (100, 230, 360)}) == list(range(2, 9))
    ref = zuker.mfe_batch_raw(seqs)
    assert ref == zuker.mfe_batch_raw(seqs, max_lds_len=4)
    assert zuker.mfe_span_batch_raw(seqs, 4096) == ref
    for k, s in enumerate(seqs):                                                   # span = L exactly, alone
        assert triples(zuker.mfe_span_batch_raw([s], len(s))) == [triples(ref)[k]], len(s)
    widest = [max(j - i + 1 for i, j in MS.pairs_of(r)) for r in ref[0]]
    assert all(w > 64 for w in widest) and max(widest) > 516                       # far candidates decide: pairs beyond round 1 and in the tail
    # lengths whose W = L gives the round counts 2, 4 and 6 (the others are above)
    more = [s[:n] for s, n in zip(seqs[1:4], (100, 230, 360))]
    ref2 = zuker.mfe_batch_raw(more)
    for k, s in enumerate(more):
        assert triples(zuker.mfe_span_batch_raw([s], len(s))) == [triples(ref2)[k]], len(s)


def wide_block_sequence(block_len, run, n_blocks, seed):
    rng = np.random.default_rng(seed)
    # a GC helix of eight pairs closes every block, so that its exterior stem is the farthest candidate of its window
    bl = ["GGGGCGCG" + "".join(rng.choice(list("ACGU"), block_len - k - 16)) + "CGCGCCCC" for k in range(n_blocks)]
    return "N" * 3 + ("N" * run).join(bl) + "N" * 2, bl


@pytest.mark.parametrize("span,block_len", [(150, 140), (300, 280), (600, 560)])
def test_gpu_mfe_span_wide_windows_that_start_above_0(span, block_len):
    """blocks a little shorter than the span between runs of `span` N: no pair leaves a block, a block's pairs reach almost the whole
    window, and every window but the first block's starts above 0.  A block of at most `span` nt between two N folds as under
    rafft_mfe_batch (test 2), so the row is the concatenation of those rows and dcal their sum."""
    seq, bl = wide_block_sequence(block_len, span, 4, span)
    rows, dcal, _, status = zuker.mfe_batch_raw(["N" + b + "N" for b in bl])
    assert not any(status)
    want_row = "..." + ("." * span).join(r[1:-1] for r in rows) + ".."
    got = zuker.mfe_span_batch_raw([seq], span)
    assert got[0] == [want_row] and got[1] == [sum(dcal)] and got[2] == [want_row.count("(")]
    check_span_rows([seq], got, span)
    far = max(j - i + 1 for i, j in MS.pairs_of(want_row))
    assert far > span - 64, far                                                    # a pair in the last round of the window
    assert zuker.mfe_span_batch_raw([seq], span - 100)[1][0] > got[1][0]           # and a narrower span binds


def test_gpu_mfe_span_150_binds_and_equals_the_mirror(sets):
    """260 nt at span 150: three rounds fetched ahead, windows that start above 0, and a span that binds - the mirror bit for bit"""
    install(sets, "builtin")
    seq = wide_sequences()[1][:260]
    want = span_mirror(sets, "builtin").fold(seq, 150)
    got = zuker.mfe_span_batch_raw([seq], 150)
    assert triples(got) == [(want[1], want[0], want[1].count("("))]
    check_span_rows([seq], got, 150)
    assert got[1][0] > zuker.mfe_batch_raw([seq])[1][0]                            # the span binds
    assert max(j - i + 1 for i, j in MS.pairs_of(want[1])) > 128                   # a pair in the third round


# ---- 3. the mirror, bit for bit

MIRROR_SPANS = (10, 30, 64, 65, 100)
# 110 A, then a hairpin (110, 123): at span 100 the window of j = 123 starts at 24 and the stem is its candidate 86
WINDOW_SEQ = "A" * 110 + "GGGGGAAAACCCCC" + "AA"
# under the flat tables: a closing helix of two pairs around three hairpins of five pairs at 2, 72 and 85 - 100 nt, the most span 100
# holds; the C split of (1, 98) has its last stem at k = 85 = (i + 6) + 78, the M split of (2, 84) at k = 72 = (i + 5) + 65.  (A helix
# of two pairs and hairpins of five are the smallest that are favourable under these tables: 65 is the largest offset span 100 allows.)
SPLIT_SEQ = "GG" + "CCCCCNNNGGGGG" + "N" * 57 + "AAAAANNNUUUUU" + "UUUUUNNNAAAAA" + "UU"


def mirror_span_sequences(which):
    if which == "builtin":
        rng = np.random.default_rng(1800)
        caps = [s + "A" * (60 - len(s)) for s in mirror_sequences()[-2:]]        # the 30 / 31 cap sequences, padded to 60 nt
        return ["".join(rng.choice(list("ACGU"), n)) for n in (60, 97, 150)] + caps + [WINDOW_SEQ]
    return [s for s in LP.tie_long_sequences() if len(s) >= 60][:3] + [SPLIT_SEQ, WINDOW_SEQ]


def mirror_span_folds(sets, which, seqs, span, temp=37.0):
    """((dcal, row) of every sequence, the largest offsets taken): SpanMirror.fold in the documented order"""
    mirror = span_mirror(sets, which, temp)
    out, off, window = [], dict(F=-1, M=-1, C=-1, I=-1), -1
    for s in seqs:
        out.append(mirror.fold(s, span))
        off = {k: max(v, mirror.offsets[k]) for k, v in off.items()}
        window = max(window, mirror.window_offset)
    return out, off, window


@pytest.mark.parametrize("which", ["builtin", "tie0"])
def test_gpu_mfe_span_rows_are_the_span_mirrors(sets, which):
    install(sets, which)
    seqs = mirror_span_sequences(which)
    assert len(SPLIT_SEQ) == 100 and all(60 <= len(s) <= 200 for s in seqs)
    for span in MIRROR_SPANS:
        want, off, window = mirror_span_folds(sets, which, seqs, span)
        raw = zuker.mfe_span_batch_raw(seqs, span)
        wrong = [(s, r, w[1]) for s, r, w in zip(seqs, raw[0], want) if r != w[1]]
        assert not wrong, (which, span, len(wrong), wrong[:3])
        assert raw[1] == [w[0] for w in want] and raw[2] == [w[1].count("(") for w in want]
        check_span_rows(seqs, raw, span)
        print(f"\n{which} span {span}: largest candidate offsets {off}, in a window that starts above 0: {window}")
        if span == 100:
            assert window >= 64                     # an exterior stem found in the second ballot round of a window that starts above 0
            if which == "tie0":
                assert off["M"] == 65 and off["C"] == 78   # the second ballot round of both, past its first lane
        if which == "builtin" and span >= 64:
            # the 30 / 31 cap of interior loops: the run of 30 is bridged by one bulge, at 31 the outer helix is given up
            r30, r31 = raw[0][-3], raw[0][-2]
            assert r30.startswith("(((((" + "." * 30 + "(((((") and not r31.startswith("(((((")


# ---- 4. other temperatures

@pytest.mark.parametrize("temp", [25.0, 60.0])
def test_gpu_mfe_span_at_another_temperature(sets, temp):
    install(sets, "synthetic")
    seqs = mirror_sequences()[:4] + exhaustive_sequences()[20:30]
    at37 = {span: zuker.mfe_span_batch_raw(seqs, span) for span in (12, 30)}
    n_other = 0
    for span in (12, 30):
        want, _, _ = mirror_span_folds(sets, "synthetic", seqs, span, temp)
        raw = zuker.mfe_span_batch_raw(seqs, span, temp=temp)
        assert raw[0] == [w[1] for w in want] and raw[1] == [w[0] for w in want]
        check_span_rows(seqs, raw, span, temp)
        n_other += sum(a != b for a, b in zip(raw[1], at37[span][1]))
    assert n_other >= 1
    for span in (12, 30):                                                          # 37 C comes back
        again = zuker.mfe_span_batch_raw(seqs, span)
        assert again == at37[span]
        want, _, _ = mirror_span_folds(sets, "synthetic", seqs, span)
        assert again[1] == [w[0] for w in want]


# ---- 5. beyond 4096 nt, with an exact expectation

RUN = 70                                            # N between two blocks: no pair of span <= 70 leaves a block
LAST_BLOCK = "GGGGCGCAAGCGCCCC"                     # closes at the last position


def blocks():
    rng = np.random.default_rng(32768)
    return ["".join(rng.choice(list("ACGU"), n)) for n in (55, 58, 60, 61, 63, 65)]


def block_sequence(length):
    """(sequence, its parts): a run of N, blocks with RUN N behind each, LAST_BLOCK - `length` positions.  parts: (text, None) of a
    run and (block, flanks) of a block, flanks being the N it has before and behind it (1 or 0)"""
    bl, parts, n, k = blocks(), [], len(LAST_BLOCK), 0
    while n + len(bl[k % len(bl)]) + RUN + 1 <= length:
        b = bl[k % len(bl)]
        parts += [(b, (1, 1)), ("N" * RUN, None)]
        n += len(b) + RUN
        k += 1
    parts = [("N" * (length - n), None)] + parts + [(LAST_BLOCK, (1, 0))]
    seq = "".join(p[0] for p in parts)
    assert len(seq) == length and length - n >= 1
    return seq, parts


def block_expectation(mirror, parts, span, cache):
    """(dcal, row) of a block sequence: no pair leaves a block, so the row is the blocks' rows between dots and dcal their sum"""
    dcal, row = 0, []
    for text, flanks in parts:
        if flanks is None:
            row.append("." * len(text))
            continue
        key = (text, flanks, span)
        if key not in cache:
            d, r = mirror.fold("N" * flanks[0] + text + "N" * flanks[1], span)
            cache[key] = (d, r[flanks[0]:len(r) - flanks[1]])
        dcal += cache[key][0]
        row.append(cache[key][1])
    return dcal, "".join(row)


def test_gpu_mfe_span_beyond_4096_nt_is_the_sum_of_its_blocks(sets):
    install(sets, "builtin")
    mirror, cache = span_mirror(sets, "builtin"), {}
    lengths = (4097, 5000, 17000, 32768)
    built = [block_sequence(n) for n in lengths]
    seqs = [b[0] for b in built]
    short = "GGGAAACCC"
    alone = {span: zuker.mfe_span_batch_raw([short], span) for span in (40, 70)}
    for span in (40, 70):
        want = [block_expectation(mirror, b[1], span, cache) for b in built]
        call = seqs + ["A" * (N.MFE_SPAN_MAX_LEN + 1), short]
        rows, dcal, n_pairs, status = zuker.mfe_span_batch_raw(call, span)
        assert status == [0] * 4 + [N.ERR_TOO_LONG, 0]
        assert N.lib().rafft_last_error().decode() == "sequence 4: longer than RAFFT_MFE_SPAN_MAX_LEN"
        for k, n in enumerate(lengths):
            assert dcal[k] == want[k][0] and rows[k] == want[k][1], (n, span)
            assert n_pairs[k] == rows[k].count("(") and dcal[k] < 0
        assert rows[3][N.MFE_SPAN_MAX_LEN - 1] == ")" and rows[3][N.MFE_SPAN_MAX_LEN - len(LAST_BLOCK)] == "("
        assert max(i for i, c in enumerate(rows[0]) if c == "(") >= 4080             # stack words beyond 12 bits of i
        check_span_rows(seqs, (rows[:4], dcal[:4], n_pairs[:4], status[:4]), span)
        assert (rows[4], dcal[4], n_pairs[4]) == ("." * (N.MFE_SPAN_MAX_LEN + 1), 0, 0)
        assert (rows[5], dcal[5], n_pairs[5]) == triples(alone[span])[0]
    assert len({w for w in cache.values()}) >= 6


# ---- 6. same input, same bits

def test_gpu_mfe_span_same_input_same_bits():
    rng = np.random.default_rng(6)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (33, 158, 71, 20, 264, 45, 80, 9)]
    for span in (30, 100):
        whole = zuker.mfe_span_batch_raw(seqs, span)
        row = dict(zip(seqs, triples(whole)))
        check_span_rows(seqs, whole, span)
        for k in (0, 4, len(seqs) - 1):                                            # alone
            assert triples(zuker.mfe_span_batch_raw([seqs[k]], span)) == [row[seqs[k]]]
        for order in (seqs[::-1], [seqs[k] for k in rng.permutation(len(seqs))], seqs[1:] + seqs[:1]):
            assert triples(zuker.mfe_span_batch_raw(order, span)) == [row[s] for s in order]
        # one sequence a chunk; room for the tables of the two longest, then less
        for budget in (1, 4 * (264 + 158) * span * 4, 4 * 80 * span * 4):
            assert zuker.mfe_span_batch_raw(seqs, span, workspace_bytes=budget) == whole


# ---- 7. errors

def test_gpu_mfe_span_errors():
    good = ["GGGGAAAACCCC", "GGGAAACCCAGGGAAACCC", "GCGCUUCGGCGC"]
    alone = zuker.mfe_span_batch_raw(good, 12)
    for span in (0, -1, N.MFE_MAX_LEN + 1):
        with pytest.raises(N.RafftError) as e:
            zuker.mfe_span_batch_raw(good, span)
        assert e.value.code == N.ERR_PARAM
    L = N.lib()
    _, arr, lens, bufs, out = N.seq_arrays(good, rows=True)
    rec = (N.MfeSeq * len(good))()
    assert L.rafft_mfe_span_batch(len(good), arr, lens, 37.0, 12, 0, None, out) == N.ERR_PARAM
    assert L.rafft_mfe_span_batch(len(good), None, lens, 37.0, 12, 0, rec, out) == N.ERR_PARAM
    assert L.rafft_mfe_span_batch(len(good), arr, lens, 37.0, 12, -1, rec, out) == N.ERR_PARAM
    seqs = [good[0], "", good[1], "GGGXAAACCC", good[2]]
    rows, dcal, n_pairs, status = zuker.mfe_span_batch_raw(seqs, 12)                 # returns: the call is RAFFT_OK
    assert status == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, 0]
    assert L.rafft_last_error().decode().startswith("sequence 1")
    assert [rows[k] for k in (1, 3)] == ["", "." * 10] and [dcal[k] for k in (1, 3)] == [0, 0]
    keep = (0, 2, 4)
    assert ([rows[k] for k in keep], [dcal[k] for k in keep], [n_pairs[k] for k in keep], [0] * 3) == alone
    got = rafft_amd.mfe_span_batch(seqs, 12, raise_errors=False)
    assert [g is None for g in got] == [False, True, False, True, False]
    assert got[0].str_struct == rows[0] and got[0].dcal == dcal[0] and rafft_amd.mfe_span(good[0], 12).str_struct == rows[0]
    with pytest.raises(KeyError):
        rafft_amd.mfe_span_batch(seqs[2:4], 12)
    for batch in (good, ["", "GGGXAACCC"]):                                        # the built-in tables are 37 C only
        with pytest.raises(N.RafftError) as e:
            zuker.mfe_span_batch_raw(batch, 12, temp=25.0)
        assert e.value.code == N.ERR_TEMP


# ---- 8. the command line

def test_gpu_cli_mfe_span(tmp_path, capsys):
    from rafft_amd import cli
    rng = np.random.default_rng(40)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (50, 90, 130)] + ["GGGGAAAACCCC"]
    fa = tmp_path / "s.fa"
    fa.write_text("".join(f">s{k}\n{s}\n" for k, s in enumerate(seqs)))
    out = tmp_path / "o.txt"
    cli.main(["-sf", str(fa), "--batch", "--mfe", "--span", "40", "-o", str(out)])
    want = rafft_amd.mfe_span_batch(seqs, 40)
    assert out.read_text().splitlines() == [cli.format_mfe_line(s, st) for s, st in zip(seqs, want)]
    assert [st.str_struct for st in want] == zuker.mfe_span_batch_raw(seqs, 40)[0]
    assert [st.str_struct for st in want] != [st.str_struct for st in rafft_amd.mfe_batch(seqs)]       # the span binds
    cli.main(["-s", seqs[0], "--mfe", "--span", "40"])
    assert capsys.readouterr().out == cli.format_mfe_line(seqs[0], want[0]) + "\n"
    csvf = tmp_path / "known.csv"
    csvf.write_text("".join(f"{s},{st.str_struct},n{k}\n" for k, (s, st) in enumerate(zip(seqs, want))))
    sc = tmp_path / "scores.csv"
    cli.main(["-sf", str(csvf), "--batch", "--mfe", "--span", "40", "--scores", str(sc)])
    got = sc.read_text().splitlines()
    assert len(got) == 1 + len(seqs) and all(line.split(",")[2] == st.str_struct for line, st in zip(got[1:], want))
    with pytest.raises(SystemExit):
        cli.main(["-s", seqs[0], "--span", "40"])
