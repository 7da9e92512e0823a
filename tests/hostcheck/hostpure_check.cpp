// Host-side check of rafft_amd/csrc/rafft_hostpure.h: the lane cut of a batch, the dot-bracket parsers, the base codes, the
// enclosing-loop walk, the row layout of the scoring calls and the planning of the batch drivers (chunk planner, sequence pack,
// graph pack, solve order, and the layouts of the four sequence drivers with the sizes of rafft_batch_layout.h), against values
// derived by hand from the rules.  Plain C++, no HIP, no GPU.  Test infrastructure.
#include <cstdio>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static std::vector<int> lens_of(std::initializer_list<std::pair<int, int>> groups)      // {count, length} ...
{
    std::vector<int> v;
    for (auto &g : groups) v.insert(v.end(), (size_t)g.first, g.second);
    return v;
}
static std::vector<SeqIn> seqs_of(const std::vector<int> &lens)
{
    std::vector<SeqIn> v;
    for (size_t i = 0; i < lens.size(); i++) v.push_back(SeqIn{nullptr, lens[i], (int)i, 0});
    return v;
}

static void check_lanes()
{
    // automatic: fewer than 32 sequences are never cut; the cut is twice the element below the top two (or the top 1 %)
    CHECK(split_length(lens_of({{29, 100}, {2, 3000}}), -1) == 0);
    CHECK(split_length(lens_of({{31, 50}}), -1) == 0);
    CHECK(split_length(lens_of({{100, 100}, {2, 300}}), -1) == 200);
    CHECK(split_length(lens_of({{2, 300}, {100, 100}}), -1) == 200);       // (the order of the batch does not matter)
    CHECK(split_length(lens_of({{100, 100}, {3, 300}}), -1) == 0);         // the element below the top two is itself 300
    CHECK(split_length(lens_of({{100, 100}, {2, 199}}), -1) == 0);
    CHECK(split_length(lens_of({{16382, 100}, {2, 3000}}), -1) == 0);      // 16 384 sequences amortise the tail
    CHECK(split_length(lens_of({{16381, 100}, {2, 3000}}), -1) == 200);
    // forced
    CHECK(split_length(lens_of({{100, 100}, {2, 300}}), 0) == 0);
    CHECK(split_length(lens_of({{16382, 100}, {2, 3000}}), 0) == 0);
    CHECK(split_length(lens_of({{32, 100}}), 150) == 150);
    CHECK(split_length(lens_of({{31, 100}}), 150) == 0);
    CHECK(split_length(lens_of({{16382, 100}, {2, 3000}}), 150) == 150);
    // lanes and estimate
    {
        const std::vector<SeqIn> good = seqs_of(lens_of({{1, 300}, {100, 100}, {1, 300}}));
        const std::vector<LaneJob> j = cut_lanes(good, 200, 0.0);
        CHECK(j.size() == 2 && j[0].lane == 0 && j[1].lane == 1);
        CHECK(j.size() == 2 && j[0].seqs.size() == 2 && j[0].seqs[0].idx == 0 && j[0].seqs[1].idx == 101 && j[0].est == 9.0);
        CHECK(j.size() == 2 && j[1].seqs.size() == 100 && j[1].seqs[0].idx == 1 && j[1].seqs[99].idx == 100 && j[1].est == 7.0);
        const std::vector<LaneJob> all_long = cut_lanes(good, 100, 0.0);     // nothing left below the cut: one job
        CHECK(all_long.size() == 1 && all_long[0].lane == 0 && all_long[0].seqs.size() == 102);
    }
    {
        const std::vector<LaneJob> a = cut_lanes(seqs_of(lens_of({{255, 250}})), 0, 0.0), b = cut_lanes(seqs_of(lens_of({{256, 250}})), 0, 0.0);
        CHECK(a.size() == 1 && a[0].lane == 0 && a[0].seqs.size() == 255 && a[0].est == 8.5);
        CHECK(b.size() == 1 && b[0].lane == 1 && b[0].seqs.size() == 256 && b[0].est == 8.5);
        const std::vector<LaneJob> c = cut_lanes(seqs_of(lens_of({{255, 250}})), 0, 2.5);
        CHECK(c.size() == 1 && c[0].est == 2.5);
        const std::vector<LaneJob> d = cut_lanes(seqs_of(lens_of({{1, 300}, {100, 100}})), 200, 2.5);
        CHECK(d.size() == 2 && d[0].est == 2.5 && d[1].est == 2.5);
        CHECK(cut_lanes({}, 0, 0.0).empty());
    }
}

static void check_parsers()
{
    std::vector<int16_t> pt;
    CHECK(parse_db("((..))", 6, pt) && pt == (std::vector<int16_t>{5, 4, -1, -1, 1, 0}));
    CHECK(parse_db("", 0, pt) && pt.empty());
    CHECK(!parse_db(")(", 2, pt));
    CHECK(!parse_db("(()", 3, pt));
    CHECK(!parse_db("(.x)", 4, pt));
    uint16_t t[8];
    int nk = -1;
    std::string err;
    CHECK(score_known_table("(<[.]>)", 7, t, &nk, err) && nk == 3);
    CHECK(t[0] == 7 && t[6] == 1 && t[1] == 6 && t[5] == 2 && t[2] == 5 && t[4] == 3 && t[3] == 0);
    CHECK(score_known_table("([)]", 4, t, &nk, err) && nk == 2 && t[0] == 3 && t[2] == 1 && t[1] == 4 && t[3] == 2);     // separate stacks
    CHECK(score_known_table("(>.", 3, t, &nk, err) && nk == 1 && t[0] == 2 && t[1] == 1 && t[2] == 0);                 // ( and < share one
    CHECK(!score_known_table("(..)", 5, t, &nk, err) && err == "known structure of length 4 for a sequence of length 5");
    CHECK(!score_known_table("(.)]", 4, t, &nk, err) && err == "known structure: unmatched ']' at position 3");
    CHECK(!score_known_table(".<(.)", 5, t, &nk, err) && err == "known structure: unclosed bracket at position 1");
    CHECK(!score_known_table("[[..]", 5, t, &nk, err) && err == "known structure: unclosed bracket at position 0");
    CHECK(!score_known_table("(.x)", 4, t, &nk, err) && err == "known structure: character 'x' at position 2");
    static const char bases[] = "NACGU";
    for (int c = 0; c < 256; c++) {
        const char *at = c ? strchr(bases, c) : nullptr;
        if (at) CHECK(kBaseCode[(unsigned char)c] == at - bases);
        else CHECK(kBaseCode[(unsigned char)c] & 8);
    }
}

static void check_enclosing_loop()
{
    std::vector<int16_t> pt;
    const char *db = "((..((..))..((..))..))";
    CHECK(parse_db(db, (int)strlen(db), pt));
    LoopOf lp = enclosing_loop(pt, 10);
    CHECK(lp.ci == 1 && lp.cj == 20 && lp.br == (std::vector<uint32_t>{4u | 9u << 16, 12u | 17u << 16}));
    lp = enclosing_loop(pt, 6);                         // inside the first inner helix: its hairpin loop, no branches
    CHECK(lp.ci == 5 && lp.cj == 8 && lp.br.empty());
    CHECK(parse_db("..(..)..", 8, pt));
    lp = enclosing_loop(pt, 0);
    CHECK(lp.ci == -1 && lp.cj == 8 && lp.br == (std::vector<uint32_t>{2u | 5u << 16}));
    lp = enclosing_loop(pt, 6);                         // behind the helix: still the exterior loop
    CHECK(lp.ci == -1 && lp.cj == 8 && lp.br.size() == 1);
}

static void check_score_layout()
{
    // three sequences of length 4, stride 5: rows of 0 and 1 in chunk A (at 10 and at 300), rows of 2 in chunk B (at 64)
    std::vector<char> A(1000, 'a'), B(500, 'b');
    const int lens[3] = {4, 4, 4}, stride[3] = {5, 5, 5}, n_rows[3] = {2, 3, 1};
    const char *rows[3] = {A.data() + 10, A.data() + 300, B.data() + 64};
    const char *base[2] = {A.data(), B.data()};
    const size_t cap[2] = {A.size(), B.size()};
    std::vector<ScoreSrc> src;
    std::vector<unsigned long long> off(3, 99);
    size_t bytes = 0;
    CHECK(score_chunk_layout(3, lens, n_rows, stride, rows, 2, base, cap, src, off, bytes));
    // chunk A: from row 0 of sequence 0 (10) to the end of the last row of sequence 1 (300 + 2 * 5 + 4 = 314): 304 bytes -> 512
    CHECK(src.size() == 2 && src[0].base == A.data() + 10 && src[0].bytes == 304 && src[0].dev_off == 0);
    CHECK(src.size() == 2 && src[1].base == B.data() + 64 && src[1].bytes == 4 && src[1].dev_off == 512);
    CHECK(off[0] == 0 && off[1] == 290 && off[2] == 512 && bytes == 768);
    for (int s = 0; s < 3; s++)       // rows_off points at the sequence's first row inside its source's device range
        for (const ScoreSrc &x : src)
            if (rows[s] >= x.base && rows[s] < x.base + x.bytes) CHECK(off[s] == x.dev_off + (size_t)(rows[s] - x.base));
    {   // a sequence without rows takes part in nothing; a chunk nobody points into gives no source
        const int nr[3] = {2, 0, 0};
        const char *rw[3] = {A.data() + 10, nullptr, nullptr};
        CHECK(score_chunk_layout(3, lens, nr, stride, rw, 2, base, cap, src, off, bytes));
        CHECK(src.size() == 1 && src[0].bytes == 9 && off[0] == 0 && off[1] == 0 && off[2] == 0 && bytes == 256);
    }
    {   // a range outside every chunk (here: its last row ends one byte past chunk B): not in chunks
        const char *rw[3] = {A.data() + 10, A.data() + 300, B.data() + 497};
        CHECK(!score_chunk_layout(3, lens, n_rows, stride, rw, 2, base, cap, src, off, bytes));
        std::vector<char> other(16, 'c');
        const char *rw2[3] = {A.data() + 10, other.data(), B.data()};
        CHECK(!score_chunk_layout(3, lens, n_rows, stride, rw2, 2, base, cap, src, off, bytes));
        CHECK(!score_chunk_layout(3, lens, n_rows, stride, rows, 0, nullptr, nullptr, src, off, bytes));
    }
    // score_pack: rows back to back with their strides kept; a sequence with a pre-set status contributes no bytes
    std::vector<char> r0 = {'(', '.', '.', ')', 0, '.', '.', '.', '.'}, r1 = {'(', '(', ')', ')'}, r2 = {'.', '(', ')', '.', 0, '(', '.', '.', ')'};
    const char *prow[3] = {r0.data(), r1.data(), r2.data()};
    const int pn[3] = {2, 1, 2};
    std::vector<char> pack;
    std::vector<unsigned long long> poff(3);
    score_pack(3, lens, pn, prow, stride, nullptr, pack, poff);
    CHECK(pack.size() == 22 && poff[0] == 0 && poff[1] == 9 && poff[2] == 13);
    CHECK(!memcmp(pack.data(), r0.data(), 9) && !memcmp(pack.data() + 9, r1.data(), 4) && !memcmp(pack.data() + 13, r2.data(), 9));
    const int pre[3] = {0, 5, 0};
    score_pack(3, lens, pn, prow, stride, pre, pack, poff);
    CHECK(pack.size() == 18 && poff[0] == 0 && poff[1] == 9 && poff[2] == 9);
    CHECK(!memcmp(pack.data(), r0.data(), 9) && !memcmp(pack.data() + 9, r2.data(), 9));
    const int none[3] = {0, 0, 0};
    score_pack(3, lens, none, prow, stride, nullptr, pack, poff);
    CHECK(pack.empty() && poff[0] == 0 && poff[2] == 0);
}

typedef std::vector<size_t> Sizes;
static Sizes flat(const ChunkPlan &p)      // a0, b0, a1, b1, ...
{
    Sizes v;
    for (const ChunkPlan::Range &c : p.chunks) { v.push_back(c.a); v.push_back(c.b); }
    return v;
}

static void check_chunk_planner()
{
    const size_t c100[3] = {100, 100, 100};
    ChunkPlan p = plan_chunks(0, nullptr, nullptr, 100, 0);
    CHECK(p.chunks.empty() && p.off.empty() && p.max_cost == 0 && p.max_cost2 == 0);
    p = plan_chunks(3, c100, nullptr, 1, 0);                         // nothing fits beside another: one item per chunk
    CHECK(flat(p) == (Sizes{0, 1, 1, 2, 2, 3}) && p.off == (Sizes{0, 0, 0}) && p.max_cost == 100 && p.max_cost2 == 0);
    p = plan_chunks(3, c100, nullptr, 200, 0);                       // 100 + 100 is not over 200
    CHECK(flat(p) == (Sizes{0, 2, 2, 3}) && p.off == (Sizes{0, 100, 0}) && p.max_cost == 200);
    p = plan_chunks(3, c100, nullptr, 199, 0);
    CHECK(flat(p) == (Sizes{0, 1, 1, 2, 2, 3}) && p.off == (Sizes{0, 0, 0}) && p.max_cost == 100);
    {   // an item larger than the budget stands alone, and is the largest total
        const size_t c[3] = {10, 500, 10};
        p = plan_chunks(3, c, nullptr, 100, 0);
        CHECK(flat(p) == (Sizes{0, 1, 1, 2, 2, 3}) && p.off == (Sizes{0, 0, 0}) && p.max_cost == 500);
    }
    {   // items without cost join the open chunk (100 + 0 is not over 100); the second 100 does not
        const size_t c[5] = {100, 0, 0, 100, 0};
        p = plan_chunks(5, c, nullptr, 100, 0);
        CHECK(flat(p) == (Sizes{0, 3, 3, 5}) && p.off == (Sizes{0, 100, 100, 0, 100}) && p.max_cost == 100);
        const size_t d[2] = {500, 0};                                // ... but not a chunk that is over the budget already
        p = plan_chunks(2, d, nullptr, 100, 0);
        CHECK(flat(p) == (Sizes{0, 1, 1, 2}) && p.off == (Sizes{0, 0}) && p.max_cost == 500);
    }
    {   // the cap on items
        const size_t c[5] = {1, 1, 1, 1, 1};
        p = plan_chunks(5, c, nullptr, 100, 2);
        CHECK(flat(p) == (Sizes{0, 2, 2, 4, 4, 5}) && p.off == (Sizes{0, 1, 0, 1, 0}) && p.max_cost == 2);
        p = plan_chunks(5, c, nullptr, 100, 0);                      // 0: no cap
        CHECK(flat(p) == (Sizes{0, 5}) && p.off == (Sizes{0, 1, 2, 3, 4}) && p.max_cost == 5);
    }
    {   // the secondary cost alone forces the cut (60 + 60 > 100 while 10 + 10 fits); 60 + 10 fits; both largest totals are reported
        const size_t c[3] = {10, 10, 10}, c2[3] = {60, 60, 10};
        p = plan_chunks(3, c, c2, 100, 0);
        CHECK(flat(p) == (Sizes{0, 1, 1, 3}) && p.off == (Sizes{0, 0, 10}) && p.max_cost == 20 && p.max_cost2 == 70);
        const size_t big2[2] = {300, 1};                             // the largest secondary total may be an oversize item's
        p = plan_chunks(2, c, big2, 100, 0);
        CHECK(flat(p) == (Sizes{0, 1, 1, 2}) && p.max_cost == 10 && p.max_cost2 == 300);
    }
}

static void check_sequence_pack()
{
    typedef std::vector<int> Ints;
    {   // four good sequences with an empty one, one with an X and one of max_len + 1 between them; max_len 19
        const char *seqs[7] = {"GGGGAAAACCCC", "", "GGGAAACCCAGGGAAACCC", "GGGXAAACCC", "GCGCUUCGGCGC", "AAAAAAAAAAAAAAAAAAAA", "ACGUACGUACGUACGUAGC"};
        const int lens[7] = {12, 0, 19, 10, 12, 20, 19};
        const SeqPack p = pack_sequences(7, seqs, lens, 19);
        CHECK(p.status == (Ints{0, RAFFT_ERR_EMPTY, 0, RAFFT_ERR_BAD_CHAR, 0, RAFFT_ERR_TOO_LONG, 0}));
        CHECK(p.len == (Ints{12, 0, 19, 10, 12, 20, 19}));
        CHECK(p.L == (Ints{12, 0, 19, 0, 12, 0, 19}));
        CHECK(p.fold == (Ints{0, 2, 4, 6}));
        CHECK(p.code_off == (std::vector<unsigned long long>{0, 12, 12, 31, 31, 43, 43}));
        CHECK(p.codes == (std::vector<uint8_t>{3, 3, 3, 3, 1, 1, 1, 1, 2, 2, 2, 2,
                                               3, 3, 3, 1, 1, 1, 2, 2, 2, 1, 3, 3, 3, 1, 1, 1, 2, 2, 2,
                                               3, 2, 3, 2, 4, 4, 2, 3, 3, 2, 3, 2,
                                               1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 1, 3, 2,
                                               0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
        CHECK(p.first_err == "sequence 1: empty");
    }
    {   // the other two texts; too long comes before a bad character, a negative length is an empty sequence of length 0; N is code 0
        const char *seqs[4] = {"NACGU", "GGGXAAACCC", "XXXXXX", "ACGU"};
        const int lens[4] = {5, 10, 6, -2};
        SeqPack p = pack_sequences(4, seqs, lens, 5);
        CHECK(p.status == (Ints{0, RAFFT_ERR_TOO_LONG, RAFFT_ERR_TOO_LONG, RAFFT_ERR_EMPTY}) && p.len == (Ints{5, 10, 6, 0}) && p.fold == (Ints{0}));
        CHECK(p.codes.size() == 21 && p.codes[0] == 0 && p.codes[1] == 1 && p.codes[2] == 2 && p.codes[3] == 3 && p.codes[4] == 4 && p.codes[5] == 0);
        CHECK(p.first_err == "sequence 1: longer than RAFFT_MFE_MAX_LEN");
        p = pack_sequences(2, seqs + 1, lens + 1, 10);
        CHECK(p.status == (Ints{RAFFT_ERR_BAD_CHAR, RAFFT_ERR_BAD_CHAR}) && p.first_err == "sequence 0: character outside ACGUN");
        p = pack_sequences(1, seqs, lens, 5);
        CHECK(p.status == (Ints{0}) && p.first_err.empty());
    }
    {   // a null sequence with a length of 0 or below is not read; a batch of nothing but errors has nothing to fold
        const char *seqs[2] = {nullptr, nullptr};
        const int lens[2] = {0, -3};
        const SeqPack p = pack_sequences(2, seqs, lens, 19);
        CHECK(p.status == (Ints{RAFFT_ERR_EMPTY, RAFFT_ERR_EMPTY}) && p.len == (Ints{0, 0}) && p.L == (Ints{0, 0}) && p.fold.empty());
        CHECK(p.codes == std::vector<uint8_t>(16, 0) && p.code_off == (std::vector<unsigned long long>{0, 0}) && p.first_err == "sequence 0: empty");
        const SeqPack none = pack_sequences(0, nullptr, nullptr, 19);
        CHECK(none.status.empty() && none.fold.empty() && none.codes.size() == 16 && none.first_err.empty());
    }
}

static void check_graph_pack()
{
    typedef std::vector<int> Ints;
    CHECK(kin_prev_step(0, 1) == 0 && kin_prev_step(0, 4) == 3 && kin_prev_step(1, 4) == 0 && kin_prev_step(3, 4) == 2);
    // graph 0: L 3 in rows of stride 5, steps of 1, 0 and 2 rows; graph 1: no steps; graph 2: L 2, stride 2, steps of 2 and 1 rows.
    // The buffer of graph 0 ends with its last row's third byte: reading a whole stride there is an overrun.
    const std::vector<char> r0 = {'.', '.', '.', 'x', 'x', '(', '.', ')', 'y', 'y', '(', ')', '.'};
    const std::vector<char> r2 = {'a', 'b', 'c', 'd', 'e', 'f'};
    const int lens[3] = {3, 4, 2}, n_steps[3] = {3, 0, 2}, stride[3] = {5, 4, 2};
    const int ss0[3] = {1, 0, 2}, ss2[2] = {2, 1};
    const int *step_size[3] = {ss0, nullptr, ss2};
    const char *rows[3] = {r0.data(), nullptr, r2.data()};
    const double e0[3] = {1.0, 2.0, 3.0}, e2[3] = {4.0, 5.0, 6.0};
    const double *energy[3] = {e0, nullptr, e2};
    KinPack p;
    CHECK(kin_pack(3, lens, n_steps, step_size, rows, stride, energy, p));
    CHECK(p.n == 6 && p.bytes == 15 && p.rows.size() == 16);
    CHECK(p.n_rows == (Ints{3, 0, 3}) && p.row0 == (Ints{0, 3, 3}) && p.off == (std::vector<unsigned long long>{0, 9, 9}));
    CHECK(p.row_graph == (Ints{0, 0, 0, 2, 2, 2}));
    // graph 0: step 0 (row 0) against the last step (rows 1, 2); step 2 (rows 1, 2) against the empty step 1, which starts at row 1.
    // graph 2: step 0 (rows 3, 4) against step 1 (row 5); step 1 against step 0
    CHECK(p.row_prev0 == (Ints{1, 1, 1, 5, 5, 3}));
    CHECK(p.row_nprev == (Ints{2, 0, 0, 1, 1, 2}));
    CHECK(!memcmp(p.rows.data(), "...(.)().abcdef", 15));
    CHECK(p.energy == (std::vector<double>{1.0, 2.0, 3.0, 4.0, 5.0, 6.0}));
    {   // a graph of one step is compared with itself; rows of stride L go over as they lie
        const int one_len[1] = {2}, one_steps[1] = {1}, one_stride[1] = {2}, ss[1] = {3};
        const int *one_ss[1] = {ss};
        const char *one_rows[1] = {r2.data()};
        const double *one_e[1] = {e2};
        CHECK(kin_pack(1, one_len, one_steps, one_ss, one_rows, one_stride, one_e, p));
        CHECK(p.n == 3 && p.bytes == 6 && p.row_prev0 == (Ints{0, 0, 0}) && p.row_nprev == (Ints{3, 3, 3}) && !memcmp(p.rows.data(), "abcdef", 6));
    }
    {   // 2^31 - 1 rows and one more: refused before a row is read
        const int big_len[2] = {1, 1}, big_steps[2] = {1, 1}, big_stride[2] = {1, 1}, sa[1] = {0x7fffffff}, sb[1] = {1};
        const int *big_ss[2] = {sa, sb};
        const char *no_rows[2] = {nullptr, nullptr};
        const double *no_e[2] = {nullptr, nullptr};
        CHECK(!kin_pack(2, big_len, big_steps, big_ss, no_rows, big_stride, no_e, p));
        CHECK(p.rows.empty() && p.row_graph.empty());
    }
    CHECK(kin_pack(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, p) && p.n == 0 && p.bytes == 0);
}

static void check_solve_order()
{
    const int S[7] = {0, 5, 200, 128, 129, 0, 1};
    int order[7] = {-1, -1, -1, -1, -1, -1, -1};
    SolveCounts c = kin_solve_order(S, 0, 7, 128, order);
    CHECK(c.n_small == 3 && c.n_big == 2);
    CHECK(order[0] == 1 && order[1] == 3 && order[2] == 6 && order[3] == 2 && order[4] == 4 && order[5] == -1 && order[6] == -1);
    int part[7] = {-1, -1, -1, -1, -1, -1, -1};                      // the chunk [2, 5) writes from order[2]
    c = kin_solve_order(S, 2, 5, 128, part);
    CHECK(c.n_small == 1 && c.n_big == 2);
    CHECK(part[0] == -1 && part[1] == -1 && part[2] == 3 && part[3] == 2 && part[4] == 4 && part[5] == -1);
    c = kin_solve_order(S, 5, 6, 128, part);                         // nothing to solve
    CHECK(c.n_small == 0 && c.n_big == 0 && part[5] == -1);
}

// ---- the layouts of the sequence drivers

typedef std::vector<int> Ints;
typedef std::vector<unsigned long long> Offs;

// a pack of sequences of these lengths (all A); a length of 0 is an empty sequence, an error between the others
static SeqPack pack_of(const Ints &lens)
{
    std::vector<std::string> text;
    for (int n : lens) text.push_back(std::string((size_t)n, 'A'));
    std::vector<const char *> seqs;
    for (const std::string &s : text) seqs.push_back(s.c_str());
    return pack_sequences((int)lens.size(), seqs.data(), lens.data(), 4096);
}
template <class Q> static Offs tab_offs(const std::vector<Q> &qs) { Offs v; for (const Q &q : qs) v.push_back(q.tab_off); return v; }

static void check_chunk_lmax()
{
    const Ints L = {5, 2, 7, 9}, order = {3, 0, 2, 1};              // lengths in the order of the plan: 9, 5, 7, 2
    CHECK(chunk_lmax(ChunkPlan::Range{0, 3}, order, L) == 9);       // the longest is the first
    CHECK(chunk_lmax(ChunkPlan::Range{1, 3}, order, L) == 7);       // ... the last
    CHECK(chunk_lmax(ChunkPlan::Range{3, 4}, order, L) == 2);       // ... the only one
    CHECK(chunk_lmax(ChunkPlan::Range{0, 4}, order, L) == 9);
    CHECK(chunk_lmax(ChunkPlan::Range{2, 2}, order, L) == 0);
}

static void check_mfe_layout()
{
    // mfe_lds_bytes: 3 triangles, F and the padded bases.  146: (3 * 10731 + 147) * 4 + 160 = 129520 <= 131072 < 131288 = (3 * 10878 + 148) * 4 + 160
    CHECK(mfe_lds_bytes(146) == 129520 && mfe_lds_bytes(147) == 131288 && MFE_LDS_BYTES == 131072 && RAFFT_MFE_LDS_LEN == 146);
    const SeqPack pk = pack_of({0, 5, 146, 147, 5});
    CHECK(pk.code_off == (Offs{0, 0, 5, 151, 298}));
    {
        const MfeLayout y = mfe_layout(pk, 146, 1 << 30);
        // 146 is the last length of the LDS class, 147 the first of the other; the two 5s keep their input order behind 146
        CHECK(y.lds_order == (Ints{2, 1, 4}) && y.hbm_order == (Ints{3}) && y.order == (Ints{2, 1, 4, 3}));
        // stacks of L + 8 words, rows of L + 1 bytes, in input order; the error takes nothing: 0 | 13 | 13 + 154 | 167 + 155 | 322 + 13
        Offs stack, db, code;
        Ints L;
        for (const MfeSeq &q : y.qs) { stack.push_back(q.stack_off); db.push_back(q.db_off); code.push_back(q.code_off); L.push_back(q.L); CHECK(q.pad == 0); }
        CHECK(stack == (Offs{0, 0, 13, 167, 322}) && y.n_stack == 335);
        CHECK(db == (Offs{0, 0, 6, 153, 301}) && y.n_db == 307);
        CHECK(code == pk.code_off && L == (Ints{0, 5, 146, 147, 5}));
        CHECK(flat(y.plan) == (Sizes{0, 1}) && y.plan.max_cost == 3 * 147 * 147 * 4 && tab_offs(y.qs) == (Offs{0, 0, 0, 0, 0}));
    }
    {   // lds_len 4: everything in the HBM class, in input order; tables of 3 L^2 ints: 300, 255792, 259308, 300 bytes
        MfeLayout y = mfe_layout(pk, 4, 1 << 30);
        CHECK(y.lds_order.empty() && y.hbm_order == (Ints{1, 2, 3, 4}) && y.order == y.hbm_order);
        CHECK(flat(y.plan) == (Sizes{0, 4}) && y.plan.off == (Sizes{0, 300, 256092, 515400}) && y.plan.max_cost == 515700);
        CHECK(tab_offs(y.qs) == (Offs{0, 0, 75, 64023, 128850}));
        y = mfe_layout(pk, 4, 259608);                              // the last two, not the first three: the tables start again in the second chunk
        CHECK(flat(y.plan) == (Sizes{0, 2, 2, 4}) && y.plan.max_cost == 259608 && tab_offs(y.qs) == (Offs{0, 0, 75, 0, 64827}));
        CHECK(y.qs[3].stack_off == 167 && y.qs[4].db_off == 301);  // ... the stacks and rows do not
        y = mfe_layout(pk, 5, 1 << 30);                             // a length equal to lds_len is in the LDS class
        CHECK(y.lds_order == (Ints{1, 4}) && y.hbm_order == (Ints{2, 3}) && y.order == (Ints{1, 4, 2, 3}) && tab_offs(y.qs) == (Offs{0, 0, 0, 63948, 0}));
    }
    {   // an error between two sequences stands where the next one starts
        const MfeLayout y = mfe_layout(pack_of({5, 0, 5}), 146, 1 << 30);
        CHECK(y.qs[1].stack_off == 13 && y.qs[2].stack_off == 13 && y.qs[1].db_off == 6 && y.qs[2].db_off == 6 && y.qs[1].L == 0);
        CHECK(y.n_stack == 26 && y.n_db == 12 && y.lds_order == (Ints{0, 2}));
        const MfeLayout none = mfe_layout(pack_of({0, 0}), 146, 1 << 30);
        CHECK(none.order.empty() && none.plan.chunks.empty() && none.plan.max_cost == 0 && none.n_stack == 0 && none.n_db == 0 && none.qs.size() == 2);
    }
}

static void check_pf_layout()
{
    const SeqPack pk = pack_of({0, 5, 7, 0, 6});
    CHECK(pk.fold == (Ints{1, 2, 4}));
    // ps, pb, F, Fr of L + 1 doubles each: 24, 32, 28; rows of L + 1 bytes: 6, 8, 7; the errors take nothing
    PfLayout y = pf_layout(pk, 3, nullptr, 1 << 30);
    Offs aux, db;
    for (const PfSeq &q : y.qs) { aux.push_back(q.aux_off); db.push_back(q.db_off); CHECK(q.mfe_dcal == 0 && q.scale == 0.0 && q.ln_scale == 0.0); }
    CHECK(aux == (Offs{0, 0, 24, 56, 56}) && y.n_aux == 84 && db == (Offs{0, 0, 6, 14, 14}) && y.n_db == 21);
    CHECK(y.qs[0].L == 0 && y.qs[1].L == 5 && y.qs[2].L == 7 && y.qs[3].L == 0 && y.qs[4].L == 6 && y.qs[4].code_off == 12);
    // three tables of L^2 doubles: 600, 1176, 864 bytes; tab_off counts doubles
    CHECK(flat(y.plan) == (Sizes{0, 3}) && y.plan.off == (Sizes{0, 600, 1776}) && y.plan.max_cost == 2640 && tab_offs(y.qs) == (Offs{0, 0, 75, 0, 222}));
    y = pf_layout(pk, 6, nullptr, 1 << 30);                          // six: 1200, 2352, 1728
    CHECK(flat(y.plan) == (Sizes{0, 3}) && y.plan.max_cost == 5280 && tab_offs(y.qs) == (Offs{0, 0, 150, 0, 444}) && y.n_aux == 84 && y.n_db == 21);
    y = pf_layout(pk, 3, nullptr, 1776);                             // 600 + 1176 is not over 1776
    CHECK(flat(y.plan) == (Sizes{0, 2, 2, 3}) && tab_offs(y.qs) == (Offs{0, 0, 75, 0, 0}) && y.plan.max_cost == 1776);
    y = pf_layout(pk, 6, nullptr, 1776);                             // ... 1200 + 2352 is
    CHECK(flat(y.plan) == (Sizes{0, 1, 1, 2, 2, 3}) && tab_offs(y.qs) == (Offs{0, 0, 0, 0, 0}) && y.plan.max_cost == 2352);
    const size_t cost2[3] = {2000, 1000, 10};                        // the tables of all three fit 2640, 2000 + 1000 does not: the second cost cuts
    y = pf_layout(pk, 3, cost2, 2640);
    CHECK(flat(y.plan) == (Sizes{0, 1, 1, 3}) && tab_offs(y.qs) == (Offs{0, 0, 0, 0, 147}) && y.plan.max_cost == 2040 && y.plan.max_cost2 == 2000);
    CHECK(y.qs[4].aux_off == 56 && y.qs[4].db_off == 14);         // (aux and rows are the whole call's, not a chunk's)
}

// the scale of a partition function (pf_temp, pf_set_scale), bit for bit against the formula of DESIGN.md section 10 spelled out
static void check_pf_scale()
{
    volatile double temp_in = 37.0;                                  // (volatile: both sides call exp and log at run time)
    volatile int L_in = 77, dcal_in = -2470;
    const double temp = temp_in, kt = (temp + 273.15) * 1.98717e-3, beta = 1.0 / (100.0 * kt);
    const PfTemp t = pf_temp(temp);
    CHECK(t.kt == kt && t.beta == beta);
    PfSeq none{0, 0, 0, 0, 0, 7, 5.0, 5.0};                          // L = 0: the exponent is 0 whatever the MFE says
    pf_set_scale(none, -1230, kt, 0.0);
    CHECK(none.mfe_dcal == -1230 && none.scale == std::exp(0.0) && none.ln_scale == std::log(std::exp(0.0)) && none.scale == 1.0 && none.ln_scale == 0.0);
    const int L = L_in, dcal = dcal_in;
    for (const double scale_factor : {0.0, 1.3}) {                   // 0: the default, 1.07
        const double sf = scale_factor > 0.0 ? scale_factor : 1.07;
        const double ln_scale = -sf * ((double)dcal / 100.0) / (kt * (double)L), scale = std::exp(ln_scale);
        PfSeq q{0, 0, 0, 0, L, 0, 0.0, 0.0};
        PfSpanSeq b{0, 0, 0, 0, 0, L, 30, 0, 0, 0.0, 0.0};
        pf_set_scale(q, dcal, kt, scale_factor);
        pf_set_scale(b, dcal, kt, scale_factor);
        CHECK(q.mfe_dcal == dcal && q.scale == scale && q.ln_scale == std::log(scale) && q.scale > 1.0);
        CHECK(b.mfe_dcal == dcal && b.scale == scale && b.ln_scale == std::log(scale));
    }
}

static void check_sample_layout()
{
    const SeqPack pk = pack_of({0, 5, 7, 0, 6});
    const unsigned long long seeds[5] = {10, 11, 12, 13, 14};
    CHECK(sample_row_costs(pk, 3) == (Sizes{18, 24, 21}));           // three rows of L + 1 bytes
    auto fields = [](const SampleLayout &y) { Offs v; for (const SampleSeq &q : y.smp) { v.push_back(q.seed); v.push_back(q.row_off); v.push_back(q.dcal_off); } return v; };
    // one chunk of three: rows back to back, the energies of the chunk's k-th sequence from int 3 k; the errors keep zeros
    SampleLayout y = sample_layout(pk, pf_layout(pk, 3, nullptr, 1 << 30).plan, 3, seeds);
    CHECK(y.row_bytes == (Sizes{18, 24, 21}) && y.max_seqs == 3);
    CHECK(fields(y) == (Offs{0, 0, 0, 11, 0, 0, 12, 18, 3, 0, 0, 0, 14, 42, 6}));
    // chunks [0, 2) and [2, 3) (the tables cut, as in check_pf_layout): rows and energies start again at 0
    const ChunkPlan two = pf_layout(pk, 3, y.row_bytes.data(), 1776).plan;
    CHECK(flat(two) == (Sizes{0, 2, 2, 3}) && two.max_cost2 == 42);
    y = sample_layout(pk, two, 3, seeds);
    CHECK(y.max_seqs == 2 && fields(y) == (Offs{0, 0, 0, 11, 0, 0, 12, 18, 3, 0, 0, 0, 14, 0, 0}));
    y = sample_layout(pk, two, 3, nullptr);                          // no seeds: every seed 0
    CHECK(fields(y) == (Offs{0, 0, 0, 0, 0, 0, 0, 18, 3, 0, 0, 0, 0, 0, 0}));
    y = sample_layout(pk, two, 0, seeds);                            // no samples: no bytes
    CHECK(y.row_bytes == (Sizes{0, 0, 0}) && y.max_seqs == 2 && fields(y) == (Offs{0, 0, 0, 11, 0, 0, 12, 0, 0, 0, 0, 0, 14, 0, 0}));
    y = sample_layout(pack_of({0}), ChunkPlan{}, 3, seeds);
    CHECK(y.row_bytes.empty() && y.max_seqs == 0 && y.smp.size() == 1);
}

static void check_subopt_layout()
{
    // a state: 16 bytes of numbers, a stack of L / 5 + 2 words rounded up to 4, a row of L + 1 bytes rounded up to 16
    //   L = 80: 16 + 4 * 20 (18 -> 20) + 96 (81 -> 96) = 192      L = 9: 16 + 4 * 4 (3 -> 4) + 16 (10 -> 16) = 48
    //   L = 79: 16 + 4 * 20 (17 -> 20) + 80 (80 -> 80) = 176      L = 1, 4, 5: 16 + 4 * 4 (2, 2, 3 -> 4) + 16 (2, 5, 6 -> 16) = 48
    CHECK(subopt_state_bytes(80) == 192 && subopt_state_bytes(9) == 48 && subopt_state_bytes(79) == 176);
    CHECK(subopt_state_bytes(1) == 48 && subopt_state_bytes(4) == 48 && subopt_state_bytes(5) == 48);
    CHECK(seg_stack_words(80) == 20 && row_bytes16(80) == 96 && row_bytes16(79) == 80 && row_bytes16(15) == 16 && row_bytes16(16) == 32);
    CHECK(sample_lds_bytes(80) == 4 * (96 + 80));
    const Ints lens = {1, 4, 5, 0, 79, 80};                          // an error between them
    const size_t state[6] = {48, 48, 48, 0, 176, 192};
    const SeqPack pk = pack_of(lens);
    CHECK(pk.fold == (Ints{0, 1, 2, 4, 5}));
    for (int M : {1, 63, 64, 65}) {
        const size_t cnt = M <= 64 ? 256 : 512;                      // M counts of 4 bytes, rounded up to 256
        // tables of 3 L^2 ints: 12, 192, 300, 74892, 76800 bytes.  Everything in one chunk; then a budget that holds the first four
        // tables (75396) but not the fifth, the frontiers (at most 3 * 6752 + 23392 = 43648) staying below it
        for (size_t budget : {(size_t)1 << 30, (size_t)80000}) {
            const bool cut = budget == 80000;
            const SuboptLayout y = subopt_layout(pk, M, budget);
            CHECK(y.tab_bytes == (Sizes{12, 192, 300, 74892, 76800}));
            CHECK(flat(y.plan) == (cut ? Sizes{0, 4, 4, 5} : Sizes{0, 5}) && y.max_seqs == (cut ? 4u : 5u));
            CHECK(tab_offs(y.qs) == (cut ? Offs{0, 3, 51, 0, 126, 0} : Offs{0, 3, 51, 0, 126, 18849}));
            CHECK(y.qs.size() == 6 && y.mq.size() == 6 && y.n_f == 174);
            size_t at = 0, total = 0;
            unsigned long long f = 0;
            for (size_t k = 0; k < pk.fold.size(); k++) {
                const int s = pk.fold[k];
                const SuboptSeq &q = y.qs[s];
                if (cut && k == 4) at = 0;                           // the frontiers of a chunk start at byte 0 ...
                CHECK(y.front_bytes[k] == 2 * (size_t)M * state[s] + cnt);
                CHECK(q.buf_off[0] == at && q.buf_off[1] - q.buf_off[0] == (size_t)M * state[s]);
                CHECK(q.cnt_off * 4 == q.buf_off[1] + (size_t)M * state[s]);          // the counts lie exactly behind the second buffer
                CHECK(q.cnt_off * 4 + 4 * (size_t)M <= at + y.front_bytes[k]);        // ... and end before the next sequence starts
                CHECK(q.f_off == f && q.L == lens[s] && q.code_off == pk.code_off[s] && q.pad == 0);     // ... the exterior energies go on
                const MfeSeq &m = y.mq[s];                           // what the table fill reads is the same sequence
                CHECK(m.code_off == q.code_off && m.tab_off == q.tab_off && m.L == q.L && m.stack_off == 0 && m.db_off == 0 && m.pad == 0);
                at += y.front_bytes[k]; f += (unsigned long long)lens[s] + 1;
                total = std::max(total, at);
            }
            CHECK(y.plan.max_cost2 == total);
            const SuboptSeq &e = y.qs[3];
            CHECK(e.L == 0 && e.code_off == 0 && e.tab_off == 0 && e.f_off == 0 && e.buf_off[0] == 0 && e.buf_off[1] == 0 && e.cnt_off == 0 && y.mq[3].L == 0);
        }
        // the packed copy of n <= M finished states - n rows, then n energies - fits the buffer of M states it is written into
        for (int L : {1, 4, 5, 79, 80})
            for (int n = 0; n <= M; n++) {
                CHECK(subopt_pack_dcal_off(n, L) >= (unsigned long long)n * (L + 1) && subopt_pack_dcal_off(n, L) % 16 == 0);
                CHECK(subopt_pack_dcal_off(n, L) + 4ull * n <= (unsigned long long)M * subopt_state_bytes(L));
            }
    }
    CHECK(subopt_pack_dcal_off(1, 1) == 16 && subopt_pack_dcal_off(64, 80) == 5184 && subopt_pack_dcal_off(63, 79) == 5040);
    {   // the frontiers cut a chunk the tables would not: 2 * 64 * 48 + 256 = 6400 each, 192 + 300 bytes of tables
        const SuboptLayout y = subopt_layout(pack_of({4, 5}), 64, 12000);
        CHECK(flat(y.plan) == (Sizes{0, 1, 1, 2}) && y.max_seqs == 1 && y.plan.max_cost == 300 && y.plan.max_cost2 == 6400);
        CHECK(y.qs[1].buf_off[0] == 0 && y.qs[1].buf_off[1] == 3072 && y.qs[1].cnt_off == 1536 && y.qs[1].tab_off == 0 && y.qs[1].f_off == 5);
        const SuboptLayout z = subopt_layout(pack_of({4, 5}), 64, 12800);
        CHECK(flat(z.plan) == (Sizes{0, 2}) && z.qs[1].buf_off[0] == 6400 && z.qs[1].cnt_off == 3136 && z.qs[1].tab_off == 48);
    }
}

int main()
{
    check_lanes();
    check_parsers();
    check_enclosing_loop();
    check_score_layout();
    check_chunk_planner();
    check_sequence_pack();
    check_graph_pack();
    check_solve_order();
    check_chunk_lmax();
    check_mfe_layout();
    check_pf_layout();
    check_pf_scale();
    check_sample_layout();
    check_subopt_layout();
    printf("hostpure: %d failures\n", fails);
    return fails ? 1 : 0;
}
