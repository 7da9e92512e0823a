// Host-side check of rafft_amd/csrc/rafft_hostpure.h: the lane cut of a batch, the dot-bracket parsers, the base codes, the
// enclosing-loop walk, the row layout of the scoring calls and the planning of the batch drivers (chunk planner, sequence pack,
// graph pack, solve order), against values derived by hand from the rules.  Plain C++, no HIP, no GPU.  Test infrastructure.
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
    printf("hostpure: %d failures\n", fails);
    return fails ? 1 : 0;
}
