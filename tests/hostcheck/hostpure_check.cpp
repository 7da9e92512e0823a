// Host-side check of rafft_amd/csrc/rafft_hostpure.h: the lane cut of a batch, the dot-bracket parsers, the base codes, the
// enclosing-loop walk and the row layout of the scoring calls, against values derived by hand from the rules.  Plain C++, no
// HIP, no GPU.  Test infrastructure.
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

int main()
{
    check_lanes();
    check_parsers();
    check_enclosing_loop();
    check_score_layout();
    printf("hostpure: %d failures\n", fails);
    return fails ? 1 : 0;
}
