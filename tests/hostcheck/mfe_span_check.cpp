// Host-side check of the span part of rafft_amd/csrc/rafft_hostpure.h: the layout of a rafft_mfe_span_batch call
// (mfe_span_layout) at the edges of the workspace budget and of the length limit, the sizes of rafft_batch_layout.h, the stack
// word's fields and the text pack_sequences gives a sequence over the limit, against values derived by hand.  Plain C++, no HIP,
// no GPU.  usage: mfe_span_check.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0, cases = 0;
#define CHECK(c) do { cases++; if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static void check_sizes()
{
    CHECK(sizeof(MfeSpanSeq) == 48 && MFE_SPAN_TABLES == 4);
    CHECK(RAFFT_MFE_SPAN_MAX_LEN == 32768 && RAFFT_MFE_SPAN_MAX_LEN == RAFFT_MAX_LEN);
    CHECK(mfe_span_width(9, 40) == 9 && mfe_span_width(40, 40) == 40 && mfe_span_width(41, 40) == 40 && mfe_span_width(32768, 1) == 1);
    CHECK(mfe_span_table_ints(32768, 4096) == 1ull << 27);
    // i | d << 15 | table << 30: the largest position, the largest d of a band, three tables
    CHECK(RAFFT_MFE_SPAN_MAX_LEN - 1 < (1 << 15) && RAFFT_MFE_MAX_LEN - 1 < (1 << 15));
    CHECK(((32767u | 4095u << 15 | 2u << 30) >> 30) == 2u && ((32767u | 4095u << 15 | 2u << 30) & 32767u) == 32767u);
    // F and the pair table over it fit the 160 KiB of LDS a workgroup may have
    CHECK(mfe_span_lds_bytes(1) == 8 && mfe_span_lds_bytes(RAFFT_MFE_SPAN_MAX_LEN) == 131076 && mfe_span_lds_bytes(RAFFT_MFE_SPAN_MAX_LEN) <= 160 << 10);
}

static void check_layout()
{
    const char *seqs[6] = {"GGGAAACCCA", "", "ACGUACGUACGUACGUACGU", "GGX", "GGGAAACCC", "GGGAAACCCA"};
    const int lens[6] = {10, 0, 20, 3, 9, 10};
    const SeqPack pk = pack_sequences(6, seqs, lens, RAFFT_MFE_SPAN_MAX_LEN, "RAFFT_MFE_SPAN_MAX_LEN");
    CHECK(pk.fold.size() == 4 && pk.first_err == "sequence 1: empty");
    const size_t t10 = 4 * 10 * 10 * 4, t20 = 4 * 20 * 12 * 4, t9 = 4 * 9 * 9 * 4;      // span 12: W = 10, 12, 9, 10
    {   // everything fits: one chunk
        const MfeSpanLayout y = mfe_span_layout(pk, 12, 1 << 20);
        CHECK(y.qs.size() == 6 && y.qs[0].W == 10 && y.qs[2].W == 12 && y.qs[4].W == 9 && y.qs[5].W == 10 && y.qs[1].L == 0 && y.qs[3].L == 0);
        CHECK(y.plan.chunks.size() == 1 && y.plan.chunks[0].a == 0 && y.plan.chunks[0].b == 4 && y.plan.max_cost == 2 * t10 + t20 + t9);
        CHECK(y.qs[0].tab_off == 0 && y.qs[2].tab_off == 400 && y.qs[4].tab_off == 400 + 960 && y.qs[5].tab_off == 400 + 960 + 324);
        CHECK(y.qs[0].f_off == 0 && y.qs[2].f_off == 11 && y.qs[4].f_off == 32 && y.qs[5].f_off == 42 && y.n_f == 53);
        CHECK(y.qs[2].stack_off == 18 && y.qs[4].stack_off == 46 && y.qs[5].stack_off == 63 && y.n_stack == 81);
        CHECK(y.qs[2].db_off == 11 && y.qs[5].db_off == 42 && y.n_db == 53);
        CHECK(y.qs[2].code_off == 10 && y.qs[4].code_off == 30);
        const ChunkPlan::Range c = y.plan.chunks[0];
        CHECK(chunk_wmax(c, pk.fold, y.qs) == 12 && chunk_lmax(c, pk.fold, pk.L) == 20);
    }
    {   // exactly fitting: 10 and 20 together, then 9 and 10; one byte less: 10 alone, 20 with 9, 10 alone
        const MfeSpanLayout y = mfe_span_layout(pk, 12, t10 + t20);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2 && y.plan.chunks[1].b == 4 && y.qs[4].tab_off == 0 && y.qs[5].tab_off == 324);
        CHECK(chunk_wmax(y.plan.chunks[1], pk.fold, y.qs) == 10);
        CHECK(y.qs[4].f_off == 32);                                                     // (what is not in the workspace is laid out for the whole call)
        const MfeSpanLayout z = mfe_span_layout(pk, 12, t10 + t20 - 1);
        CHECK(z.plan.chunks.size() == 3 && z.plan.chunks[0].b == 1 && z.plan.chunks[1].b == 3 && z.qs[2].tab_off == 0 && z.qs[4].tab_off == 960 && z.qs[5].tab_off == 0);
        CHECK(z.plan.max_cost == t20 + t9);
    }
    {   // a workspace of one byte: one sequence a chunk, each at offset 0
        const MfeSpanLayout y = mfe_span_layout(pk, 12, 1);
        CHECK(y.plan.chunks.size() == 4 && y.plan.max_cost == t20);
        for (int s : pk.fold) CHECK(y.qs[s].tab_off == 0);
    }
    {   // spans of 1 and of the maximum
        const MfeSpanLayout y = mfe_span_layout(pk, 1, 1 << 20);
        CHECK(y.qs[2].W == 1 && y.plan.max_cost == 4 * (10 + 20 + 9 + 10) * 4);
        const MfeSpanLayout z = mfe_span_layout(pk, RAFFT_MFE_MAX_LEN, 1 << 20);
        CHECK(z.qs[2].W == 20 && z.qs[4].W == 9);
    }
}

static void check_limit()
{
    std::vector<char> big(RAFFT_MFE_SPAN_MAX_LEN + 1, 'A');
    const char *seqs[3] = {big.data(), big.data(), "GGGAAACCC"};
    const int lens[3] = {RAFFT_MFE_SPAN_MAX_LEN, RAFFT_MFE_SPAN_MAX_LEN + 1, 9};
    const SeqPack pk = pack_sequences(3, seqs, lens, RAFFT_MFE_SPAN_MAX_LEN, "RAFFT_MFE_SPAN_MAX_LEN");
    CHECK(pk.status[0] == 0 && pk.status[1] == RAFFT_ERR_TOO_LONG && pk.status[2] == 0 && pk.len[1] == RAFFT_MFE_SPAN_MAX_LEN + 1 && pk.L[1] == 0);
    CHECK(pk.first_err == "sequence 1: longer than RAFFT_MFE_SPAN_MAX_LEN");
    // the text of the callers that name no limit is what it was
    CHECK(pack_sequences(3, seqs, lens, RAFFT_MFE_MAX_LEN).first_err == "sequence 0: longer than RAFFT_MFE_MAX_LEN");
    // the largest sequence at the widest span is a chunk of its own, 2 GiB, whatever the budget; offsets in ints stay exact
    const MfeSpanLayout y = mfe_span_layout(pk, RAFFT_MFE_MAX_LEN, (size_t)512 << 20);
    CHECK(y.plan.chunks.size() == 2 && y.plan.max_cost == (size_t)4 * 32768 * 4096 * 4 && y.qs[0].W == 4096 && y.qs[2].tab_off == 0);
    CHECK(y.n_f == 32769 + 10 && y.qs[2].f_off == 32769 && y.qs[2].stack_off == 32776);
    const MfeSpanLayout z = mfe_span_layout(pk, 150, (size_t)512 << 20);
    CHECK(z.plan.chunks.size() == 1 && z.plan.max_cost == (size_t)4 * 32768 * 150 * 4 + 4 * 81 * 4 && z.qs[2].tab_off == 4ull * 32768 * 150);
}

int main()
{
    check_sizes();
    check_layout();
    check_limit();
    printf("%d checks, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
