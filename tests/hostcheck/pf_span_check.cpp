// Host-side check of the banded partition function's part of rafft_amd/csrc/rafft_hostpure.h: the layout of a rafft_pf_span_batch
// call (pf_span_layout) - offsets disjoint and 8-byte aligned, the byte count of a sequence as the comments of
// rafft_batch_layout.h and include/rafft_hip.h give it, chunks at the edges of the workspace budget, and the largest sequence at the
// widest span without an overflow of size_t arithmetic - against values derived by hand.  Plain C++, no HIP, no GPU.
// usage: pf_span_check.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0, cases = 0;
#define CHECK(c) do { cases++; if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

// 48 L W + 8 (3 L + 2 W + 6) + 8 (L + 1) + L + 1, as the header comment states it
static unsigned long long stated_bytes(unsigned long long L, unsigned long long W) { return 48 * L * W + 8 * (3 * L + 2 * W + 6) + 8 * (L + 1) + L + 1; }

static void check_sizes()
{
    CHECK(sizeof(PfSpanSeq) == 72 && PF_SPAN_TABLES == 6);
    CHECK(PF_SPAN_RING == RAFFT_MFE_MAX_LEN && (PF_SPAN_RING & (PF_SPAN_RING - 1)) == 0 && PF_SPAN_RING * 12 == 48 << 10);
    CHECK(pf_span_table_doubles(32768, 4096) == 1ull << 27);
    CHECK(pf_span_aux_doubles(10, 8) == 2 * 10 + 2 * 11 + 10 && pf_span_exp_ints(10) == 22 && pf_span_exp_ints(9) % 2 == 0);
    for (int L : {1, 9, 10, 150, 4097, 32768})
        for (int span : {1, 4, 5, 150, 4096}) {
            const int W = mfe_span_width(L, span);
            CHECK(pf_span_seq_bytes(L, W) == stated_bytes((unsigned long long)L, (unsigned long long)W));
        }
    CHECK(pf_span_seq_bytes(32768, 150) == 237013401ull);                            // 226 MiB
    CHECK(pf_span_seq_bytes(32768, 4096) == 6ull * 8 * 32768 * 4096 + 8 * (3 * 32768 + 2 * 4096 + 6) + 8 * 32769 + 32769);
}

// the arrays of every folded sequence within each buffer: [first, last) in bytes, sorted by first as the layout deals them out
static void check_disjoint(const SeqPack &pk, const PfSpanLayout &y)
{
    unsigned long long aux_end = 0, exp_end = 0, db_end = 0;
    for (int s : pk.fold) {
        const PfSpanSeq &q = y.qs[s];
        CHECK(q.aux_off * 8 == aux_end && q.exp_off * 4 == exp_end && q.db_off == db_end);
        CHECK((q.tab_off * 8) % 8 == 0 && (q.aux_off * 8) % 8 == 0 && (q.exp_off * 4) % 8 == 0);
        aux_end += 8 * pf_span_aux_doubles(q.L, q.W); exp_end += 4 * pf_span_exp_ints(q.L); db_end += (unsigned long long)q.L + 1;
    }
    CHECK(aux_end == 8 * y.n_aux && exp_end == 4 * y.n_exp && db_end == y.n_db);
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        unsigned long long end = 0;
        for (size_t k = c.a; k < c.b; k++) {
            const PfSpanSeq &q = y.qs[pk.fold[k]];
            CHECK(q.tab_off * 8 == end);
            end += 8 * PF_SPAN_TABLES * pf_span_table_doubles(q.L, q.W);
        }
        CHECK(end <= y.plan.max_cost);
    }
}

static void check_layout()
{
    const char *seqs[6] = {"GGGAAACCCA", "", "ACGUACGUACGUACGUACGU", "GGX", "GGGAAACCC", "GGGAAACCCA"};
    const int lens[6] = {10, 0, 20, 3, 9, 10};
    const SeqPack pk = pack_sequences(6, seqs, lens, RAFFT_MFE_SPAN_MAX_LEN, "RAFFT_MFE_SPAN_MAX_LEN");
    CHECK(pk.fold.size() == 4 && pk.first_err == "sequence 1: empty");
    const size_t t10 = 6 * 10 * 10 * 8, t20 = 6 * 20 * 12 * 8, t9 = 6 * 9 * 9 * 8;      // span 12: W = 10, 12, 9, 10
    {   // everything fits: one chunk
        const PfSpanLayout y = pf_span_layout(pk, 12, 1 << 20);
        CHECK(y.qs.size() == 6 && y.qs[0].W == 10 && y.qs[2].W == 12 && y.qs[4].W == 9 && y.qs[5].W == 10 && y.qs[1].L == 0 && y.qs[3].L == 0);
        CHECK(y.plan.chunks.size() == 1 && y.plan.chunks[0].a == 0 && y.plan.chunks[0].b == 4 && y.plan.max_cost == 2 * t10 + t20 + t9);
        CHECK(y.qs[0].tab_off == 0 && y.qs[2].tab_off == 600 && y.qs[4].tab_off == 600 + 1440 && y.qs[5].tab_off == 600 + 1440 + 486);
        // aux: 2 (W + 2) + 2 (L + 1) + L doubles: 56 for (10, 10), 90 for (20, 12), 51 for (9, 9)
        CHECK(y.qs[0].aux_off == 0 && y.qs[2].aux_off == 56 && y.qs[4].aux_off == 146 && y.qs[5].aux_off == 197 && y.n_aux == 253);
        CHECK(y.qs[2].exp_off == 22 && y.qs[4].exp_off == 64 && y.qs[5].exp_off == 84 && y.n_exp == 106);
        CHECK(y.qs[2].db_off == 11 && y.qs[5].db_off == 42 && y.n_db == 53);
        CHECK(y.qs[2].code_off == 10 && y.qs[4].code_off == 30);
        CHECK(chunk_wmax(y.plan.chunks[0], pk.fold, y.qs) == 12 && chunk_lmax(y.plan.chunks[0], pk.fold, pk.L) == 20);
        check_disjoint(pk, y);
    }
    {   // exactly fitting: 10 and 20 together, then 9 and 10; one byte less: 10 alone, 20 with 9, 10 alone
        const PfSpanLayout y = pf_span_layout(pk, 12, t10 + t20);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2 && y.plan.chunks[1].b == 4 && y.qs[4].tab_off == 0 && y.qs[5].tab_off == 486);
        CHECK(chunk_wmax(y.plan.chunks[1], pk.fold, y.qs) == 10);
        CHECK(y.qs[4].aux_off == 146);                                                  // (what is not in the workspace is laid out for the whole call)
        check_disjoint(pk, y);
        const PfSpanLayout z = pf_span_layout(pk, 12, t10 + t20 - 1);
        CHECK(z.plan.chunks.size() == 3 && z.plan.chunks[0].b == 1 && z.plan.chunks[1].b == 3 && z.qs[2].tab_off == 0 && z.qs[4].tab_off == 1440 && z.qs[5].tab_off == 0);
        CHECK(z.plan.max_cost == t20 + t9);
        check_disjoint(pk, z);
    }
    {   // a workspace of one byte: one sequence a chunk, each at offset 0
        const PfSpanLayout y = pf_span_layout(pk, 12, 1);
        CHECK(y.plan.chunks.size() == 4 && y.plan.max_cost == t20);
        for (int s : pk.fold) CHECK(y.qs[s].tab_off == 0);
        check_disjoint(pk, y);
    }
    {   // spans of 1 and of the maximum
        const PfSpanLayout y = pf_span_layout(pk, 1, 1 << 20);
        CHECK(y.qs[2].W == 1 && y.plan.max_cost == 6 * (10 + 20 + 9 + 10) * 8);
        const PfSpanLayout z = pf_span_layout(pk, RAFFT_MFE_MAX_LEN, 1 << 20);
        CHECK(z.qs[2].W == 20 && z.qs[4].W == 9);
        check_disjoint(pk, z);
    }
}

static void check_limit()
{
    std::vector<char> big(RAFFT_MFE_SPAN_MAX_LEN + 1, 'A');
    const char *seqs[3] = {big.data(), big.data(), "GGGAAACCC"};
    const int lens[3] = {RAFFT_MFE_SPAN_MAX_LEN, RAFFT_MFE_SPAN_MAX_LEN + 1, 9};
    const SeqPack pk = pack_sequences(3, seqs, lens, RAFFT_MFE_SPAN_MAX_LEN, "RAFFT_MFE_SPAN_MAX_LEN");
    CHECK(pk.status[0] == 0 && pk.status[1] == RAFFT_ERR_TOO_LONG && pk.status[2] == 0 && pk.L[1] == 0);
    // the largest sequence at the widest span is a chunk of its own, 6 GiB, whatever the budget: beyond 32 bits, exact in size_t
    static_assert(sizeof(size_t) == 8, "the table bytes of one sequence need 64 bits");
    const PfSpanLayout y = pf_span_layout(pk, RAFFT_MFE_MAX_LEN, (size_t)512 << 20);
    CHECK(y.plan.chunks.size() == 2 && y.plan.max_cost == (size_t)6 * 32768 * 4096 * 8 && y.plan.max_cost == (size_t)6 << 30 && y.qs[0].W == 4096 && y.qs[2].tab_off == 0);
    CHECK(y.qs[0].tab_off + 6 * pf_span_table_doubles(32768, 4096) == 6ull << 27);   // one past its last double
    CHECK(y.n_aux == pf_span_aux_doubles(32768, 4096) + pf_span_aux_doubles(9, 9) && y.qs[2].aux_off == 2 * 4098 + 2 * 32769 + 32768);
    CHECK(y.n_exp == 2 * 32769 + 20 && y.qs[2].exp_off == 65538 && y.qs[2].db_off == 32769);
    check_disjoint(pk, y);
    const PfSpanLayout z = pf_span_layout(pk, 150, (size_t)512 << 20);
    CHECK(z.plan.chunks.size() == 1 && z.plan.max_cost == (size_t)6 * 32768 * 150 * 8 + 6 * 81 * 8 && z.qs[2].tab_off == 6ull * 32768 * 150);
    check_disjoint(pk, z);
}

int main()
{
    check_sizes();
    check_layout();
    check_limit();
    printf("%d checks, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
