// Host-side check of the MEA part of rafft_amd/csrc/rafft_hostpure.h: the layout of a rafft_mea_probs_batch call
// (mea_probs_layout) at the edges of the workspace budget, the records of rafft_mea_batch over a pf_layout (mea_layout), the sizes
// of rafft_batch_layout.h and the entry check of a matrix (mea_probs_bad_entry), against values derived by hand.  Plain C++, no
// HIP, no GPU.  usage: mea_check.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0, cases = 0;
#define CHECK(c) do { cases++; if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static void check_sizes()
{
    CHECK(sizeof(rafft_mea_seq) == 48 && sizeof(rafft_mea_probs_seq) == 32);
    CHECK(sizeof(MeaSeq) == 72 && sizeof(MeaRec) == 24);
    CHECK(mea_aux_doubles(1) == 4 && mea_aux_doubles(4096) == 8194 && mea_stack_words(1) == 9 && mea_stack_words(4096) == 4104);
    for (int L = 1; L <= 4096; L++) {
        CHECK(mea_aux_doubles(L) <= 4ull * ((unsigned long long)L + 1));        // q, the shares and the diversity fit where ps, pb, F, Fr lay
        CHECK(mea_stack_words(L) >= (unsigned long long)L / 2 + 2);             // a pair leaves at most one interval more behind
    }
    CHECK(RAFFT_PF_MAX_LEN <= 0xffff && RAFFT_PF_MAX_LEN <= 32767);             // (i | j << 16 of an interval; int16 pair tables)
}

static void check_probs_layout()
{
    const int lens[6] = {10, 0, 20, 4097, 9, 10};
    const size_t t10 = 4 * 100 * 8, t20 = 4 * 400 * 8, t9 = 4 * 81 * 8;
    {   // everything fits: one chunk of the four matrices without an error
        const MeaProbsLayout y = mea_probs_layout(6, lens, 1 << 20);
        CHECK(y.status[0] == 0 && y.status[1] == RAFFT_ERR_EMPTY && y.status[3] == RAFFT_ERR_TOO_LONG && y.status[5] == 0);
        CHECK(y.len[1] == 0 && y.len[3] == 4097 && y.L[3] == 0 && y.L[2] == 20);
        CHECK(y.order.size() == 4 && y.order[0] == 0 && y.order[1] == 2 && y.order[2] == 4 && y.order[3] == 5);
        CHECK(y.first_err.rfind("sequence 1:", 0) == 0);
        CHECK(y.plan.chunks.size() == 1 && y.plan.chunks[0].a == 0 && y.plan.chunks[0].b == 4 && y.plan.max_cost == 2 * t10 + t20 + t9);
        CHECK(y.qs[0].p_off == 0 && y.qs[0].wt_off == 100 && y.qs[0].e_off == 200 && y.qs[0].et_off == 300);
        CHECK(y.qs[2].p_off == 400 && y.qs[2].wt_off == 800 && y.qs[2].et_off == 1600 && y.qs[4].p_off == 2000 && y.qs[5].p_off == 2000 + 324);
        CHECK(y.qs[0].aux_off == 0 && y.qs[2].aux_off == 22 && y.qs[4].aux_off == 22 + 42 && y.qs[5].aux_off == 22 + 42 + 20 && y.n_aux == 22 + 42 + 20 + 22);
        CHECK(y.qs[2].stack_off == 18 && y.qs[4].stack_off == 18 + 28 && y.n_stack == 18 + 28 + 17 + 18);
        CHECK(y.qs[2].pt_off == 10 && y.qs[4].pt_off == 30 && y.n_pt == 49 && y.qs[2].db_off == 11 && y.qs[5].db_off == 11 + 21 + 10 && y.n_db == 11 + 21 + 10 + 11);
        CHECK(y.qs[1].L == 0 && y.qs[3].L == 0 && y.qs[5].L == 10);
    }
    {   // exactly fitting: 10 and 20 together, then 9 and 10
        const MeaProbsLayout y = mea_probs_layout(6, lens, t10 + t20);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2 && y.plan.chunks[1].a == 2 && y.plan.chunks[1].b == 4 && y.plan.max_cost == t10 + t20);
        CHECK(y.qs[2].p_off == 400 && y.qs[4].p_off == 0 && y.qs[5].p_off == 324 && y.qs[5].et_off == 324 + 300);
        CHECK(y.qs[4].aux_off == 22 + 42);                                      // (what is not in the workspace is laid out for the whole call)
        const MeaProbsLayout z = mea_probs_layout(6, lens, t10 + t20 - 1);      // one byte less: the first alone, 20 with 9, the last alone
        CHECK(z.plan.chunks.size() == 3 && z.plan.chunks[0].b == 1 && z.plan.chunks[1].b == 3 && z.qs[2].p_off == 0 && z.qs[4].p_off == 1600 && z.qs[5].p_off == 0);
        CHECK(z.plan.max_cost == t20 + t9);
    }
    {   // every matrix larger than the workspace: one a chunk, each at offset 0
        const MeaProbsLayout y = mea_probs_layout(6, lens, 1);
        CHECK(y.plan.chunks.size() == 4 && y.plan.max_cost == t20);
        for (int s : y.order) CHECK(y.qs[s].p_off == 0 && y.qs[s].wt_off == (unsigned long long)lens[s] * lens[s]);
    }
    {   // nothing to run
        const int none[2] = {0, -3};
        const MeaProbsLayout y = mea_probs_layout(2, none, 100);
        CHECK(y.order.empty() && y.plan.chunks.empty() && y.n_aux == 0 && y.status[1] == RAFFT_ERR_EMPTY && y.len[1] == 0);
        CHECK(mea_probs_layout(0, none, 100).qs.empty());
    }
}

static void check_pf_layout()
{
    const char *seqs[3] = {"GGGAAACCC", "GGX", "ACGUACGUACGU"};
    const int lens[3] = {9, 3, 12};
    const SeqPack pk = pack_sequences(3, seqs, lens, RAFFT_MFE_MAX_LEN);
    const PfLayout p = pf_layout(pk, 6, nullptr, 1 << 20);
    const MeaLayout y = mea_layout(p.qs);
    CHECK(y.qs.size() == 3 && y.qs[1].L == 0 && y.n_stack == 17 + 20);
    CHECK(y.qs[0].wt_off == 0 && y.qs[0].e_off == 81 && y.qs[0].et_off == 162 && y.qs[0].p_off == 243);
    CHECK(y.qs[2].wt_off == 486 && y.qs[2].e_off == 486 + 144 && y.qs[2].et_off == 486 + 288 && y.qs[2].p_off == 486 + 432);
    CHECK(y.qs[0].aux_off == p.qs[0].aux_off && y.qs[2].aux_off == 40 && y.qs[2].stack_off == 17 && y.qs[2].pt_off == 9 && y.qs[2].db_off == 10);
    // the three tables of mea lie within tables 0..2 and P is table 3: nothing reaches tables 4, 5 or the next sequence
    CHECK(y.qs[0].p_off + 81 <= p.qs[2].tab_off && y.qs[0].et_off + 81 == y.qs[0].p_off);
}

static void check_entries()
{
    const int L = 6;
    std::vector<double> P((size_t)L * L, 0.0);
    int i = -1, j = -1;
    const char *why = nullptr;
    CHECK(!mea_probs_bad_entry(P.data(), L, i, j, why));
    P[0 * L + 4] = 1.0; P[1 * L + 5] = 0.125;
    P[3 * L + 0] = 7.0; P[2 * L + 2] = std::numeric_limits<double>::quiet_NaN();       // at or below the diagonal: not read
    CHECK(!mea_probs_bad_entry(P.data(), L, i, j, why));
    P[1 * L + 5] = 1.5;
    CHECK(mea_probs_bad_entry(P.data(), L, i, j, why) && i == 1 && j == 5 && std::string(why).find("outside") != std::string::npos);
    P[1 * L + 5] = -0.25;
    CHECK(mea_probs_bad_entry(P.data(), L, i, j, why) && i == 1 && j == 5);
    P[1 * L + 5] = std::numeric_limits<double>::infinity();
    CHECK(mea_probs_bad_entry(P.data(), L, i, j, why) && i == 1 && j == 5 && std::string(why).find("finite") != std::string::npos);
    P[1 * L + 5] = std::numeric_limits<double>::quiet_NaN();
    CHECK(mea_probs_bad_entry(P.data(), L, i, j, why) && i == 1 && j == 5 && std::string(why).find("finite") != std::string::npos);
    P[1 * L + 5] = 0.0; P[2 * L + 5] = 0.5;
    CHECK(mea_probs_bad_entry(P.data(), L, i, j, why) && i == 2 && j == 5 && std::string(why).find("j - i") != std::string::npos);
    P[0 * L + 1] = 0.25;                                                                // the first in row-major order is named
    CHECK(mea_probs_bad_entry(P.data(), L, i, j, why) && i == 0 && j == 1);
}

int main()
{
    check_sizes();
    check_probs_layout();
    check_pf_layout();
    check_entries();
    printf("%d checks, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
