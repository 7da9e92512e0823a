// Host-side check of the cofold part of rafft_amd/csrc/rafft_hostpure.h and rafft_batch_layout.h: the cuts of a
// rafft_cofold_batch call (cut_pack) - null cuts, cut 0, the two ends of the valid range, every bad cut, sequences with an error of
// their own - the record, the LDS size of the dimer kernel and the room G has in the HBM class, against values derived by hand.
// Plain C++, no HIP, no GPU.  usage: cofold_check.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0, cases = 0;
#define CHECK(c) do { cases++; if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static void check_sizes()
{
    CHECK(sizeof(rafft_cofold_seq) == 24 && sizeof(rafft_mfe_seq) == 16);
    // G behind the bases: 129520 + 592 bytes at 146 nt, a size the kernel asks for itself, within 160 KiB
    CHECK(mfe_lds_bytes(146) == 129520 && cofold_lds_bytes(146) == 129520 + 592 && cofold_lds_bytes(146) <= COFOLD_LDS_BYTES && COFOLD_LDS_BYTES == 160 << 10);
    CHECK(cofold_lds_bytes(1) == mfe_lds_bytes(1) + 16 && cofold_lds_bytes(3) == mfe_lds_bytes(3) + 16 && cofold_lds_bytes(4) == mfe_lds_bytes(4) + 32);
    for (int L = 1; L <= RAFFT_MFE_LDS_LEN; L++) CHECK(cofold_lds_bytes(L) % 4 == 0 && cofold_lds_bytes(L) - mfe_lds_bytes(L) >= 4 * (L + 1));      // G is L + 1 int32
}

static void check_cuts()
{
    const char *seqs[7] = {"GGGAAACCC", "", "GGGAAACCC", "GGX", "GC", "G", "GGGAAACCC"};
    const int lens[7] = {9, 0, 9, 3, 2, 1, 9};
    const SeqPack pk = pack_sequences(7, seqs, lens, RAFFT_MFE_MAX_LEN);
    {   // no cuts at all: every sequence a single strand
        const CutPack p = cut_pack(7, pk.L.data(), nullptr);
        for (int s = 0; s < 7; s++) CHECK(p.status[s] == 0 && p.cut[s] == 0);
        CHECK(p.first_seq < 0 && p.first_err.empty());
    }
    {   // 0, the two ends of the range, and the cuts of sequences with an error are not looked at
        const int cuts[7] = {1, 77, 8, -5, 1, 0, 0};
        const CutPack p = cut_pack(7, pk.L.data(), cuts);
        for (int s = 0; s < 7; s++) CHECK(p.status[s] == 0);
        CHECK(p.cut[0] == 1 && p.cut[1] == 0 && p.cut[2] == 8 && p.cut[3] == 0 && p.cut[4] == 1 && p.cut[5] == 0 && p.cut[6] == 0 && p.first_seq < 0);
    }
    {   // outside 0 .. L - 1: that sequence's error, its neighbours keep their cuts, the first one is named
        const int cuts[7] = {4, 0, 9, 0, -1, 1, 2147483647};
        const CutPack p = cut_pack(7, pk.L.data(), cuts);
        CHECK(p.status[0] == 0 && p.status[1] == 0 && p.status[2] == RAFFT_ERR_STRUCT && p.status[3] == 0 && p.status[4] == RAFFT_ERR_STRUCT);
        CHECK(p.status[5] == RAFFT_ERR_STRUCT && p.status[6] == RAFFT_ERR_STRUCT);
        CHECK(p.cut[0] == 4 && p.cut[2] == 0 && p.cut[4] == 0 && p.cut[5] == 0 && p.cut[6] == 0);
        CHECK(p.first_seq == 2 && p.first_err.find("sequence 2") == 0 && p.first_err.find("cut") != std::string::npos);
    }
    {   // the layout a dimer shares with a single strand: G of the HBM class lies at stack_off, where the sequence owns L + 8 >= L + 1 ints
        const MfeLayout y = mfe_layout(pk, 4, (size_t)1 << 20);
        CHECK(y.lds_order.size() == 2 && y.hbm_order.size() == 3 && y.n_stack == 3 * 17 + 10 + 9);
        for (size_t a = 0; a < y.order.size(); a++)
            for (size_t b = 0; b < y.order.size(); b++) {
                const MfeSeq &qa = y.qs[y.order[a]], &qb = y.qs[y.order[b]];
                if (a != b) CHECK(qa.stack_off + (unsigned long long)qa.L + 1 <= qb.stack_off || qb.stack_off + (unsigned long long)qb.L + 1 <= qa.stack_off);
                CHECK(qa.stack_off + (unsigned long long)qa.L + 1 <= y.n_stack);
            }
    }
}

int main()
{
    check_sizes();
    check_cuts();
    printf("%d checks, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
