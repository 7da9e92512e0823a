// Host-side check of the constraint part of rafft_amd/csrc/rafft_hostpure.h: the packs of a rafft_mfe_constrained_batch call
// (constraint_pack) - offsets, codes, prefixes, every malformed string, null arrays and null entries, the soft bound - and the
// sizes of rafft_batch_layout.h, against values derived by hand.  Plain C++, no HIP, no GPU.  usage: mfe_con_check.  Test
// infrastructure.
#include <cstdio>
#include <cstdlib>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0, cases = 0;
#define CHECK(c) do { cases++; if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static void check_sizes()
{
    CHECK(sizeof(rafft_mfe_con_seq) == 24 && sizeof(rafft_mfe_seq) == 16);
    CHECK(RAFFT_ERR_INFEASIBLE == 10 && RAFFT_MFE_SOFT_MAX == 20000);
    CHECK(mfe_con_pack_ints(1) == 6 && mfe_con_pack_ints(146) == 586 && mfe_con_pack_ints(4096) == 16386);
    // the pack behind the bases: 129520 + 2344 bytes at 146 nt - more than the 128 KiB of the unconstrained kernel, within 160 KiB
    CHECK(mfe_lds_bytes(146) == 129520 && mfe_con_lds_bytes(146) == 131872 && mfe_con_lds_bytes(146) > MFE_LDS_BYTES && mfe_con_lds_bytes(146) <= MFE_CON_LDS_BYTES);
    CHECK(mfe_con_lds_bytes(1) == mfe_lds_bytes(1) + 32 && MFE_CON_LDS_BYTES == 160 << 10);
    for (int L = 1; L <= RAFFT_MFE_LDS_LEN; L++) CHECK(mfe_con_lds_bytes(L) % 4 == 0 && mfe_lds_bytes(L) % 4 == 0);    // the pack is int32
    // the soft terms of the longest sequence stay below the guard: a position counts once in u or at most twice in b
    CHECK(4096ll * 2 * RAFFT_MFE_SOFT_MAX < 500000000ll);
    CHECK(MFE_CON_ANY < 0 && MFE_CON_UNPAIRED < 0 && MFE_CON_PAIRED < 0 && MFE_CON_DOWN < 0 && MFE_CON_UP < 0);     // no position
}

// a pack of the sequences `seqs` (all foldable) with the given inputs
static ConstraintPack pack_of(int n, const char *const *seqs, const int *lens, const char *const *con, const int32_t *const *u, const int32_t *const *b)
{
    const SeqPack pk = pack_sequences(n, seqs, lens, RAFFT_MFE_MAX_LEN);
    return constraint_pack(n, pk.L.data(), pk.codes.data(), pk.code_off.data(), con, u, b);
}

static void check_pack()
{
    //                     0123456789
    const char *seqs[6] = {"GGGAAACCCA", "", "GGGAAACCC", "GGGAAACCCA", "GGX", "GCAAAGC"};
    const int lens[6] = {10, 0, 9, 10, 3, 7};
    const char *con[6] = {"(x|...<>).", "....", nullptr, "..........", "...", nullptr};
    const int32_t u0[10] = {1, 2, 3, 4, 5, 6, 7, 8, 9, -20000}, b5[7] = {-5, 0, 0, 0, 0, 0, 20000};
    const int32_t *u[6] = {u0, nullptr, nullptr, nullptr, nullptr, nullptr}, *b[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, b5};
    const ConstraintPack p = pack_of(6, seqs, lens, con, u, b);
    CHECK(p.param_seq < 0 && p.first_seq < 0 && p.first_err.empty());
    for (int s = 0; s < 6; s++) CHECK(p.status[s] == 0);
    // sequences with an error (1, 4) and without any constraint (2) take no space and point at nothing
    CHECK(p.off[1] == MFE_CON_NONE && p.off[2] == MFE_CON_NONE && p.off[4] == MFE_CON_NONE);
    CHECK(p.off[0] == 0 && p.off[3] == 42 && p.off[5] == 84 && p.data.size() == 84 + 30 + 4);
    const int32_t *d = p.data.data();
    const int32_t code0[10] = {8, MFE_CON_UNPAIRED, MFE_CON_PAIRED, MFE_CON_ANY, MFE_CON_ANY, MFE_CON_ANY, MFE_CON_DOWN, MFE_CON_UP, 0, MFE_CON_ANY};
    const int32_t must0[11] = {0, 1, 1, 2, 2, 2, 2, 3, 4, 5, 5}, usum0[11] = {0, 1, 3, 6, 10, 15, 21, 28, 36, 45, -19955};
    for (int k = 0; k < 10; k++) CHECK(d[k] == code0[k] && d[32 + k] == 0);
    for (int k = 0; k <= 10; k++) CHECK(d[10 + k] == must0[k] && d[21 + k] == usum0[k]);
    // an all-'.' string is a pack of its own: every code ANY, every prefix 0
    for (int k = 0; k < 10; k++) CHECK(d[42 + k] == MFE_CON_ANY);
    for (int k = 10; k < 42; k++) CHECK(d[42 + k] == 0);
    // soft_stack alone: codes ANY, b behind the two prefixes
    for (int k = 0; k < 7; k++) CHECK(d[84 + k] == MFE_CON_ANY && d[84 + 7 + 8 + 8 + k] == b5[k]);
    for (int k = 0; k < 4; k++) CHECK(d[84 + 30 + k] == 0);
    // null arrays as a whole
    const ConstraintPack none = pack_of(6, seqs, lens, nullptr, nullptr, nullptr);
    for (int s = 0; s < 6; s++) CHECK(none.off[s] == MFE_CON_NONE && none.status[s] == 0);
    CHECK(none.data.size() == 4 && none.first_seq < 0 && none.param_seq < 0);
    const ConstraintPack only_u = pack_of(6, seqs, lens, nullptr, u, nullptr);
    CHECK(only_u.off[0] == 0 && only_u.off[3] == MFE_CON_NONE && only_u.data.size() == 42 + 4 && only_u.data[21 + 10] == -19955);
}

static void check_malformed()
{
    //                  012345678
    const char *seq = "GGGAAACCC";
    struct { const char *con; bool good; } cases_[] = {
        {"(((...)))", true}, {"(.......)", true}, {"..(...)..", true}, {"x|<>.....", true},
        {"((.....))", true},
        {"(((...))", false},            // a string of the wrong length
        {"(((...))).", false},
        {"", false},
        {"(((...)).", false},           // unbalanced: an open bracket left
        {".((...)))", false},           // unbalanced: a closing bracket without a partner
        {")(.......", false},
        {"..(..)...", false},           // G-A: not canonical... and encloses 2
        {"...(...).", false},           // A-C: not canonical
        {"(.)......", false},           // G-G: not canonical
        {".(..)....", false},           // encloses fewer than 3 (G-A as well)
        {"[[[...]]]", false},           // other characters
        {"(((.X.)))", false},
        {"(((. .)))", false},
        {"(((...)))\n", false},
    };
    for (const auto &c : cases_) {
        const char *seqs[1] = {seq}, *con[1] = {c.con};
        const int lens[1] = {9};
        const ConstraintPack p = pack_of(1, seqs, lens, con, nullptr, nullptr);
        CHECK((p.status[0] == 0) == c.good);
        CHECK(c.good ? p.off[0] == 0 && p.first_seq < 0 : p.status[0] == RAFFT_ERR_STRUCT && p.off[0] == MFE_CON_NONE && p.first_seq == 0 && p.data.size() == 4);
        CHECK(p.param_seq < 0);
    }
    {   // a canonical pair that encloses exactly 2 / exactly 3: GAAC / GAAAC
        const char *s4[1] = {"GAAC"}, *c4[1] = {"(..)"}, *s5[1] = {"GAAAC"}, *c5[1] = {"(...)"}, *g5[1] = {"GAAAU"};
        const int l4[1] = {4}, l5[1] = {5};
        CHECK(pack_of(1, s4, l4, c4, nullptr, nullptr).status[0] == RAFFT_ERR_STRUCT);
        CHECK(pack_of(1, s5, l5, c5, nullptr, nullptr).status[0] == 0);
        CHECK(pack_of(1, g5, l5, c5, nullptr, nullptr).status[0] == 0);         // GU
    }
    {   // an error is that sequence's: its neighbours keep their packs, back to back; the first error is named
        const char *seqs[4] = {seq, seq, seq, seq}, *con[4] = {"(((...)))", "(((...))", "...xxx...", "((((.))))"};
        const int lens[4] = {9, 9, 9, 9};
        const ConstraintPack p = pack_of(4, seqs, lens, con, nullptr, nullptr);
        CHECK(p.status[0] == 0 && p.status[1] == RAFFT_ERR_STRUCT && p.status[2] == 0 && p.status[3] == RAFFT_ERR_STRUCT);
        CHECK(p.off[0] == 0 && p.off[1] == MFE_CON_NONE && p.off[2] == 38 && p.off[3] == MFE_CON_NONE && p.data.size() == 76 + 4);
        CHECK(p.first_seq == 1 && p.first_err.find("sequence 1") == 0 && p.first_err.find("length") != std::string::npos);
        CHECK(p.data[0] == 8 && p.data[8] == 0 && p.data[38 + 3] == MFE_CON_UNPAIRED && p.data[38 + 9 + 9] == 0);
    }
}

static void check_soft_bound()
{
    const char *seqs[2] = {"GGGAAACCC", "GGGAAACCC"};
    const int lens[2] = {9, 9};
    int32_t a[9] = {0, 20000, -20000, 0, 0, 0, 0, 0, 0}, c[9] = {0};
    const int32_t *u[2] = {a, c}, *b[2] = {c, a};
    CHECK(pack_of(2, seqs, lens, nullptr, u, b).param_seq < 0);
    c[8] = 20001;
    const ConstraintPack hi = pack_of(2, seqs, lens, nullptr, u, b);
    CHECK(hi.param_seq == 0 && hi.first_err.find("RAFFT_MFE_SOFT_MAX") != std::string::npos);      // (b of sequence 0 is c)
    c[8] = 0; a[0] = -20001;
    CHECK(pack_of(2, seqs, lens, nullptr, u, b).param_seq == 0);
    a[0] = 0; c[4] = INT32_MIN;
    CHECK(pack_of(2, seqs, lens, nullptr, u, nullptr).param_seq == 1);
    // the values of a sequence with an error are not looked at
    const char *bad[2] = {"GGGXAACCC", "GGGAAACCC"};
    const int32_t *ub[2] = {c, nullptr};
    CHECK(pack_of(2, bad, lens, nullptr, ub, nullptr).param_seq < 0);
}

int main()
{
    check_sizes();
    check_pack();
    check_malformed();
    check_soft_bound();
    printf("%d checks, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
