// Host-side check of the kinfold part of rafft_amd/csrc/rafft_hostpure.h: the weight table (kinfold_weights) against entries the
// test passes in and against its own invariants, the checks of a call's arguments (kinfold_check_call, kinfold_check_watch), and
// the layout of a call (kinfold_layout, the kinfold_* sizes of rafft_batch_layout.h) at the edges of the workspace budget against
// values derived by hand.  Plain C++, no HIP, no GPU.
// usage: kinfold_check [TEMP KT D W]...   entry D of the table at (TEMP, KT) is W, give or take 1.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static void check_weights()
{
    std::vector<uint64_t> w(RAFFT_KINFOLD_NW);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(kinfold_weights(37.0, 0.0, w.data()));
    CHECK(w[0] == (1ull << 32) && w[0] == KINFOLD_W0 && w[1] < w[0] && w[1] > (1ull << 31));
    for (int d = 1; d < RAFFT_KINFOLD_NW; d++) CHECK(w[d] <= w[d - 1]);
    int zero = 0;
    while (zero < RAFFT_KINFOLD_NW && w[zero]) zero++;
    // the first zero entry: 2^32 exp(-d / (100 kT)) < 1/2, d > 100 kT * 33 ln 2
    const double kT = 1.98717e-3 * 310.15;
    CHECK(kinfold_kT(37.0, 0.0) == kT && kinfold_kT(37.0, 0.5) == 0.5);
    CHECK(zero == (int)std::floor(100.0 * kT * 33.0 * std::log(2.0)) + 1);
    for (int d = zero; d < RAFFT_KINFOLD_NW; d++) CHECK(w[d] == 0);
    // a kt of its own; a kT so large that nothing reaches zero, so small that everything uphill does
    CHECK(kinfold_weights(37.0, 50.0, w.data()) && w[RAFFT_KINFOLD_NW - 1] > 0 && w[1] < w[0]);
    CHECK(kinfold_weights(37.0, 1e-4, w.data()) && w[0] == KINFOLD_W0 && w[1] == 0);
    CHECK(!kinfold_weights(37.0, -1.0, w.data()) && !kinfold_weights(37.0, inf, w.data()) && !kinfold_weights(37.0, nan, w.data()));
    CHECK(!kinfold_weights(-273.15, 0.0, w.data()) && !kinfold_weights(-300.0, 0.0, w.data()));
}

static void check_arguments()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double grid[3] = {0.0, 1.5, 10.0}, down[3] = {0.0, 2.0, 1.0}, neg[2] = {-1.0, 1.0}, bad[2] = {1.0, nan}, same[3] = {1.0, 1.0, 1.0};
    CHECK(!kinfold_check_call(1, 0.0, 10.0, 0, 3, grid, 0));
    CHECK(!kinfold_check_call(1, 0.0, 10.0, 0, 0, nullptr, 0) && !kinfold_check_call(7, 0.6, 0.0, 5, 0, nullptr, 1));
    CHECK(!kinfold_check_call(1, 0.0, 1.0, 0, 3, same, 0));            // (equal times ascend)
    CHECK(kinfold_check_call(0, 0.0, 10.0, 0, 3, grid, 0) && kinfold_check_call(-1, 0.0, 10.0, 0, 3, grid, 0));
    CHECK(kinfold_check_call(1, -0.1, 10.0, 0, 3, grid, 0) && kinfold_check_call(1, nan, 10.0, 0, 3, grid, 0) && kinfold_check_call(1, inf, 10.0, 0, 3, grid, 0));
    CHECK(kinfold_check_call(1, 0.0, -1.0, 0, 0, nullptr, 0) && kinfold_check_call(1, 0.0, inf, 0, 0, nullptr, 0) && kinfold_check_call(1, 0.0, nan, 0, 0, nullptr, 0));
    CHECK(kinfold_check_call(1, 0.0, 10.0, -1, 3, grid, 0) && kinfold_check_call(1, 0.0, 10.0, 0, -1, grid, 0) && kinfold_check_call(1, 0.0, 10.0, 0, 3, grid, -1));
    CHECK(kinfold_check_call(1, 0.0, 10.0, 0, 3, nullptr, 0));
    CHECK(kinfold_check_call(1, 0.0, 9.0, 0, 3, grid, 0));             // a time above t_max
    CHECK(kinfold_check_call(1, 0.0, 10.0, 0, 3, down, 0) && kinfold_check_call(1, 0.0, 10.0, 0, 2, neg, 0) && kinfold_check_call(1, 0.0, 10.0, 0, 2, bad, 0));
    CHECK(!kinfold_check_watch(0, 0) && !kinfold_check_watch(64, 64) && !kinfold_check_watch(64, 0) && !kinfold_check_watch(3, 2));
    CHECK(kinfold_check_watch(65, 0) && kinfold_check_watch(3, 4) && kinfold_check_watch(-1, 0) && kinfold_check_watch(2, -1));
}

static void check_sizes()
{
    CHECK(kinfold_io_bytes(1) == 16 && kinfold_io_bytes(9) == 32 && kinfold_io_bytes(4096) == 8192);
    for (int L = 1; L <= 4096; L++) CHECK(kinfold_io_bytes(L) >= (unsigned long long)L + 1 && kinfold_pt_bytes(L) >= 2 * L && kinfold_pt_bytes(L) % 16 == 0);
    CHECK(kinfold_bound(0) == RAFFT_KINFOLD_DEFAULT_STEPS && kinfold_bound(3) == 3 && RAFFT_KINFOLD_DEFAULT_STEPS == 1 << 20);
    CHECK(kinfold_log_bytes(3) == 48 && kinfold_log_bytes(1 << 20) == 16ull << 20);
    CHECK(kinfold_lds_bytes(1) == 24 && kinfold_lds_bytes(4096) == 40 * 1024 && kinfold_lds_bytes(RAFFT_KINFOLD_MAX_LEN) <= 64 * 1024);
    CHECK(RAFFT_KINFOLD_MAX_LEN == RAFFT_DESCEND_MAX_LEN && RAFFT_KINFOLD_MAX_LEN <= 32767 && RAFFT_KINFOLD_MAX_WATCH == 64 && RAFFT_KINFOLD_NW == 4096);
    // the sum of the weights of every neighbour of the longest chain stays in 64 bits: below L^2 / 2 moves of 2^32
    CHECK((unsigned long long)RAFFT_KINFOLD_MAX_LEN * RAFFT_KINFOLD_MAX_LEN / 2 < (1ull << 31));
    CHECK(sizeof(KfTraj) == 64 && sizeof(KfRec) == 32 && sizeof(KfSample) == 8 && sizeof(rafft_kinfold_seq) == 16 && sizeof(rafft_kinfold_traj) == 32);
    CHECK(KF_TIME == RAFFT_KINFOLD_TIME && KF_STOP == RAFFT_KINFOLD_STOP && KF_ABSORBED == RAFFT_KINFOLD_ABSORBED && KF_MORE == RAFFT_KINFOLD_MORE);
}

static void check_layout()
{
    // four trajectories: 10, 10, 20 and 9 positions, the second and the fourth with a log; bound 3, two sample times
    const int L[4] = {10, 10, 20, 9}, nw[4] = {0, 0, 5, 64}, ns[4] = {0, 0, 2, 64};
    const unsigned k[4] = {0, 1, 0, 7};
    const unsigned long long code_off[4] = {0, 0, 10, 30}, wt_off[4] = {0, 0, 0, 100}, seed[4] = {5, 5, 6, ~0ull};
    const unsigned char lg[4] = {0, 1, 0, 1};
    const size_t b0 = 32 + 16, b1 = 32 + 16 + 48, b2 = 48 + 16, b3 = 32 + 16 + 48;
    {   // everything fits: one chunk
        const KfLayout y = kinfold_layout(4, L, k, code_off, wt_off, seed, nw, ns, lg, 3, 2, 1 << 20);
        CHECK(y.plan.chunks.size() == 1 && y.plan.chunks[0].a == 0 && y.plan.chunks[0].b == 4 && y.plan.max_cost == b0 + b1 + b2 + b3);
        CHECK(y.bytes[0] == b0 && y.bytes[1] == b1 && y.bytes[2] == b2 && y.bytes[3] == b3);
        CHECK(y.ws[0].io_off == 0 && y.ws[1].io_off == 32 && y.ws[2].io_off == 64 && y.ws[3].io_off == 112 && y.chunk_io[0] == 144);
        CHECK(y.ws[0].log_off == KINFOLD_NO_LOG && y.ws[1].log_off == 0 && y.ws[2].log_off == KINFOLD_NO_LOG && y.ws[3].log_off == 48 && y.chunk_log[0] == 96);
        CHECK(y.ws[2].code_off == 10 && y.ws[2].L == 20 && y.ws[2].bound == 3 && y.ws[2].n_watch == 5 && y.ws[2].n_stop == 2 && y.ws[2].seed == 6);
        CHECK(y.ws[3].k == 7 && y.ws[3].wt_off == 100 && y.ws[3].seed == ~0ull && y.ws[3].n_watch == 64 && y.ws[1].k == 1);
        CHECK(y.chunk_lmax[0] == 20 && y.max_io == 144 && y.max_log == 96 && y.max_traj == 4);
    }
    {   // exactly fitting: the first two, then the other two in b2 + b3 bytes
        const KfLayout y = kinfold_layout(4, L, k, code_off, wt_off, seed, nw, ns, lg, 3, 2, b2 + b3);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2 && y.plan.chunks[1].a == 2 && y.plan.chunks[1].b == 4);
        CHECK(y.ws[2].io_off == 0 && y.ws[3].io_off == 48 && y.ws[3].log_off == 0 && y.ws[1].log_off == 0 && y.max_traj == 2);
        CHECK(y.chunk_io[0] == 64 && y.chunk_io[1] == 80 && y.chunk_log[0] == 48 && y.chunk_log[1] == 48 && y.chunk_lmax[0] == 10 && y.chunk_lmax[1] == 20);
        const KfLayout z = kinfold_layout(4, L, k, code_off, wt_off, seed, nw, ns, lg, 3, 2, b2 + b3 - 1);     // one byte less: the last alone
        CHECK(z.plan.chunks.size() == 3 && z.plan.chunks[0].b == 2 && z.plan.chunks[1].b == 3 && z.ws[1].io_off == 32 && z.ws[2].io_off == 0 && z.ws[3].io_off == 0);
    }
    {   // every trajectory larger than the workspace: one per chunk, each at offset 0
        const KfLayout y = kinfold_layout(4, L, k, code_off, wt_off, seed, nw, ns, lg, 3, 2, 1);
        CHECK(y.plan.chunks.size() == 4 && y.max_io == 48 && y.max_log == 48 && y.max_traj == 1);
        for (int t = 0; t < 4; t++) CHECK(y.ws[t].io_off == 0 && (y.ws[t].log_off == 0 || y.ws[t].log_off == KINFOLD_NO_LOG));
    }
    {   // no log, no sample times: rows only
        const unsigned char none[4] = {0, 0, 0, 0};
        const KfLayout y = kinfold_layout(4, L, k, code_off, wt_off, seed, nw, ns, none, 0 + RAFFT_KINFOLD_DEFAULT_STEPS, 0, 1 << 20);
        CHECK(y.max_log == 0 && y.chunk_log[0] == 0 && y.plan.max_cost == 32 + 32 + 48 + 32 && y.ws[0].bound == 1 << 20);
    }
    {   // nothing to run
        const KfLayout y = kinfold_layout(0, L, k, code_off, wt_off, seed, nw, ns, lg, 3, 2, 100);
        CHECK(y.plan.chunks.empty() && y.max_io == 0 && y.ws.empty() && y.max_traj == 0);
    }
}

int main(int argc, char **argv)
{
    check_weights();
    check_arguments();
    check_sizes();
    check_layout();
    if ((argc - 1) % 4) { fprintf(stderr, "usage: kinfold_check [TEMP KT D W]...\n"); return 2; }
    std::vector<uint64_t> w(RAFFT_KINFOLD_NW);
    for (int a = 1; a + 3 < argc; a += 4) {
        const int d = atoi(argv[a + 2]);
        const unsigned long long want = strtoull(argv[a + 3], nullptr, 10);
        if (!kinfold_weights(atof(argv[a]), atof(argv[a + 1]), w.data()) || d < 0 || d >= RAFFT_KINFOLD_NW || (w[d] > want ? w[d] - want : want - w[d]) > 1) {
            fails++;
            fprintf(stderr, "FAIL %s %s %s: expected %s\n", argv[a], argv[a + 1], argv[a + 2], argv[a + 3]);
        }
    }
    printf("%d cases, %d failures\n", (argc - 1) / 4, fails);
    return fails ? 1 : 0;
}
