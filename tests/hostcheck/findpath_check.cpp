// Host-side check of the findpath part of rafft_amd/csrc/rafft_hostpure.h: the moves and conflict masks of a problem
// (findpath_moves) against descriptions the test passes in, and the layout of a call (findpath_layout, the fp_* sizes of
// rafft_batch_layout.h) at the edges of the workspace budget against values derived by hand.  Plain C++, no HIP, no GPU.
// usage: findpath_check [SEQ A B STATUS DESC]...   DESC = "n_rem;i-j,i-j,...;mask,mask,..." (all moves in order; per addition the
// conflict mask as hexadecimal, words joined by ':'), ignored when STATUS != 0.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static std::string describe(const FpMoves &m)
{
    std::string s = std::to_string(m.n_rem) + ";";
    for (int k = 0; k < m.d; k++) s += (k ? "," : "") + std::to_string(m.moves[k] & 0xffffu) + "-" + std::to_string(m.moves[k] >> 16);
    s += ";";
    const int mw = fp_mask_words(m.d);
    char buf[32];
    for (int k = m.n_rem; k < m.d; k++) {
        if (k > m.n_rem) s += ",";
        for (int w = 0; w < mw; w++) {
            snprintf(buf, sizeof buf, "%s%llx", w ? ":" : "", (unsigned long long)m.conf[(size_t)(k - m.n_rem) * mw + w]);
            s += buf;
        }
    }
    return s;
}

static void check_case(const char *seq, const char *a, const char *b, int want_status, const char *want)
{
    const int L = (int)strlen(seq);
    std::vector<uint8_t> codes((size_t)L + 16, 0);
    for (int x = 0; x < L; x++) codes[x] = (uint8_t)(kBaseCode[(unsigned char)seq[x]] & 7);
    FpMoves m;
    const int st = findpath_moves(codes.data(), L, a, b, m);
    if (st != want_status) { fails++; fprintf(stderr, "FAIL %s %s %s: status %d, expected %d\n", seq, a, b, st, want_status); return; }
    if (st) return;
    CHECK((int)m.pt_a.size() == L && (int)m.pt_b.size() == L && (int)m.moves.size() == m.d);
    CHECK(m.conf.size() == (size_t)(m.d - m.n_rem) * fp_mask_words(m.d));
    const std::string got = describe(m);
    if (got != want) { fails++; fprintf(stderr, "FAIL %s %s %s: %s, expected %s\n", seq, a, b, got.c_str(), want); }
}

static void check_sizes()
{
    CHECK(fp_mask_words(0) == 1 && fp_mask_words(1) == 1 && fp_mask_words(64) == 1 && fp_mask_words(65) == 2 && fp_mask_words(4096) == 64);
    // L = 10, d = 3 moves of which 1 removal: two tables of 32 bytes, 16 bytes of moves, two masks of one word
    CHECK(fp_in_pt_bytes(10) == 32 && fp_in_moves_off(10) == 64 && fp_in_conf_off(10, 3) == 80 && fp_in_bytes(10, 3, 1) == 96);
    CHECK(fp_out_dcal_off(3) == 32 && fp_out_bytes(3) == 48);
    CHECK(fp_out_dcal_off(0) == 0 && fp_out_bytes(0) == 16 && fp_in_bytes(10, 0, 0) == 64);
    // W = 4: two beams of 4 masks (64 bytes), two of 4 (energy, saddle) (64), 12 keys (96), 12 records (96)
    CHECK(fp_ws_mask_bytes(3, 4) == 32 && fp_ws_es_off(3, 4) == 64 && fp_ws_keys_off(3, 4) == 128 && fp_ws_back_off(3, 4) == 224 && fp_ws_bytes(3, 4) == 320);
    CHECK(fp_ws_bytes(0, 4) == 128);
    // the largest problem the caps allow: 1024 x 1024 candidates
    CHECK(fp_ws_bytes(1024, 1024) == 2ull * 1024 * 16 * 8 + 2ull * 1024 * 8 + 2ull * 8 * (1ull << 20));
    CHECK((1 << FINDPATH_INDEX_BITS) == RAFFT_FINDPATH_MAX_CANDIDATES && 2 * FINDPATH_KEY_BITS + FINDPATH_INDEX_BITS == 64);
    CHECK(RAFFT_FINDPATH_MAX_WIDTH <= 0xffff && RAFFT_FINDPATH_MAX_LEN <= 0xffff);     // (parent rank | move << 16 of a level's records)
}

static void check_layout()
{
    // five problems of the call; 1 and 3 have an error and take no room
    const int L[5] = {10, 0, 10, 0, 20}, d[5] = {3, 0, 3, 0, 0}, n_rem[5] = {1, 0, 1, 0, 0}, W[5] = {4, 0, 4, 0, 8};
    const unsigned long long code_off[5] = {0, 10, 10, 20, 20};
    const std::vector<int> run{0, 2, 4};
    const size_t ws03 = 320, ws4 = (size_t)fp_ws_bytes(0, 8), io03 = 96 + 48, io4 = (size_t)(fp_in_bytes(20, 0, 0) + fp_out_bytes(0));
    CHECK(ws4 == 2 * 64 + 128 && io4 == 96 + 16);
    {   // everything fits: one chunk
        const FpLayout y = findpath_layout(5, run, L, d, n_rem, W, code_off, 1 << 20);
        CHECK(y.plan.chunks.size() == 1 && y.plan.chunks[0].a == 0 && y.plan.chunks[0].b == 3 && y.plan.max_cost == 2 * ws03 + ws4);
        CHECK(y.ps[0].in_off == 0 && y.ps[2].in_off == 96 && y.ps[4].in_off == 192 && y.chunk_in[0] == 192 + 96);
        CHECK(y.ps[0].out_off == 0 && y.ps[2].out_off == 48 && y.ps[4].out_off == 96 && y.chunk_out[0] == 112);
        CHECK(y.ps[0].ws_off == 0 && y.ps[2].ws_off == 320 && y.ps[4].ws_off == 640 && y.chunk_dmax[0] == 3);
        CHECK(y.ps[2].code_off == 10 && y.ps[2].L == 10 && y.ps[2].d == 3 && y.ps[2].n_rem == 1 && y.ps[2].W == 4);
        CHECK(y.ps[1].L == 0 && y.ps[1].W == 0 && y.ps[3].ws_off == 0);
        CHECK(y.max_in == 288 && y.max_out == 112 && y.ws_bytes.size() == 3 && y.ws_bytes[2] == ws4 && y.io_bytes[0] == io03 && y.io_bytes[2] == io4);
    }
    {   // exactly fitting: two problems in 640 bytes, the third opens a chunk
        const FpLayout y = findpath_layout(5, run, L, d, n_rem, W, code_off, 640);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2 && y.plan.chunks[1].a == 2 && y.plan.chunks[1].b == 3);
        CHECK(y.ps[2].ws_off == 320 && y.ps[4].ws_off == 0 && y.ps[4].in_off == 0 && y.ps[4].out_off == 0);
        CHECK(y.chunk_in[0] == 192 && y.chunk_in[1] == 96 && y.chunk_out[0] == 96 && y.chunk_out[1] == 16 && y.chunk_dmax[0] == 3 && y.chunk_dmax[1] == 0);
        CHECK(y.plan.max_cost == 640 && y.max_in == 192 && y.max_out == 96);
        const FpLayout z = findpath_layout(5, run, L, d, n_rem, W, code_off, 639);      // one byte less: the first alone, then 320 + 256
        CHECK(z.plan.chunks.size() == 2 && z.plan.chunks[0].b == 1 && z.ps[2].ws_off == 0 && z.ps[2].in_off == 0 && z.ps[4].ws_off == 320 && z.ps[4].in_off == 96);
    }
    {   // every problem larger than the workspace: one problem per chunk, each at offset 0
        const FpLayout y = findpath_layout(5, run, L, d, n_rem, W, code_off, 1);
        CHECK(y.plan.chunks.size() == 3 && y.plan.max_cost == 320 && y.max_in == 96 && y.max_out == 48);
        for (int p : run) CHECK(y.ps[p].ws_off == 0 && y.ps[p].in_off == 0 && y.ps[p].out_off == 0);
    }
    {   // the second cost cuts as well: inputs and outputs of two problems are 288 bytes
        const FpLayout y = findpath_layout(5, run, L, d, n_rem, W, code_off, 700);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2);
        const int W2[5] = {1, 0, 1, 0, 1};          // work areas of 80, 80 and 32 bytes: now the inputs and outputs decide
        CHECK(fp_ws_bytes(3, 1) == 80);
        const FpLayout z = findpath_layout(5, run, L, d, n_rem, W2, code_off, 2 * io03);
        CHECK(z.plan.chunks.size() == 2 && z.plan.chunks[0].b == 2 && z.plan.max_cost2 == 2 * io03);
        const FpLayout u = findpath_layout(5, run, L, d, n_rem, W2, code_off, 2 * io03 - 1);
        CHECK(u.plan.chunks.size() == 2 && u.plan.chunks[0].b == 1 && u.plan.max_cost2 == io03 + io4);
    }
    {   // nothing to run
        const FpLayout y = findpath_layout(2, {}, L, d, n_rem, W, code_off, 100);
        CHECK(y.plan.chunks.empty() && y.max_in == 0 && y.ps.size() == 2);
    }
}

int main(int argc, char **argv)
{
    check_sizes();
    check_layout();
    if ((argc - 1) % 5) { fprintf(stderr, "usage: findpath_check [SEQ A B STATUS DESC]...\n"); return 2; }
    for (int k = 1; k + 4 < argc; k += 5) check_case(argv[k], argv[k + 1], argv[k + 2], atoi(argv[k + 3]), argv[k + 4]);
    printf("%d cases, %d failures\n", (argc - 1) / 5, fails);
    return fails ? 1 : 0;
}
