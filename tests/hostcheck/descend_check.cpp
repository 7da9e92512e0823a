// Host-side check of the descend part of rafft_amd/csrc/rafft_hostpure.h: the pair table and status of a start row
// (descend_parse_row) against what the test passes in, and the layout of a call (descend_layout, the descend_* sizes of
// rafft_batch_layout.h) at the edges of the workspace budget against values derived by hand, and the row intake the three row
// drivers share (row_ptr, copy_row_back, FirstError).  Plain C++, no HIP, no GPU.
// usage: descend_check [SEQ ROW STATUS PAIRS]...   PAIRS = "i-j,i-j,..." (ascending 5' end), ignored when STATUS != 0; ROW may be
// shorter than SEQ (the library then meets its NUL).  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

static void check_case(const char *seq, const char *row, int want_status, const char *want)
{
    const int L = (int)strlen(seq);
    std::vector<uint8_t> codes((size_t)L + 16, 0);
    for (int x = 0; x < L; x++) codes[x] = (uint8_t)(kBaseCode[(unsigned char)seq[x]] & 7);
    // the row as the library meets it: L bytes of a buffer, nothing readable behind them but what the row itself holds
    std::vector<char> buf(strlen(row) + 1);
    memcpy(buf.data(), row, buf.size());
    std::vector<int16_t> pt;
    const int st = descend_parse_row(codes.data(), L, buf.data(), pt);
    if (st != want_status) { fails++; fprintf(stderr, "FAIL %s %s: status %d, expected %d\n", seq, row, st, want_status); return; }
    if (st) return;
    CHECK((int)pt.size() == L);
    std::string got;
    for (int i = 0; i < L; i++) {
        if (pt[i] > i) { got += (got.empty() ? "" : ",") + std::to_string(i) + "-" + std::to_string(pt[i]); CHECK(pt[pt[i]] == i); }
        else if (pt[i] < 0) CHECK(pt[i] == -1);
    }
    if (got != want) { fails++; fprintf(stderr, "FAIL %s %s: %s, expected %s\n", seq, row, got.c_str(), want); }
}

static void check_sizes()
{
    CHECK(descend_io_bytes(1) == 16 && descend_io_bytes(8) == 16 && descend_io_bytes(9) == 32 && descend_io_bytes(4096) == 8192);
    for (int L = 1; L <= 4096; L++) CHECK(descend_io_bytes(L) >= (unsigned long long)L + 1 && descend_io_bytes(L) >= 2ull * L);       // (the end row and its NUL lie over the table)
    CHECK(descend_bound(10, 0) == 36 && descend_bound(10, 3) == 3 && descend_bound(4096, 0) == 8208 && descend_bound(1, 0) == 18);
    CHECK(descend_moves_bytes(3) == 32 && descend_moves_bytes(36) == 288 && descend_moves_bytes(2) == 16);
    CHECK(descend_lds_bytes(1) == 16 && descend_lds_bytes(4096) == 8192 && descend_lds_bytes(4096) <= 64 * 1024);
    CHECK(RAFFT_DESCEND_MAX_LEN <= 0xffff && RAFFT_DESCEND_MAX_LEN <= 32767);       // (i << 16 | j of a key; int16 pair tables)
    CHECK(sizeof(DsWalk) == 32 && sizeof(DsRec) == 16 && sizeof(rafft_descend_seq) == 16 && sizeof(rafft_descend_row) == 16);
}

static void check_layout()
{
    // four walks: 10, 10, 20 and 9 positions, the second and the fourth with moves (bounds 36 and 3)
    const int L[4] = {10, 10, 20, 9}, bound[4] = {36, 36, 56, 3};
    const unsigned long long code_off[4] = {0, 0, 10, 30};
    const unsigned char mv[4] = {0, 1, 0, 1};
    const size_t b0 = 32, b1 = 32 + 288, b2 = 48, b3 = 32 + 32;
    {   // everything fits: one chunk
        const DsLayout y = descend_layout(4, L, bound, code_off, mv, 1 << 20);
        CHECK(y.plan.chunks.size() == 1 && y.plan.chunks[0].a == 0 && y.plan.chunks[0].b == 4 && y.plan.max_cost == b0 + b1 + b2 + b3);
        CHECK(y.bytes[0] == b0 && y.bytes[1] == b1 && y.bytes[2] == b2 && y.bytes[3] == b3);
        CHECK(y.ws[0].io_off == 0 && y.ws[1].io_off == 32 && y.ws[2].io_off == 64 && y.ws[3].io_off == 112 && y.chunk_io[0] == 144);
        CHECK(y.ws[0].mv_off == DESCEND_NO_MOVES && y.ws[1].mv_off == 0 && y.ws[2].mv_off == DESCEND_NO_MOVES && y.ws[3].mv_off == 288 && y.chunk_mv[0] == 320);
        CHECK(y.ws[2].code_off == 10 && y.ws[2].L == 20 && y.ws[2].bound == 56 && y.ws[3].L == 9 && y.ws[3].bound == 3);
        CHECK(y.chunk_lmax[0] == 20 && y.max_io == 144 && y.max_mv == 320);
    }
    {   // exactly fitting: the first two in b0 + b1 bytes, then the other two
        const DsLayout y = descend_layout(4, L, bound, code_off, mv, b0 + b1);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2 && y.plan.chunks[1].a == 2 && y.plan.chunks[1].b == 4);
        CHECK(y.ws[2].io_off == 0 && y.ws[3].io_off == 48 && y.ws[3].mv_off == 0 && y.ws[1].mv_off == 0);
        CHECK(y.chunk_io[0] == 64 && y.chunk_io[1] == 80 && y.chunk_mv[0] == 288 && y.chunk_mv[1] == 32 && y.chunk_lmax[0] == 10 && y.chunk_lmax[1] == 20);
        CHECK(y.max_io == 80 && y.max_mv == 288);
        const DsLayout z = descend_layout(4, L, bound, code_off, mv, b0 + b1 - 1);      // one byte less: the first alone
        CHECK(z.plan.chunks.size() == 3 && z.plan.chunks[0].b == 1 && z.plan.chunks[1].b == 2 && z.ws[1].io_off == 0 && z.ws[2].io_off == 0 && z.ws[3].io_off == 48);
    }
    {   // every walk larger than the workspace: one walk per chunk, each at offset 0
        const DsLayout y = descend_layout(4, L, bound, code_off, mv, 1);
        CHECK(y.plan.chunks.size() == 4 && y.max_io == 48 && y.max_mv == 288);
        for (int k = 0; k < 4; k++) CHECK(y.ws[k].io_off == 0 && (y.ws[k].mv_off == 0 || y.ws[k].mv_off == DESCEND_NO_MOVES));
    }
    {   // nobody asked for moves: no move bytes anywhere
        const unsigned char none[4] = {0, 0, 0, 0};
        const DsLayout y = descend_layout(4, L, bound, code_off, none, 1 << 20);
        CHECK(y.max_mv == 0 && y.chunk_mv[0] == 0 && y.plan.max_cost == 32 + 32 + 48 + 32);
    }
    {   // nothing to run
        const DsLayout y = descend_layout(0, L, bound, code_off, mv, 100);
        CHECK(y.plan.chunks.empty() && y.max_io == 0 && y.ws.empty());
    }
}

static void check_intake()
{
    // row_ptr: blocks of rows with a stride of their own each
    const char a[] = "....\0((..))\0", b[] = "x.yy.zz.";
    const char *const rows[2] = {a, b};
    const int stride[2] = {7, 3};
    CHECK(row_ptr(rows, stride, 0, 0) == a && row_ptr(rows, stride, 0, 1) == a + 7 && row_ptr(rows, stride, 1, 2) == b + 6);
    // copy_row_back: the row's bytes up to L or an earlier NUL, then a NUL; nothing behind it is written or read
    {
        std::vector<char> row = {'(', '(', '.', 0}, db(8, '#');          // (an early NUL: the row ends there, and so does the buffer)
        copy_row_back(db.data(), row.data(), 6);
        CHECK(std::string(db.data(), 8) == std::string("((.\0####", 8));
        std::vector<char> full = {'(', '.', '.', '.', ')'}, db2(8, '#'); // (no NUL within L: exactly L bytes are read)
        copy_row_back(db2.data(), full.data(), 5);
        CHECK(std::string(db2.data(), 8) == std::string("(...)\0##", 8));
        std::vector<char> empty = {0}, db3(2, '#');
        copy_row_back(db3.data(), empty.data(), 1);
        CHECK(db3[0] == 0 && db3[1] == '#');
    }
    // FirstError: the lowest (sequence, item) wins, item -1 is the sequence itself, the first note of a place stays
    {
        SeqPack pk;
        pk.status = {0, RAFFT_ERR_EMPTY, 0, RAFFT_ERR_BAD_CHAR};
        pk.first_err = "sequence 1: empty";
        FirstError e(pk);
        CHECK(e.text() == "sequence 1: empty");
        e.note(2, 0, "s2 r0");          CHECK(e.text() == "sequence 1: empty");        // behind the pack's error
        e.note(1, 3, "s1 r3");          CHECK(e.text() == "sequence 1: empty");        // at the sequence that has it: the sequence comes first
        e.note(1, -1, "s1");            CHECK(e.text() == "sequence 1: empty");        // ... and stays (strictly lower only)
        e.note(0, 5, "s0 r5");          CHECK(e.text() == "s0 r5");
        e.note(0, 2, "s0 r2");          CHECK(e.text() == "s0 r2");                    // a note out of order
        e.note(0, 4, "s0 r4");          CHECK(e.text() == "s0 r2");
        e.note(0, 2, "s0 r2 again");    CHECK(e.text() == "s0 r2");
        e.note(0, 0, "s0 r0");          CHECK(e.text() == "s0 r0");
        e.note(0, -1, "s0");            CHECK(e.text() == "s0");                       // item -1 against item 0
        e.note(0, 0, "s0 r0 again");    CHECK(e.text() == "s0");
        e.note(0, -1, "s0 again");      CHECK(e.text() == "s0");
    }
    {
        SeqPack pk;
        pk.status = {0, 0, 0};
        FirstError e(pk);
        CHECK(e.text().empty() && e.at < 0);
        e.note(2, -1, "s2");            CHECK(e.text() == "s2");
        e.note(1, 0x7ffffffell, "s1 last");     CHECK(e.text() == "s1 last");          // the largest item stays below the next sequence
        e.note(1, 0, "s1 r0");          CHECK(e.text() == "s1 r0");
        e.note(2, -1, "s2 again");      CHECK(e.text() == "s1 r0");
    }
    CHECK(std::string("sequence 0 row 0") + ROW_PARSE_ERR == "sequence 0 row 0: malformed, a non-canonical pair, or a hairpin of fewer than 3");
}

int main(int argc, char **argv)
{
    check_sizes();
    check_layout();
    check_intake();
    if ((argc - 1) % 4) { fprintf(stderr, "usage: descend_check [SEQ ROW STATUS PAIRS]...\n"); return 2; }
    for (int k = 1; k + 3 < argc; k += 4) check_case(argv[k], argv[k + 1], atoi(argv[k + 2]), argv[k + 3]);
    printf("%d cases, %d failures\n", (argc - 1) / 4, fails);
    return fails ? 1 : 0;
}
