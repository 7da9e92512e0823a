// Host-side check of the barriers part of rafft_amd/csrc/rafft_hostpure.h: the tree from the edges between basins (barriers_tree)
// on constructed edge lists and on the graphs the test passes in with their expected trees, and the sizes and the layout of a call
// (barriers_layout, the barriers_* sizes of rafft_batch_layout.h) at the edges of the workspace budget against values derived by
// hand.  Plain C++, no HIP, no GPU.
// usage: barriers_check [N_MINIMA EDGES FATHERS SADDLES]...   EDGES = "a-b-t,a-b-t,..." in any order (sorted here as the library
// sorts them), FATHERS and SADDLES = "v,v,..." (N_MINIMA values, -1 for a root).  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include "../../rafft_amd/csrc/rafft_hostpure.h"
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); } } while (0)

typedef std::vector<rafft_barriers_edge> Edges;
typedef std::vector<int32_t> Ints;

static void sort_edges(Edges &ed)
{
    std::sort(ed.begin(), ed.end(), [](const rafft_barriers_edge &u, const rafft_barriers_edge &v) {
        return u.saddle_rank != v.saddle_rank ? u.saddle_rank < v.saddle_rank : u.a != v.a ? u.a < v.a : u.b < v.b;
    });
}

static bool tree_is(int n, Edges ed, const Ints &father, const Ints &saddle)
{
    sort_edges(ed);
    Ints f, s;
    barriers_tree(n, ed, f, s);
    return f == father && s == saddle;
}

static void check_constructed()
{
    // a chain 0 - 1 - 2 - 3 with rising saddles: each hangs under its left neighbour's component root, which is 0 by then
    CHECK(tree_is(4, Edges{{0, 1, 10}, {1, 2, 20}, {2, 3, 30}}, Ints{-1, 0, 0, 0}, Ints{-1, 10, 20, 30}));
    // the same chain with falling saddles: 3 joins 2 first, then {2, 3} joins 1, then all join 0
    CHECK(tree_is(4, Edges{{0, 1, 30}, {1, 2, 20}, {2, 3, 10}}, Ints{-1, 0, 1, 2}, Ints{-1, 30, 20, 10}));
    // a star: one saddle rank merges three components at once; every old root gets the lowest root
    CHECK(tree_is(4, Edges{{1, 2, 7}, {1, 3, 7}, {0, 1, 7}}, Ints{-1, 0, 0, 0}, Ints{-1, 7, 7, 7}));
    // ... and with sub-components formed before: {2, 4} under 2 at 3, {1, 5} under 1 at 4, the star at 9
    CHECK(tree_is(6, Edges{{2, 4, 3}, {1, 5, 4}, {1, 2, 9}, {0, 2, 9}, {2, 3, 9}}, Ints{-1, 0, 0, 0, 2, 1}, Ints{-1, 9, 9, 9, 3, 4}));
    // two components that nothing connects: two roots
    CHECK(tree_is(5, Edges{{0, 2, 5}, {1, 3, 6}, {3, 4, 8}}, Ints{-1, -1, 0, 1, 1}, Ints{-1, -1, 5, 6, 8}));
    // equal saddle ranks in groups that do not touch, and an edge inside a component (no effect)
    CHECK(tree_is(4, Edges{{0, 1, 5}, {2, 3, 5}, {0, 1, 6}, {1, 3, 9}}, Ints{-1, 0, 0, 2}, Ints{-1, 5, 9, 5}));
    // no edges, no minima, one minimum
    CHECK(tree_is(3, Edges{}, Ints{-1, -1, -1}, Ints{-1, -1, -1}));
    CHECK(tree_is(0, Edges{}, Ints{}, Ints{}));
    CHECK(tree_is(1, Edges{}, Ints{-1}, Ints{-1}));
}

static Ints ints_of(const char *text)
{
    Ints v;
    for (const char *p = text; *p;) { char *e; v.push_back((int32_t)strtol(p, &e, 10)); p = *e ? e + 1 : e; }
    return v;
}

static void check_case(int n, const char *edges, const char *fathers, const char *saddles)
{
    Edges ed;
    for (const char *p = edges; *p;) {
        char *e;
        const int a = (int)strtol(p, &e, 10), b = (int)strtol(e + 1, &e, 10), t = (int)strtol(e + 1, &e, 10);
        ed.push_back(rafft_barriers_edge{a, b, t});
        p = *e ? e + 1 : e;
    }
    if (!tree_is(n, ed, ints_of(fathers), ints_of(saddles))) { fails++; fprintf(stderr, "FAIL %d %s: expected %s / %s\n", n, edges, fathers, saddles); }
}

static void check_sizes()
{
    CHECK(barriers_pt_bytes(1) == 16 && barriers_pt_bytes(8) == 16 && barriers_pt_bytes(9) == 32 && barriers_pt_bytes(4096) == 8192);
    CHECK(barriers_lds_bytes(1) == 16 && barriers_lds_bytes(4096) == 8192);
    CHECK(barriers_pow2(0) == 1 && barriers_pow2(1) == 1 && barriers_pow2(3) == 4 && barriers_pow2(4) == 4 && barriers_pow2(5) == 8);
    // 2 n exactly on a power of two, and one row more
    CHECK(barriers_row_slots(1) == 2 && barriers_row_slots(512) == 1024 && barriers_row_slots(513) == 2048 && barriers_row_slots(0) == 2);
    CHECK(barriers_row_slots(RAFFT_BARRIERS_MAX_ROWS) == (1ull << 25));             // (a rank and a mask fit 32 bits)
    for (long long n = 1; n < 5000; n++) CHECK(barriers_row_slots(n) >= 2ull * (unsigned long long)n && barriers_row_slots(n) < 4ull * (unsigned long long)n + 2);
    CHECK(barriers_edge_cap(10, 0) == 1024 && barriers_edge_cap(256, 0) == 1024 && barriers_edge_cap(257, 0) == 1028 && barriers_edge_cap(100000, 0) == 400000);
    CHECK(barriers_edge_cap(100000, 5) == 1024 && barriers_edge_cap(10, 1025) == 1025 && barriers_edge_cap(10, 0x7fffffff) == (1ll << 30));
    CHECK(barriers_edge_slots(1024) == 2048 && barriers_edge_slots(1025) == 4096 && barriers_edge_slots(1ll << 30) == (1ull << 31));
    CHECK(barriers_area_bytes(10, 3, 1024) == 3 * (32 + 24) + 8 * 8 + 12 * 2048);
    CHECK(sizeof(BarSeq) == 64 && sizeof(BarRec) == 24);
    CHECK(sizeof(rafft_barriers_min) == 24 && sizeof(rafft_barriers_edge) == 12 && sizeof(rafft_barriers_seq) == 48 && sizeof(rafft_barriers_result) == 24);
    CHECK(RAFFT_BARRIERS_MAX_LEN <= 32767 && RAFFT_BARRIERS_MAX_ROWS <= (1 << 24));
}

static void check_layout()
{
    // three sequences: 10 nt x 3 rows, 20 nt x 600 rows, 9 nt x 1 row; max_edges 0
    const int L[3] = {10, 20, 9}, n[3] = {3, 600, 1};
    const unsigned long long code_off[3] = {0, 10, 30};
    const size_t a0 = 3 * 56 + 8 * 8 + 12 * 2048, a1 = 600 * (48 + 24) + 8 * 2048 + 12 * 8192, a2 = 1 * 56 + 8 * 2 + 12 * 2048;
    {   // everything fits: one chunk, every buffer from 0
        const BarLayout y = barriers_layout(3, L, n, code_off, 0, 1 << 20);
        CHECK(y.bytes[0] == a0 && y.bytes[1] == a1 && y.bytes[2] == a2);
        CHECK(y.plan.chunks.size() == 1 && y.plan.chunks[0].a == 0 && y.plan.chunks[0].b == 3 && y.max_seqs == 3);
        CHECK(y.qs[0].row0 == 0 && y.qs[1].row0 == 3 && y.qs[2].row0 == 603 && y.chunk_rows[0] == 604);
        CHECK(y.qs[0].pt_off == 0 && y.qs[1].pt_off == 96 && y.qs[2].pt_off == 96 + 600 * 48 && y.chunk_pt[0] == 96 + 600 * 48 + 32);
        CHECK(y.qs[0].tab_off == 0 && y.qs[1].tab_off == 8 && y.qs[2].tab_off == 8 + 2048 && y.chunk_tab[0] == 8 + 2048 + 2);
        CHECK(y.qs[0].tab_mask == 7 && y.qs[1].tab_mask == 2047 && y.qs[2].tab_mask == 1);
        CHECK(y.qs[0].edge_off == 0 && y.qs[1].edge_off == 2048 && y.qs[2].edge_off == 2048 + 8192 && y.chunk_edge[0] == 2048 + 8192 + 2048);
        CHECK(y.qs[0].edge_mask == 2047 && y.qs[1].edge_mask == 8191 && y.qs[0].edge_cap == 1024 && y.qs[1].edge_cap == 2400);
        CHECK(y.qs[1].code_off == 10 && y.qs[1].L == 20 && y.qs[1].n_rows == 600 && y.qs[1].pt_stride == 48 && y.qs[2].pt_stride == 32);
        CHECK(y.chunk_lmax[0] == 20 && y.max_rows == 604);
    }
    {   // exactly the first two, then the third; one byte less: one sequence per chunk
        const BarLayout y = barriers_layout(3, L, n, code_off, 0, a0 + a1);
        CHECK(y.plan.chunks.size() == 2 && y.plan.chunks[0].b == 2 && y.plan.chunks[1].a == 2);
        CHECK(y.qs[2].row0 == 0 && y.qs[2].pt_off == 0 && y.qs[2].tab_off == 0 && y.qs[2].edge_off == 0 && y.chunk_lmax[1] == 9);
        CHECK(y.max_rows == 603 && y.max_tab == 2056 && y.max_edge == 2048 + 8192 && y.max_seqs == 2);
        const BarLayout z = barriers_layout(3, L, n, code_off, 0, a0 + a1 - 1);
        // (the first alone; the third, a little smaller than the first, now joins the second)
        CHECK(z.plan.chunks.size() == 2 && z.plan.chunks[0].b == 1 && z.qs[1].row0 == 0 && z.qs[1].pt_off == 0 && z.qs[1].tab_off == 0 && z.qs[1].edge_off == 0);
        CHECK(z.qs[2].row0 == 600 && z.qs[2].tab_off == 2048 && z.qs[2].edge_off == 8192 && z.max_rows == 601);
        const BarLayout w = barriers_layout(3, L, n, code_off, 0, 1);               // every sequence larger than the workspace: one per chunk
        CHECK(w.plan.chunks.size() == 3 && w.max_seqs == 1 && w.qs[1].row0 == 0 && w.qs[2].row0 == 0 && w.max_rows == 600);
    }
    {   // max_edges given: the caps and the slots follow it
        const BarLayout y = barriers_layout(3, L, n, code_off, 3000, 1 << 20);
        CHECK(y.qs[0].edge_cap == 3000 && y.qs[0].edge_mask == 8191 && y.qs[1].edge_off == 8192);
    }
    {   // nothing to run
        const BarLayout y = barriers_layout(0, L, n, code_off, 0, 100);
        CHECK(y.plan.chunks.empty() && y.qs.empty() && y.max_rows == 0);
    }
}

int main(int argc, char **argv)
{
    check_constructed();
    check_sizes();
    check_layout();
    if ((argc - 1) % 4) { fprintf(stderr, "usage: barriers_check [N_MINIMA EDGES FATHERS SADDLES]...\n"); return 2; }
    for (int k = 1; k + 3 < argc; k += 4) check_case(atoi(argv[k]), argv[k + 1], argv[k + 2], argv[k + 3]);
    printf("%d cases, %d failures\n", (argc - 1) / 4, fails);
    return fails ? 1 : 0;
}
