// rafft_score.hip - accuracy of whole beams against known structures on the GPU.
//
// Replaces the scoring half of the reference's benchmark, benchmark_results/scoring.py:76-94: every structure of a beam is
// compared with the sequence's known structure (RNAstructure `scorer`: PPV and sensitivity, one position of slip) and the last
// structure that reaches the highest PPV is kept (`>=`), or the first one (`--one`).
//
// Tables: t[x] = partner of x, 1-based, 0 = unpaired, 16 bits per position.  K = the known structure's table (built on the host,
// one per sequence), P = a predicted row's table (built here, one wavefront per row).  A predicted pair (i, j), i < j, is found
// in the known structure when K holds (i, j), (i +- 1, j) or (i, j +- 1):  K[i] in {j - 1, j, j + 1}  or  K[j] in {i - 1, i + 1}
// (partners outside 0..L-1 do not exist); the same with the roles swapped for a known pair against P.  Integer work only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rafft_hip.h"

struct ScoreSeq {                        // one sequence of the call
    unsigned long long rows_off;         // first row, bytes into the device copy of the rows
    unsigned int known_off;              // K, 16-bit elements into the known tables
    int L, n_rows, stride, row0;         // row0: index of the first row record
    int n_known, status;                 // status != 0: no row of it is scored
    int _pad;
};
struct ScoreItem { int seq, r0, r1; };   // a workgroup's share: rows [r0, r1) of one sequence

#define SC_NT 256
#define SC_WAVES (SC_NT / 64)
#define SC_ROWS 16                       // rows per work item: 4 per wavefront
#define SC_L_SMALL 512                   // LDS plans: 14 bytes per position (K, and per wavefront P and the stack of open positions)
#define SC_L_LDS 4608                    // 63 KiB; longer sequences keep K, P and the stacks in global memory

// writes of one lane, reads of another, same wavefront
template <bool LDS>
__device__ __forceinline__ void score_wave_sync()
{
    if (LDS) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int score_wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);      // fixed tree
    return v;
}

// One wavefront parses `row` (L characters of ( ) .) into P, 64 characters per step: brackets that close inside the chunk are
// matched from the two ballot masks in rounds (a `)` whose nearest unmatched bracket to the left is a `(` takes it: one round per
// nesting level of the chunk), what stays is `)))(((`: the closes take the top of the stack of open positions carried from the
// chunks before, the opens are pushed.  Returns false (for the whole wavefront) for another character or an unbalanced row; P is
// then incomplete.  stk holds L / 2 entries: a deeper nesting cannot close within L.
template <bool LDS>
__device__ __forceinline__ bool score_parse_row(const char *row, int L, uint16_t *P, uint16_t *stk, int lane)
{
    const unsigned long long bit = 1ull << lane, below = bit - 1, above = ~below & ~bit;
    const int cap = L / 2;
    int top = 0;
    char c_next = lane < L ? row[lane] : '.';
    for (int base = 0; base < L; base += 64) {
        const int x = base + lane;
        const char c = c_next;
        if (base + 64 < L) c_next = x + 64 < L ? row[x + 64] : '.';
        unsigned long long O = __ballot(c == '('), C = __ballot(c == ')');
        if (__ballot(c != '(' && c != ')' && c != '.')) return false;
        if (x < L && c == '.') P[x] = 0;
        for (;;) {
            const unsigned long long B = O | C;
            bool mc = false, mo = false;
            if (C & bit) {
                const unsigned long long m = B & below;
                if (m) {
                    const int q = 63 - __clzll((long long)m);
                    if ((O >> q) & 1) { mc = true; P[base + q] = (uint16_t)(x + 1); P[x] = (uint16_t)(base + q + 1); }
                }
            } else if (O & bit) {
                const unsigned long long m = B & above;
                if (m) mo = (C >> (__ffsll((long long)m) - 1)) & 1;
            }
            const unsigned long long MC = __ballot(mc);
            if (!MC) break;
            C &= ~MC;
            O &= ~__ballot(mo);
        }
        const int nc = __popcll(C), no = __popcll(O);
        if (nc > top) return false;
        if (C & bit) {
            const int q = stk[top - 1 - __popcll(C & below)];
            P[q] = (uint16_t)(x + 1); P[x] = (uint16_t)(q + 1);
        }
        top -= nc;
        if (top + no > cap) return false;
        score_wave_sync<LDS>();                       // the pops above read what the pushes below overwrite
        if (O & bit) stk[top + __popcll(O & below)] = (uint16_t)x;
        top += no;
        score_wave_sync<LDS>();
    }
    return top == 0;
}

// grid: work items (grid-stride); the known table is staged once per item, each wavefront takes every fourth row of the item.
// LDS = false: K is read through the caches, P and the stacks live in `scratch` (6 * Lc 16-bit elements per workgroup, by
// blockIdx: per wavefront P of Lc and a stack of Lc / 2).
// Lc: positions the plan is laid out for (even, >= every L of the launch).
template <bool LDS>
__global__ __launch_bounds__(SC_NT) void score_rows_kernel(int n_items, const ScoreItem *items, const ScoreSeq *seqs, const char *rows,
                                                            const uint16_t *known, int Lc, uint16_t *scratch, rafft_score_row *row_out)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t sc_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const ScoreItem item = items[it];
        const ScoreSeq sq = seqs[item.seq];
        const int L = sq.L;
        const uint16_t *K;
        uint16_t *P;
        if constexpr (LDS) {
            __syncthreads();                          // the item before is done with K
            for (int x = threadIdx.x; x < L; x += SC_NT) sc_lds[x] = known[sq.known_off + x];
            __syncthreads();
            K = sc_lds;
            P = sc_lds + Lc + wv * (Lc + Lc / 2);
        } else {
            K = known + sq.known_off;
            P = scratch + ((size_t)blockIdx.x * SC_WAVES + wv) * (size_t)(Lc + Lc / 2) ;
        }
        uint16_t *stk = P + Lc;
        for (int r = item.r0 + wv; r < item.r1; r += SC_WAVES) {
            score_wave_sync<LDS>();                   // the row before is done with P
            const bool ok = score_parse_row<LDS>(rows + sq.rows_off + (size_t)r * (size_t)sq.stride, L, P, stk, lane);
            score_wave_sync<LDS>();
            int n_pred = 0, hit_pred = 0, hit_known = 0, n_exact = 0;
            if (ok) {
                for (int x = lane; x < L; x += 64) {
                    const int p = P[x], k = K[x];
                    if (p > x + 1) {                  // x opens the predicted pair (x, p - 1)
                        const int kj = K[p - 1];
                        n_pred++;
                        hit_pred += (k >= p - 1 && k <= p + 1) || (kj != 0 && (kj == x || kj == x + 2));
                        n_exact += k == p;
                    }
                    if (k > x + 1) {                  // x opens the known pair (x, k - 1)
                        const int pj = P[k - 1];
                        hit_known += (p >= k - 1 && p <= k + 1) || (pj != 0 && (pj == x || pj == x + 2));
                    }
                }
                n_pred = score_wave_sum(n_pred); hit_pred = score_wave_sum(hit_pred);
                hit_known = score_wave_sum(hit_known); n_exact = score_wave_sum(n_exact);
            }
            if (lane == 0) {
                rafft_score_row o;
                o.n_pred = n_pred; o.hit_pred = hit_pred; o.hit_known = hit_known; o.n_exact = n_exact;
                o.status = ok ? RAFFT_OK : RAFFT_ERR_STRUCT;
                row_out[(size_t)sq.row0 + r] = o;
            }
        }
    }
}

// a PPV as a fraction, and the row it belongs to; a row without pairs counts as 0 / 1
struct ScorePick { long long hit, n; int row; };

// b replaces a: in row order `>=` keeps the last row of the highest PPV (scoring.py:90-91); hit_b / n_b >= hit_a / n_a in integers
__device__ __forceinline__ bool score_pick_takes(const ScorePick &a, const ScorePick &b)
{
    if (b.row < 0) return false;
    if (a.row < 0) return true;
    const long long l = b.hit * a.n, r = a.hit * b.n;
    return l > r || (l == r && b.row > a.row);
}

// One wavefront per sequence: the last row with the highest PPV among the rows that parsed, and row 0.
__global__ __launch_bounds__(SC_NT) void score_pick_kernel(int n_seq, const ScoreSeq *seqs, const rafft_score_row *row_out, rafft_score_seq *seq_out)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (s >= n_seq) return;
    const ScoreSeq sq = seqs[s];
    const int n_rows = sq.status ? 0 : sq.n_rows;
    const rafft_score_row *rec = row_out + sq.row0;
    ScorePick best = {0, 1, -1};
    for (int r = lane; r < n_rows; r += 64) {
        if (rec[r].status) continue;
        const ScorePick c = {rec[r].n_pred ? rec[r].hit_pred : 0, rec[r].n_pred ? rec[r].n_pred : 1, r};
        if (score_pick_takes(best, c)) best = c;
    }
    for (int o = 32; o > 0; o >>= 1) {
        ScorePick c;
        c.hit = __shfl_down(best.hit, o, 64); c.n = __shfl_down(best.n, o, 64); c.row = __shfl_down(best.row, o, 64);
        if (score_pick_takes(best, c)) best = c;
    }
    if (lane) return;
    rafft_score_seq *o = seq_out + s;
    o->status = sq.status; o->n_known = sq.n_known; o->n_rows = sq.n_rows; o->row0 = sq.row0;
    o->pick_ppv = best.row; o->pick_first = n_rows > 0 ? 0 : -1;
    const rafft_score_row *pb = rec + (best.row >= 0 ? best.row : 0), *pf = rec;      // read only when there is such a row
    const bool hb = best.row >= 0, hf = n_rows > 0;
    o->best.n_pred = hb ? pb->n_pred : 0; o->best.hit_pred = hb ? pb->hit_pred : 0; o->best.hit_known = hb ? pb->hit_known : 0;
    o->best.n_exact = hb ? pb->n_exact : 0; o->best.status = hb ? pb->status : sq.status;
    o->first.n_pred = hf ? pf->n_pred : 0; o->first.hit_pred = hf ? pf->hit_pred : 0; o->first.hit_known = hf ? pf->hit_known : 0;
    o->first.n_exact = hf ? pf->n_exact : 0; o->first.status = hf ? pf->status : sq.status;
}
