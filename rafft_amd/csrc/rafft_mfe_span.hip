// rafft_mfe_span.hip - minimum-free-energy folds under a base-pair span (gfx950): the recurrences of rafft_mfe.hip with a pair
// (i,j) allowed iff j - i + 1 <= max_span, for sequences of up to RAFFT_MAX_LEN.  DESIGN.md section 18.  Included by rafft_api.hip
// after rafft_mfe.hip, whose mfe_cell and mfe_traceback run here unchanged over a banded view.
//
// A cell (i,j) with d = j - i < W = min(max_span, L) reads only cells of a smaller d, so the tables are L x W and the fill is W
// launches, one per anti-diagonal, of up to L independent cells each.  The exterior loop is not restricted: F[j] looks at the
// stems (i,j) of the window i >= j - W + 1 and at F[j-1].
#pragma once

#include "rafft_batch_layout.h"     // MfeSpanSeq

#define MFE_SPAN_NT 256
#define MFE_SPAN_AHEAD 8            // rounds of 64 exterior candidates the exterior loop fetches one step ahead
#define MFE_SPAN_TAIL 4             // rounds it fetches together of the candidates beyond them

// The banded view.  A split reads M along a row (k - 1 varies: d varies at a fixed i) and M1 along a column (k varies: d varies at
// a fixed j), so C and M are stored by their 5' end and M1 by its 3' end: the 64 lanes of a split read 64 consecutive words of
// each, as in the views of rafft_mfe.hip.  X[j][d] = C[i][j] + exterior stem (MFE_INF where C is): what the exterior loop reads of
// a column of C, by its 3' end, so that the 64 stems ending at j are 64 consecutive words.
struct MfeTabBand {
    int *C, *M, *M1, *X;
    int W;
    __device__ __forceinline__ size_t by5(int i, int j) const { return (size_t)i * W + (j - i); }
    __device__ __forceinline__ size_t by3(int i, int j) const { return (size_t)j * W + (j - i); }
    __device__ __forceinline__ int &c(int i, int j) const { return C[by5(i, j)]; }
    __device__ __forceinline__ int &m(int i, int j) const { return M[by5(i, j)]; }
    __device__ __forceinline__ int &m1(int i, int j) const { return M1[by3(i, j)]; }
    __device__ __forceinline__ int &x(int i, int j) const { return X[by3(i, j)]; }
};
__device__ __forceinline__ MfeTabBand mfe_span_view(const MfeSpanSeq &q, int *tabs)
{
    int *t0 = tabs + q.tab_off;
    const size_t n = (size_t)mfe_span_table_ints(q.L, q.W);
    return MfeTabBand{t0, t0 + n, t0 + 2 * n, t0 + 3 * n, q.W};
}

// the traceback's walk over the band: 15 bits of i, 15 of d, the table above them; exterior stems from the window's start
struct MfeWalkBand {
    int W;
    __device__ __forceinline__ uint32_t pack(int i, int j, int kind) const { return (uint32_t)i | (uint32_t)(j - i) << 15 | (uint32_t)kind << 30; }
    __device__ __forceinline__ void unpack(uint32_t w, int &i, int &j, int &kind) const { i = (int)(w & 32767u); j = i + (int)((w >> 15) & 32767u); kind = (int)(w >> 30); }
    __device__ __forceinline__ int lo(int j) const { return max(0, j - W + 1); }
    __device__ __forceinline__ int ext(const MfeTabBand &tb, const SmallT *, const uint8_t *, int, int i, int j) const { return tb.x(i, j); }
};

// anti-diagonal d of the sequences order[0 .. gridDim.y), four cells per workgroup and round
__global__ __launch_bounds__(MFE_SPAN_NT) void mfe_span_diag_kernel(const EnergyTables *ET, const MfeSpanSeq *seqs, const int *order, const uint8_t *codes, int *tabs, int d)
{
    const MfeSpanSeq q = seqs[order[blockIdx.y]];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= q.W) return;
    const MfeTabBand tb = mfe_span_view(q, tabs);
    const uint8_t *S = codes + q.code_off;
    const SmallT *T = &ET->s;
    for (int i = blockIdx.x * (MFE_SPAN_NT / 64) + wave; i + d < L; i += gridDim.x * (MFE_SPAN_NT / 64)) {
        const int j = i + d;
        mfe_cell(tb, MfeConNone(), MfeCutNone(), T, &ET->b, S, L, i, j, lane);
        if (lane == 0) {
            const int c = tb.c(i, j);
            tb.x(i, j) = c < MFE_INFH ? c + mfe_stem_ext(T, S, L, i, j) : MFE_INF;
        }
    }
}

// The steps of the exterior loop of one sequence, F[j + 1] = min(F[j], min over d in 4 .. min(j, W - 1) of F[j - d] + X[j][d]).  The
// rows of X do not depend on F: the first NR rounds of 64 candidates of step j + 1 are on their way while step j is reduced, and a
// band wider than 4 + 64 MFE_SPAN_AHEAD reads the rest MFE_SPAN_TAIL rounds at a time.  NR is a template parameter so that the
// loop of a narrow band holds no round it does not need and no branch between its loads (a count in a register cost more time
// than it saved: DESIGN.md section 18).
template <int NR>
__device__ inline void mfe_span_exterior_steps(const int *X, int L, int W, int *F, int lane)
{
    auto fetch = [&](int j, int r) {
        const int d = 4 + lane + 64 * r;
        return d < W && d <= j ? X[(size_t)j * W + d] : MFE_INF;
    };
    int nx[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) nx[r] = MFE_INF;               // (step 0 has no candidate)
    for (int j = 0; j < L; j++) {
        int cur[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) cur[r] = nx[r];
        if (j + 1 < L) {
#pragma unroll
            for (int r = 0; r < NR; r++) nx[r] = fetch(j + 1, r);
        }
        int best = MFE_INF;
#pragma unroll
        for (int r = 0; r < NR; r++)
            if (cur[r] < MFE_INFH) best = min(best, F[j - (4 + lane + 64 * r)] + cur[r]);
        if (NR == MFE_SPAN_AHEAD) {
            const int dmax = min(W - 1, j);
            for (int d0 = 4 + lane + 64 * MFE_SPAN_AHEAD; d0 <= dmax; d0 += 64 * MFE_SPAN_TAIL) {
                int e[MFE_SPAN_TAIL];
#pragma unroll
                for (int r = 0; r < MFE_SPAN_TAIL; r++) e[r] = d0 + 64 * r <= dmax ? X[(size_t)j * W + d0 + 64 * r] : MFE_INF;
#pragma unroll
                for (int r = 0; r < MFE_SPAN_TAIL; r++)
                    if (e[r] < MFE_INFH) best = min(best, F[j - (d0 + 64 * r)] + e[r]);
            }
        }
        best = mfe_wave_min(best);
        const int prev = F[j];
        if (lane == 0) F[j + 1] = min(prev, best);
        wave_sync();
    }
}

// One wavefront a sequence: the exterior loop, L dependent steps; F in LDS, copied out at the end
__global__ __launch_bounds__(64) void mfe_span_exterior_kernel(const MfeSpanSeq *seqs, const int *order, const int *tabs, int *fs)
{
    extern __shared__ __align__(16) int mfe_span_lds[];
    int *F = mfe_span_lds;
    const MfeSpanSeq q = seqs[order[blockIdx.x]];
    const int L = q.L, W = q.W, lane = (int)threadIdx.x;
    const int *X = tabs + q.tab_off + 3 * (size_t)mfe_span_table_ints(L, W);
    if (lane == 0) F[0] = 0;
    wave_sync();
    static_assert(MFE_SPAN_AHEAD == 8, "one case a round count");
    switch ((W - 4 + 63) / 64) {                                // rounds of 64 candidates d = 4 .. W - 1: the same in every lane
    case 0: case 1: mfe_span_exterior_steps<1>(X, L, W, F, lane); break;
    case 2: mfe_span_exterior_steps<2>(X, L, W, F, lane); break;
    case 3: mfe_span_exterior_steps<3>(X, L, W, F, lane); break;
    case 4: mfe_span_exterior_steps<4>(X, L, W, F, lane); break;
    case 5: mfe_span_exterior_steps<5>(X, L, W, F, lane); break;
    case 6: mfe_span_exterior_steps<6>(X, L, W, F, lane); break;
    case 7: mfe_span_exterior_steps<7>(X, L, W, F, lane); break;
    default: mfe_span_exterior_steps<MFE_SPAN_AHEAD>(X, L, W, F, lane); break;
    }
    int *out = fs + q.f_off;
    for (int x = lane; x <= L; x += 64) out[x] = F[x];
}

// One wavefront a sequence: mfe_traceback over the band, F (then the pair table) in LDS
__global__ __launch_bounds__(64) void mfe_span_traceback_kernel(const EnergyTables *ET, const MfeSpanSeq *seqs, const int *order, const uint8_t *codes, int *tabs,
                                                               const int *fs, uint32_t *stacks, char *db, int4 *rec)
{
    extern __shared__ __align__(16) int mfe_span_lds[];
    int *F = mfe_span_lds;
    const int s = order[blockIdx.x];
    const MfeSpanSeq q = seqs[s];
    const int L = q.L, lane = (int)threadIdx.x;
    const int *in = fs + q.f_off;
    for (int x = lane; x <= L; x += 64) F[x] = in[x];
    wave_sync();
    mfe_traceback(mfe_span_view(q, tabs), MfeWalkBand{q.W}, MfeConNone(), MfeCutNone(), &ET->s, &ET->b, codes + q.code_off, L, F, stacks + q.stack_off, L + 8, db + q.db_off, rec + s, lane);
}
