// rafft_cofold.hip - minimum-free-energy folds of two-strand dimers (gfx950): mfe_cell, mfe_exterior and mfe_traceback of
// rafft_mfe.hip under the cut policy MfeCut.  DESIGN.md section 22.  Included by rafft_api.hip, after rafft_mfe.hip.
//
// The model.  A dimer is the concatenation S = A B of length L = La + Lb <= RAFFT_MFE_MAX_LEN with cut c = La: position c is the
// first base of B, the nick is the missing backbone bond between c-1 and c.  Write x(i,j) for i < c <= j (a cross cell).
//   Ensemble: canonical non-crossing pairs; (i,j) on one strand needs j - i - 1 >= 3, a cross pair any j - i >= 1; real interior
//   loops have at most 30 unpaired positions.
//   Energy: the nick lies in exactly one loop - the exterior loop if no pair spans it, else the loop closed by the innermost
//   spanning pair.  Every other loop has the energy rafft_eval_structure gives it.  The loop with the nick and the exterior loop are
//   both exterior loops: 0 for unpaired positions, e_stem(.., ext = true) for every stem in them - the pair that closes the nick
//   loop read from inside, rtype(t) with neighbours S[j-1], S[i+1] - and a neighbour across a strand end does not exist (the 5'
//   neighbour of p exists iff p > 0 && p != c, the 3' neighbour of q iff q < L-1 && q+1 != c).  duplex_init is added once iff a
//   pair spans the nick.  No symmetry correction for A == B.
//   C[i][j]   intra cell: as rafft_mfe.hip.  Cross cell: no hairpin; the nick loop stem_ext_inside(i,j) + FA[i+1] + FB[j-1];
//             interior loops whose inner pair is a cross pair too; the multiloop term if i+1 != c && j != c
//   M1[i][j]  min(C[i][j] + stem_ml if i != c && j+1 != c, M1[i][j-1] + ml_base if j != c)
//   M[i][j]   min(M1[i][j], M[i+1][j] + ml_base if i+1 != c, min_k M[i][k-1] + M1[k][j] if k != c)
//   FB[j]     j >= c, exterior energy of c..j: min(FB[j-1], min_{i >= c} FB[i-1] + C[i][j] + stem_ext(i,j)), FB[c-1] = 0
//   FA[i]     i < c, exterior energy of i..c-1: min(FA[i+1], min_{j < c} C[i][j] + stem_ext(i,j) + FA[j+1]), FA[c] = 0
//   F[j]      min(F[j-1], min_i F[i-1] + C[i][j] + stem_ext(i,j) + (x(i,j) ? duplex_init : 0))
// FA and FB read intra cells only, a cross cell reads FA, FB and cells of a smaller j - i: three phases - the intra cells of both
// strands by anti-diagonal, one wavefront for FA and FB (cofold_ends), the cross cells by anti-diagonal.
// The traceback order: cross C - the nick loop; interior loops, p ascending then q descending; splits, k ascending.  FB as F: j
// unpaired, stems with i ascending from c.  FA: i unpaired, stems (i,j) with j ascending.  M, M1, F as rafft_mfe.hip.
// A sequence with cut 0 is a single strand: a workgroup-uniform branch folds it under MfeCutNone, as mfe_*_kernel folds it.
#pragma once

#include "rafft_mfe.hip"

// One wavefront: G (L + 1 ints, MfeCut) of a dimer whose intra cells are filled
template <class Tab>
__device__ inline void cofold_ends(const Tab &tb, const MfeWalkCut &wk, const SmallT *T, const uint8_t *S, int L, int c, int *G, int lane)
{
    if (lane == 0) G[c] = 0;
    wave_sync();
    for (int j = c; j < L; j++) {
        int best = MFE_INF;
        for (int i = c + lane; i <= j - 4; i += 64) {
            const int e = wk.ext(tb, T, S, L, i, j);
            if (e < MFE_INFH) best = min(best, G[i] + e);
        }
        best = mfe_wave_min(best);
        if (lane == 0) G[j + 1] = min(G[j], best);
        wave_sync();
    }
    for (int i = c - 1; i >= 0; i--) {
        int best = MFE_INF;
        for (int j = i + 4 + lane; j < c; j += 64) {
            const int e = wk.ext(tb, T, S, L, i, j);
            if (e < MFE_INFH) best = min(best, e + G[j + 1]);
        }
        best = mfe_wave_min(best);
        if (lane == 0) G[i] = min(G[i + 1], best);
        wave_sync();
    }
}

// LDS class: a workgroup folds the dimer s with cut c > 0 in the three phases; tables, F, bases and G in LDS
__device__ __forceinline__ void cofold_lds_fold(const MfeTabLds &tb, const MfeCut &ct, const EnergyTables *ET, const MfeSeq &q, int *F, int *G, const uint8_t *S,
                                                uint32_t *stacks, char *db, int4 *rec)
{
    const int L = q.L, c = ct.c, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SmallT *T = &ET->s;
    const BigT *B = &ET->b;
    const MfeWalkCut wk(ct);
    for (int d = 0; d < max(c, L - c); d++) {
        for (int i = wave; i + d < L; i += MFE_LDS_NT / 64)
            if (!ct.x(i, i + d)) mfe_cell(tb, MfeConNone(), ct, T, B, S, L, i, i + d, lane);
        __syncthreads();
    }
    if (wave == 0) cofold_ends(tb, wk, T, S, L, c, G, lane);
    __syncthreads();
    for (int d = 1; d < L; d++) {
        for (int i = max(0, c - d) + wave; i < c && i + d < L; i += MFE_LDS_NT / 64) mfe_cell(tb, MfeConNone(), ct, T, B, S, L, i, i + d, lane);
        __syncthreads();
    }
    if (wave == 0) {
        mfe_exterior(tb, wk, MfeConNone(), ct, T, S, L, F, lane);
        mfe_traceback(tb, wk, MfeConNone(), ct, T, B, S, L, F, stacks + q.stack_off, L + 8, db + q.db_off, rec, lane);
    }
}
// workgroup b folds sequence order[b], cut at cuts[order[b]]; G behind the bases (cofold_lds_bytes)
__global__ __launch_bounds__(MFE_LDS_NT) void cofold_lds_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes, const int *cuts,
                                                               int dinit, uint32_t *stacks, char *db, int4 *rec)
{
    extern __shared__ __align__(16) int mfe_lds[];
    const int s = order[blockIdx.x];
    const MfeSeq q = seqs[s];
    const int c = cuts[s];
    const int L = q.L, N = L * (L + 1) / 2, tid = threadIdx.x;
    const MfeTabLds tb{mfe_lds, mfe_lds + N, mfe_lds + 2 * N, L};
    int *F = mfe_lds + 3 * N;
    uint8_t *S = (uint8_t *)(F + L + 1);
    int *G = mfe_lds + mfe_lds_bytes(L) / 4;
    for (int x = tid; x < L; x += MFE_LDS_NT) S[x] = codes[q.code_off + x];
    __syncthreads();
    if (c) cofold_lds_fold(tb, MfeCut{c, dinit, G}, ET, q, F, G, S, stacks, db, rec + s);
    else mfe_lds_fold(tb, MfeConNone(), ET, q, F, S, stacks, db, rec + s);
}

// HBM class: anti-diagonal d of the sequences order[0 .. gridDim.y), the intra cells (cross = 0) or the cross cells (cross = 1);
// ends: G of a sequence at its stack_off (the L + 1 ints cofold_ends_kernel wrote, read by the cross cells)
__global__ __launch_bounds__(MFE_HBM_NT) void cofold_diag_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes, const int *cuts,
                                                                int dinit, const int *ends, int *tabs, int d, int cross)
{
    const int s = order[blockIdx.y];
    const MfeSeq q = seqs[s];
    if (d >= q.L) return;
    const int c = cuts[s];
    if (!c) {
        if (!cross) mfe_diag_fill(MfeConNone(), ET, q, codes, tabs, d);
        return;
    }
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int *t0 = tabs + q.tab_off;
    const size_t LL = (size_t)L * L;
    const MfeTabHbm tb{t0, t0 + LL, t0 + 2 * LL, L};
    const uint8_t *S = codes + q.code_off;
    const MfeCut ct{c, dinit, ends + q.stack_off};
    const int w0 = blockIdx.x * (MFE_HBM_NT / 64) + wave, step = gridDim.x * (MFE_HBM_NT / 64);
    if (cross) {
        for (int i = max(0, c - d) + w0; i < c && i + d < L; i += step) mfe_cell(tb, MfeConNone(), ct, &ET->s, &ET->b, S, L, i, i + d, lane);
    } else {
        for (int i = w0; i + d < L; i += step)
            if (!ct.x(i, i + d)) mfe_cell(tb, MfeConNone(), ct, &ET->s, &ET->b, S, L, i, i + d, lane);
    }
}
// one wavefront per sequence: G of a dimer from its intra cells, in LDS and from there to `ends`
__global__ __launch_bounds__(64) void cofold_ends_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes, const int *cuts, int *ends,
                                                        int *tabs)
{
    __shared__ int G[RAFFT_MFE_MAX_LEN + 1];
    const int s = order[blockIdx.x];
    const MfeSeq q = seqs[s];
    const int c = cuts[s], L = q.L, lane = (int)threadIdx.x;
    if (!c) return;
    int *t0 = tabs + q.tab_off;
    const size_t LL = (size_t)L * L;
    const MfeTabHbm tb{t0, t0 + LL, t0 + 2 * LL, L};
    cofold_ends(tb, MfeWalkCut(MfeCut{c, 0, G}), &ET->s, codes + q.code_off, L, c, G, lane);
    for (int x = lane; x <= L; x += 64) ends[q.stack_off + x] = G[x];
}
// the exterior loop and the traceback, one wavefront per sequence; F and G in LDS
__global__ __launch_bounds__(64) void cofold_traceback_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes, const int *cuts,
                                                             int dinit, const int *ends, int *tabs, uint32_t *stacks, char *db, int4 *rec)
{
    __shared__ int F[RAFFT_MFE_MAX_LEN + 1];
    __shared__ int G[RAFFT_MFE_MAX_LEN + 1];
    const int s = order[blockIdx.x];
    const MfeSeq q = seqs[s];
    const int c = cuts[s], L = q.L, lane = (int)threadIdx.x;
    if (!c) {
        mfe_hbm_trace(MfeConNone(), ET, q, codes, tabs, F, stacks, db, rec + s);
        return;
    }
    for (int x = lane; x <= L; x += 64) G[x] = ends[q.stack_off + x];
    wave_sync();
    int *t0 = tabs + q.tab_off;
    const size_t LL = (size_t)L * L;
    const MfeTabHbm tb{t0, t0 + LL, t0 + 2 * LL, L};
    const MfeCut ct{c, dinit, G};
    const MfeWalkCut wk(ct);
    mfe_exterior(tb, wk, MfeConNone(), ct, &ET->s, codes + q.code_off, L, F, lane);
    mfe_traceback(tb, wk, MfeConNone(), ct, &ET->s, &ET->b, codes + q.code_off, L, F, stacks + q.stack_off, L + 8, db + q.db_off, rec + s, lane);
}
