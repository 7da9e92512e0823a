// rafft_mea.hip - maximum-expected-accuracy structures of a batch (gfx950): from a matrix of pair probabilities (or pair
// frequencies) P the unpaired probabilities q, the weights W = (gamma + gamma) P, the table
//   E[i][j] = max(E[i][j-1] + q_j,  max over candidates (k,j), i <= k < j, of (E[i][k-1] + W(k,j)) + E[k+1][j-1]),  E[i][j] = 0 for j < i
// (a candidate is a cell with P > 0), mea = E[0][L-1], the row a traceback with a fixed order reads off E, and the ensemble
// diversity sum 2 P (1 - P).  DESIGN.md section 17.  Included by rafft_api.hip, after rafft_pf.hip.
// Every cell is formed by additions of stored values only (W is rounded once, in mea_prepare_kernel), so a numpy restatement
// reproduces the bits (tests/_mea_np.py); the maximum of a cell does not depend on the order of its candidates.
// One size class: full L x L fp64 tables in device memory, one launch per anti-diagonal (stream order is the synchronisation), one
// wavefront per cell, candidates over the 64 lanes.  The three reads of candidate k are consecutive in k: E[i][k-1] along row i,
// E[k+1][j-1] from the transposed copy ET[j-1][k+1], W(k,j) from the transposed WT[j][k].
#pragma once

#include "rafft_batch_layout.h"     // MeaSeq

#define MEA_NT 256
#define MEA_TILE 32

struct MeaTab {
    const double *P;
    double *WT, *E, *ET;
    int L;
    __device__ __forceinline__ double p(int i, int j) const { return P[(size_t)i * L + j]; }
    __device__ __forceinline__ double &wt(int k, int j) const { return WT[(size_t)j * L + k]; }
    __device__ __forceinline__ double &e(int i, int j) const { return E[(size_t)i * L + j]; }
    __device__ __forceinline__ double &et(int i, int j) const { return ET[(size_t)j * L + i]; }
    // the value of candidate (k,j) in the interval that starts at i, in the association of the definition
    __device__ __forceinline__ double cand(int i, int k, int j, double w) const
    {
        const double left = k > i ? e(i, k - 1) : 0.0, inner = k + 1 <= j - 1 ? et(k + 1, j - 1) : 0.0;
        return (left + w) + inner;
    }
};
__device__ __forceinline__ MeaTab mea_tab(double *ws, const MeaSeq &q) { return MeaTab{ws + q.p_off, ws + q.wt_off, ws + q.e_off, ws + q.et_off, q.L}; }

// max over the 64 lanes of a wavefront (all of them active), the same bits in every lane.  No value is a NaN or -0
__device__ __forceinline__ double mea_wave_max(double x)
{
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// From P of the sequences order[0 .. gridDim.y): q (one thread per position: the partners in ascending order, one running sum),
// the position's share of the diversity (its partners above it, ascending; mea_traceback_kernel adds the shares up), and WT, tile
// by tile through LDS so that P is read along its rows and WT written along its rows.  aux of a sequence: q (L), the shares (L),
// the diversity (1).
__global__ __launch_bounds__(MEA_NT) void mea_prepare_kernel(const MeaSeq *seqs, const int *order, double *ws, double *aux, double gamma)
{
    __shared__ double tile[MEA_TILE][MEA_TILE + 1];
    const MeaSeq q = seqs[order[blockIdx.y]];
    const int L = q.L;
    const MeaTab tb = mea_tab(ws, q);
    double *qq = aux + q.aux_off, *share = qq + L;
    for (int i = blockIdx.x * MEA_NT + threadIdx.x; i < L; i += gridDim.x * MEA_NT) {
        double s = 0.0, dv = 0.0;
        for (int p = 0; p < i; p++) s += tb.p(p, i);
        for (int p = i + 1; p < L; p++) {
            const double x = tb.p(i, p);
            s += x;
            dv += (x + x) * (1.0 - x);
        }
        qq[i] = fmax(0.0, 1.0 - s);
        share[i] = dv;
    }
    const double g2 = gamma + gamma;
    const int nt = (L + MEA_TILE - 1) / MEA_TILE, tx = threadIdx.x % MEA_TILE, ty = threadIdx.x / MEA_TILE;
    for (int t = blockIdx.x; t < nt * nt; t += gridDim.x) {
        const int k0 = (t / nt) * MEA_TILE, j0 = (t % nt) * MEA_TILE;       // rows k0.. of P, columns j0..
        __syncthreads();
        for (int r = ty; r < MEA_TILE; r += MEA_NT / MEA_TILE) {
            const int k = k0 + r, j = j0 + tx;
            tile[r][tx] = k < L && j < L && k < j ? g2 * tb.p(k, j) : 0.0;
        }
        __syncthreads();
        for (int r = ty; r < MEA_TILE; r += MEA_NT / MEA_TILE) {
            const int j = j0 + r, k = k0 + tx;
            if (j < L && k < L) tb.wt(k, j) = tile[tx][r];
        }
    }
}

// one wavefront fills cell (i,j) of E and ET; every cell of a smaller j - i is there
__device__ __forceinline__ void mea_cell(const MeaTab &tb, const double *qq, int i, int j, int lane)
{
    double best = (j > i ? tb.e(i, j - 1) : 0.0) + qq[j];
    for (int k = i + lane; k < j; k += 64) {
        const double w = tb.wt(k, j);
        if (w != 0.0) best = fmax(best, tb.cand(i, k, j, w));
    }
    best = mea_wave_max(best);
    if (lane == 0) { tb.e(i, j) = best; tb.et(i, j) = best; }
}

// anti-diagonal d of the sequences order[0 .. gridDim.y), four cells per workgroup and round
__global__ __launch_bounds__(MEA_NT) void mea_diag_kernel(const MeaSeq *seqs, const int *order, double *ws, const double *aux, int d)
{
    const MeaSeq q = seqs[order[blockIdx.y]];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= L) return;
    const MeaTab tb = mea_tab(ws, q);
    const double *qq = aux + q.aux_off;
    for (int i = blockIdx.x * (MEA_NT / 64) + wave; i + d < L; i += gridDim.x * (MEA_NT / 64)) mea_cell(tb, qq, i, i + d, lane);
}

#define MEA_BAD_STACK 1             // more pending intervals than the stack holds (cannot happen: a pair leaves one behind)
#define MEA_BAD_CELL 2              // a cell that neither the unpaired term nor a candidate reproduces

// One wavefront per sequence: the diversity (the shares of mea_prepare_kernel: lane x adds those of x, x + 64, ..., then a butterfly
// of fixed order), and the row.  Intervals (i | j << 16) wait on a stack in device memory that lane 0 owns; of an interval the
// last position is unpaired when E[i][j] == E[i][j-1] + q_j, else it pairs with the first k ascending whose candidate has the bits
// of E[i][j]: 64 candidates per ballot, the lowest set lane wins.  The pair table (int16, -1 = unpaired: what eval_kernel reads),
// then the row, the number of pairs and mea into the record.
__global__ __launch_bounds__(64) void mea_traceback_kernel(const MeaSeq *seqs, const int *order, double *ws, double *aux, uint32_t *stacks, int16_t *pts,
                                                           char *db, MeaRec *rec)
{
    __shared__ int16_t pt[RAFFT_MFE_MAX_LEN];
    const int s = order[blockIdx.x], lane = (int)threadIdx.x;
    const MeaSeq q = seqs[s];
    const int L = q.L, cap = L + 8;
    const MeaTab tb = mea_tab(ws, q);
    const double *qq = aux + q.aux_off, *share = qq + L;
    uint32_t *stack = stacks + q.stack_off;
    double dv = 0.0;
    for (int x = lane; x < L; x += 64) { dv += share[x]; pt[x] = -1; }
    for (int o = 32; o > 0; o >>= 1) dv += __shfl_xor(dv, o, 64);
    wave_sync();
    int sp = 0, npairs = 0, bad = 0;
    if (lane == 0) stack[0] = (uint32_t)(L - 1) << 16;
    sp = 1;
    while (sp > 0 && !bad) {
        sp--;
        uint32_t w = 0;
        if (lane == 0) w = stack[sp];
        w = (uint32_t)__shfl((int)w, 0, 64);
        const int i = (int)(w & 0xffffu);
        int j = (int)(w >> 16);
        while (j >= i) {
            const double v = tb.e(i, j);
            if (v == (j > i ? tb.e(i, j - 1) : 0.0) + qq[j]) { j--; continue; }
            int found = -1;
            for (int k0 = i; k0 < j && found < 0; k0 += 64) {
                const int k = k0 + lane;
                bool hit = false;
                if (k < j) {
                    const double wk = tb.wt(k, j);
                    hit = wk != 0.0 && tb.cand(i, k, j, wk) == v;
                }
                const unsigned long long bal = __ballot(hit);
                if (bal) found = k0 + __ffsll((long long)bal) - 1;
            }
            if (found < 0) { bad = MEA_BAD_CELL; break; }
            if (lane == 0) { pt[found] = (int16_t)j; pt[j] = (int16_t)found; }
            npairs++;
            if (found > i) {                            // (i, found - 1) waits; (found + 1, j - 1) goes on
                if (sp >= cap) { bad = MEA_BAD_STACK; break; }
                if (lane == 0) stack[sp] = (uint32_t)i | (uint32_t)(found - 1) << 16;
                sp++;
            }
            w = (uint32_t)(found + 1) | (uint32_t)(j - 1) << 16;
            if (found + 1 <= j - 1) {
                if (sp >= cap) { bad = MEA_BAD_STACK; break; }
                if (lane == 0) stack[sp] = w;
                sp++;
            }
            break;
        }
    }
    wave_sync();
    char *row = db + q.db_off;
    int16_t *gpt = pts + q.pt_off;
    for (int x = lane; x < L; x += 64) {
        const int p = bad ? -1 : pt[x];
        gpt[x] = (int16_t)p;
        row[x] = p < 0 ? '.' : p > x ? '(' : ')';
    }
    if (lane == 0) {
        row[L] = 0;
        aux[q.aux_off + 2 * (size_t)L] = dv;
        rec[s] = MeaRec{bad, bad ? 0 : npairs, tb.e(0, L - 1), dv};
    }
}
