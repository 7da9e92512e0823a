// rafft_findpath.hip - folding barriers between pairs of structures (gfx950): the direct-path search of ViennaRNA's findpath (Flamm
// et al. 2001) for a batch of independent problems, defined exactly in DESIGN.md section 13 and include/rafft_hip.h.  Every loop
// term comes from loop_energy (rafft_device.h) through FpView, and the energy of a whole row is rafft_moves.h's structure_energy:
// the energy model is not stated again.  findpath_expand_kernel keeps ITS OWN COPY of the enclosing-pair walk: on enclosing_pair
// the compiler shaped that loop differently (same registers) and the calls took 0.8-1.1 % longer on the MI355X
// (profiles/move_set_refactor_ab.txt); a change to the walk in rafft_moves.h must be made there as well.  Included by
// rafft_kernels.hip, after rafft_io_kernels.hip (PlainView, select_smallest_inplace) and rafft_moves.h.
//
// A STATE of a problem is the set of applied moves (a mask of fp_mask_words(d) 64-bit words) with its energy and its saddle so far;
// the BEAM of a level holds up to W states in key order.  A LEVEL of a chunk is two launches in stream order (no other
// synchronisation; a workgroup whose problem has fewer levels, or has left the key's range, returns at once):
//   findpath_expand_kernel  one wavefront per (problem, state).  The state's pair table is rebuilt in LDS from A's table and the
//                           mask (removals, then additions).  A candidate (state s, move m) duplicates an earlier one exactly when a
//                           state s' < s of the beam has mask(s') \ mask(s) = {m} - both lead to the same set, and the lower rank
//                           sorts first since its saddle is no higher - so the wave compares its mask with those of the lower
//                           ranks word by word and marks such moves: no hash is involved.  Then the 64 lanes take the unapplied,
//                           unmarked, legal moves: the enclosing pair by a walk to the left, two or three loop energies, one key
//                           (biased saddle << 42 | biased energy << 20 | s d + m), appended to the problem's key list.
//   findpath_select_kernel  one workgroup per problem: the W smallest keys (radix select), sorted (bitonic, LDS); the next beam
//                           - mask of the parent with the move's bit, energy and saddle from the key - and per kept state one
//                           record (parent rank | move << 16, energy) of the level.
// findpath_init_kernel forms the energies of A and B as eval_kernel does and the first beam; findpath_trace_kernel follows the
// records of survivor 0 back and writes moves, energies, the saddle and its first step.
#pragma once

#include "../../include/rafft_hip.h" // RAFFT_FINDPATH_MAX_WIDTH
#include "rafft_batch_layout.h"     // FpProb, FpRec, the fp_* sizes, FINDPATH_*

// The four kernels are templates (of a number that means nothing) for the sake of where their code lies: a template's code is
// emitted where it is first used - in findpath_batch, the last driver of the translation unit - so every kernel that was in the
// library before keeps its place in the code object, the fold's among them, and with it the alignment of its hot loops.
// (512 threads, a size the beam step does not use: select_smallest_inplace<1024> and <256> stay the beam step's alone, inlined
//  into it as before)
#define FP_SEL_NT 512
#define FP_NO_KEY (~0ull)

__device__ __forceinline__ bool fp_in_range(int e) { return e > -FINDPATH_BIAS && e < FINDPATH_BIAS; }

template <int FP_EMIT_LAST>
__global__ __launch_bounds__(64) void findpath_init_kernel(const EnergyTables *ET, const FpProb *ps, const int *ord, const uint8_t *codes,
                                                           const unsigned char *d_in, unsigned char *d_ws, FpRec *rec)
{
    const int p = ord[blockIdx.x], lane = threadIdx.x;
    const FpProb q = ps[p];
    const int L = q.L;
    const uint8_t *S = codes + q.code_off;
    const int16_t *ptA = (const int16_t *)(d_in + q.in_off), *ptB = (const int16_t *)(d_in + q.in_off + fp_in_pt_bytes(L));
    // one call site of loop_energy for both structures
    int ea = 0, eb = 0, bad = 0;
#pragma unroll 1
    for (int which = 0; which < 2; which++) {
        const int e = structure_energy(ET, S, L, which ? ptB : ptA, lane, &bad);
        if (which) eb = e; else ea = e;
    }
    for (int o = 32; o > 0; o >>= 1) { ea += __shfl_xor(ea, o, 64); eb += __shfl_xor(eb, o, 64); bad |= __shfl_xor(bad, o, 64); }
    const int mw = fp_mask_words(q.d);
    unsigned long long *mask0 = (unsigned long long *)(d_ws + q.ws_off);
    for (int w = lane; w < mw; w += 64) mask0[w] = 0;
    if (lane == 0) {
        int2 *es = (int2 *)(d_ws + q.ws_off + fp_ws_es_off(q.d, q.W));
        es[0] = make_int2(ea, ea);
        const int flags = ((bad & 1) ? FP_BAD_PAIR : 0) | (fp_in_range(ea) && fp_in_range(eb) ? 0 : FP_RANGE);
        rec[p] = FpRec{1, 0, flags, ea, ea, eb, ea, 0};
    }
}

// dynamic LDS of the expand kernel for the longest problem of a chunk: the pair table, the state's mask, the marked moves
__host__ __device__ constexpr int fp_expand_lds_pt(int L) { return (2 * L + 15) & ~15; }
__host__ __device__ constexpr int fp_expand_lds_bytes(int L, int dmax) { return fp_expand_lds_pt(L) + 2 * 8 * fp_mask_words(dmax); }

template <int FP_EMIT_LAST>
__global__ __launch_bounds__(64) void findpath_expand_kernel(const EnergyTables *ET, const FpProb *ps, const int *ord, const uint8_t *codes,
                                                             const unsigned char *d_in, unsigned char *d_ws, FpRec *rec, int level, int lds_pt)
{
    extern __shared__ __align__(16) unsigned char fp_lds[];
    const int p = ord[blockIdx.y], lane = threadIdx.x, s = blockIdx.x;
    const FpProb q = ps[p];
    if (level >= q.d) return;
    const int n_cur = rec[p].n_cur;
    if (rec[p].flags || s >= n_cur) return;
    const int L = q.L, d = q.d, n_rem = q.n_rem, W = q.W, mw = fp_mask_words(d), cur = level & 1;
    int16_t *pt = (int16_t *)fp_lds;
    unsigned long long *msk = (unsigned long long *)(fp_lds + lds_pt);
    unsigned int *dup = (unsigned int *)(msk + mw);
    const uint8_t *S = codes + q.code_off;
    const unsigned char *in = d_in + q.in_off;
    const int16_t *ptA = (const int16_t *)in;
    const uint32_t *moves = (const uint32_t *)(in + fp_in_moves_off(L));
    const unsigned long long *conf = (const unsigned long long *)(in + fp_in_conf_off(L, d));
    unsigned char *ws = d_ws + q.ws_off;
    const unsigned long long *masks = (const unsigned long long *)(ws + (unsigned long long)cur * fp_ws_mask_bytes(d, W));
    const int2 es = ((const int2 *)(ws + fp_ws_es_off(d, W)))[cur * W + s];
    unsigned long long *keys = (unsigned long long *)(ws + fp_ws_keys_off(d, W));

    for (int x = lane; x < L; x += 64) pt[x] = ptA[x];
    for (int w = lane; w < mw; w += 64) { msk[w] = masks[(size_t)s * mw + w]; dup[2 * w] = 0; dup[2 * w + 1] = 0; }
    __syncthreads();
    for (int m = lane; m < n_rem; m += 64)
        if ((msk[m >> 6] >> (m & 63)) & 1ull) { const uint32_t u = moves[m]; pt[u & 0xffffu] = -1; pt[u >> 16] = -1; }
    __syncthreads();
    for (int m = n_rem + lane; m < d; m += 64)
        if ((msk[m >> 6] >> (m & 63)) & 1ull) { const uint32_t u = moves[m]; pt[u & 0xffffu] = (int16_t)(u >> 16); pt[u >> 16] = (int16_t)(u & 0xffffu); }
    // moves whose candidate a lower rank forms as well
    for (int s2 = lane; s2 < s; s2 += 64) {
        const unsigned long long *o = masks + (size_t)s2 * mw;
        int cnt = 0, bit = 0;
        for (int w = 0; w < mw && cnt < 2; w++) {
            const unsigned long long x = o[w] & ~msk[w];
            if (x) { cnt += __popcll(x); bit = w * 64 + (int)__builtin_ctzll(x); }
        }
        if (cnt == 1) atomicOr(&dup[bit >> 5], 1u << (bit & 31));
    }
    __syncthreads();

    for (int base = 0; base < d; base += 64) {
        const int m = base + lane;
        bool ok = m < d;
        if (ok) ok = !((msk[m >> 6] >> (m & 63)) & 1ull) && !((dup[m >> 5] >> (m & 31)) & 1u);
        if (ok && m >= n_rem) {
            const unsigned long long *c = conf + (size_t)(m - n_rem) * mw;
            for (int w = 0; w < mw && ok; w++) ok = (c[w] & ~msk[w]) == 0;
        }
        unsigned long long key = FP_NO_KEY;
        if (ok) {
            const uint32_t u = moves[m];
            const int i = (int)(u & 0xffffu), j = (int)(u >> 16);
            // the pair that encloses i (and j: nothing present crosses the move): leftwards, over whole helices
            int ci = -1, cj = L;
            for (int x = i - 1; x >= 0; x--) {
                const int y = pt[x];
                if (y < 0) continue;
                if (y < x) { x = y; continue; }
                ci = x; cj = y;
                break;
            }
            const bool rem = m < n_rem;
            // one call site of loop_energy: the enclosing loop as it is, the enclosing loop after the move, the loop of (i,j) itself
            // (before a removal, after an addition)
            int bad = 0, le[3];
#pragma unroll 1
            for (int k = 0; k < 3; k++) {
                const bool moved = k == 1 || (k == 2 && !rem);
                const FpView v{pt, moved ? i : -1, moved ? j : -1, rem ? -1 : j, rem ? -1 : i};
                const int e1 = loop_energy(&ET->s, &ET->b, S, L, v, k == 2 ? i : ci, k == 2 ? j : cj, &bad);
                le[k] = e1;
            }
            const int e_out0 = le[0], e_out1 = le[1], e_in = le[2];
            const int e = es.x + e_out1 - e_out0 + (rem ? -e_in : e_in);
            const int sad = e > es.y ? e : es.y;
            if (bad & 1) atomicOr(&rec[p].flags, FP_BAD_PAIR);
            if (!fp_in_range(e)) { atomicOr(&rec[p].flags, FP_RANGE); ok = false; }
            else key = ((unsigned long long)(unsigned)(sad + FINDPATH_BIAS) << (FINDPATH_KEY_BITS + FINDPATH_INDEX_BITS)) |
                       ((unsigned long long)(unsigned)(e + FINDPATH_BIAS) << FINDPATH_INDEX_BITS) | (unsigned long long)((unsigned)s * (unsigned)d + (unsigned)m);
        }
        const unsigned long long bal = __ballot(ok);
        const int tot = __popcll(bal);
        if (tot == 0) continue;
        const int pre = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        int at = 0;
        if (lane == 0) at = atomicAdd(&rec[p].n_keys, tot);
        at = __shfl(at, 0, 64);
        if (ok && at + pre < n_cur * d) keys[at + pre] = key;       // (n_cur d <= W d slots: every (state, move) has one)
    }
}

template <int FP_EMIT_LAST>
__global__ __launch_bounds__(FP_SEL_NT) void findpath_select_kernel(const FpProb *ps, const int *ord, unsigned char *d_ws, FpRec *rec, int level)
{
    __shared__ int hist[256], sh[32];
    __shared__ unsigned long long srt[RAFFT_FINDPATH_MAX_WIDTH];
    const int p = ord[blockIdx.x], tid = threadIdx.x;
    const FpProb q = ps[p];
    if (level >= q.d) return;
    const int flags = rec[p].flags, N = rec[p].n_keys;
    if (flags) return;
    __syncthreads();                    // (every thread has read the record that thread 0 writes below)
    if (N <= 0) { if (tid == 0) rec[p].flags = FP_STUCK; return; }
    const int d = q.d, W = q.W, mw = fp_mask_words(d), cur = level & 1;
    unsigned char *ws = d_ws + q.ws_off;
    unsigned long long *keys = (unsigned long long *)(ws + fp_ws_keys_off(d, W));
    const int K = N < W ? N : W;
    select_smallest_inplace<FP_SEL_NT>(keys, N, K, hist, sh);
    __syncthreads();
    int P2 = 1;
    while (P2 < K) P2 <<= 1;
    for (int t = tid; t < P2; t += FP_SEL_NT) srt[t] = t < K ? keys[t] : FP_NO_KEY;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P2; t += FP_SEL_NT) {
                const int o = t ^ j;
                if (o > t) {
                    const unsigned long long a = srt[t], b = srt[o];
                    const bool up = (t & k) == 0;
                    if ((a > b) == up) { srt[t] = b; srt[o] = a; }
                }
            }
            __syncthreads();
        }
    const unsigned long long *m_cur = (const unsigned long long *)(ws + (unsigned long long)cur * fp_ws_mask_bytes(d, W));
    unsigned long long *m_nxt = (unsigned long long *)(ws + (unsigned long long)(cur ^ 1) * fp_ws_mask_bytes(d, W));
    int2 *es_nxt = (int2 *)(ws + fp_ws_es_off(d, W)) + (cur ^ 1) * W;
    int2 *back = (int2 *)(ws + fp_ws_back_off(d, W)) + (size_t)level * W;
    const unsigned idx_mask = (1u << FINDPATH_INDEX_BITS) - 1u, f_mask = (1u << FINDPATH_KEY_BITS) - 1u;
    for (int x = tid; x < K * mw; x += FP_SEL_NT) {
        const int r = x / mw, w = x - r * mw;
        const unsigned ci = (unsigned)srt[r] & idx_mask;
        const int par = (int)(ci / (unsigned)d), m = (int)(ci - (unsigned)par * (unsigned)d);
        m_nxt[(size_t)r * mw + w] = m_cur[(size_t)par * mw + w] | ((m >> 6) == w ? 1ull << (m & 63) : 0ull);
    }
    for (int t = tid; t < K; t += FP_SEL_NT) {
        const unsigned long long key = srt[t];
        const unsigned ci = (unsigned)key & idx_mask;
        const int par = (int)(ci / (unsigned)d), m = (int)(ci - (unsigned)par * (unsigned)d);
        const int e = (int)((unsigned)(key >> FINDPATH_INDEX_BITS) & f_mask) - FINDPATH_BIAS;
        const int sad = (int)((unsigned)(key >> (FINDPATH_KEY_BITS + FINDPATH_INDEX_BITS)) & f_mask) - FINDPATH_BIAS;
        es_nxt[t] = make_int2(e, sad);
        back[t] = make_int2(par | (m << 16), e);
    }
    if (tid == 0) { rec[p].n_cur = K; rec[p].n_keys = 0; }
}

// one lane per problem: the records of survivor 0, level by level back to A
template <int FP_EMIT_LAST>
__global__ __launch_bounds__(64) void findpath_trace_kernel(int n, const FpProb *ps, const int *ord, const unsigned char *d_in, const unsigned char *d_ws,
                                                            unsigned char *d_out, FpRec *rec)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int p = ord[k];
    const FpProb q = ps[p];
    FpRec r = rec[p];
    if (r.flags) return;
    const int d = q.d, W = q.W;
    const uint32_t *moves = (const uint32_t *)(d_in + q.in_off + fp_in_moves_off(q.L));
    const int2 *back = (const int2 *)(d_ws + q.ws_off + fp_ws_back_off(d, W));
    int *om = (int *)(d_out + q.out_off), *oe = (int *)(d_out + q.out_off + fp_out_dcal_off(d));
    int rank = 0;
    for (int l = d; l >= 1; l--) {
        const int2 b = back[(size_t)(l - 1) * W + rank];
        const int m = b.x >> 16;
        const uint32_t u = moves[m];
        const int i = (int)(u & 0xffffu), j = (int)(u >> 16);
        om[2 * (l - 1)] = m < q.n_rem ? -i - 1 : i;
        om[2 * (l - 1) + 1] = m < q.n_rem ? -j - 1 : j;
        oe[l] = b.y;
        rank = b.x & 0xffff;
    }
    oe[0] = r.start;
    int sad = r.start, step = 0, e = r.start;
    for (int l = 1; l <= d; l++) {
        e = oe[l];
        if (e > sad) { sad = e; step = l; }
    }
    r.end = e; r.saddle = sad; r.saddle_step = step;
    rec[p] = r;
}
