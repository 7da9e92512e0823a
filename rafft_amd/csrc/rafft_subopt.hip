// rafft_subopt.hip - every structure of a sequence within an energy band above its minimum (gfx950): the enumeration of Wuchty et
// al. 1999 over the unambiguous decomposition rafft_pf.hip / rafft_sample.hip use, with the integer tables C, M, M1 and F of
// rafft_mfe.hip as lower bounds.  Every loop term comes from the device functions those kernels use (e_hairpin, e_intloop over the
// mfe_il table, mfe_ml_close, mfe_stem_ml, mfe_stem_ext): the energy model is not stated again.  DESIGN.md section 12.  Included by
// rafft_api.hip, after rafft_sample.hip.
//
// A STATE is a partial structure: the row so far, e_fixed (the loop terms decided), a LIFO stack of pending segments (words
// i | j << 12 | kind << 24, as rafft_sample.hip) and e_pending (the sum of the table minima of the pending segments).  A STEP pops
// the top segment, forms its candidates and keeps those with e_fixed + e_cand + e_pending' <= mfe + delta.  Candidates, in order:
//   F(0..j):  j unpaired -> F(0..j-1); stems (i,j), i ascending -> F(0..i-1), C(i,j)
//   C(i,j):   hairpin; interior loops in the order of mfe_il -> C(p,q); multiloop splits, k ascending -> M(i+1,k-1), M1(k,j-1)
//   M1(i,j):  j unpaired -> M1(i,j-1); the stem -> C(i,j)
//   M(i,j):   k ascending from i, for each k "unpaired alone before k" -> M1(k,j), then M(i,k-1), M1(k,j) (one lane holds both)
// Of one candidate the segment named last is pushed last and so expanded first.  An exterior segment of fewer than five positions
// holds nothing to choose and is not pushed.  The bound of a kept state is attained, so it completes to at least one structure of
// the band, and different states have disjoint completions: the frontier never holds more states than the answer has rows.
//
// A LEVEL of a chunk is three launches in stream order (no other synchronisation): subopt_level_kernel<false> counts the kept
// candidates of every state (one wavefront per state, rounds of 64 candidates, ballot and popcount; a finished state counts 1),
// subopt_scan_kernel turns the counts of a sequence into offsets and decides whether the sequence is finished, over its capacity
// or goes on, subopt_level_kernel<true> forms the candidates again and writes child r of a state to offset + r of the other
// buffer, all 64 lanes storing consecutive words; finished states are copied through at their offset.  After the last level the
// states of a sequence are its structures in the left-to-right order of the leaves of the decision tree.
#pragma once

#include "rafft_batch_layout.h"     // SuboptSeq, SuboptRec, subopt_state_bytes, seg_stack_words, subopt_pack_dcal_off

#define SUBOPT_NT 256               // four wavefronts: four states per workgroup and round
#define SUBOPT_SCAN_NT 1024
#define SUBOPT_SCAN_ITEMS 4
#define SUBOPT_NONE 0xffffffffu
enum { SUBOPT_K_F = 3 };            // beside MFE_K_C, MFE_K_M, MFE_K_M1: the exterior loop of 0..j
enum { SUBOPT_ACTIVE = 0, SUBOPT_DONE = 1, SUBOPT_OVER = 2, SUBOPT_BROKEN = 3 };
enum { SUBOPT_BAD_STACK = 1, SUBOPT_BAD_CELL = 2 };

struct SuboptCand { int e, pend; uint32_t w1, w2; };     // loop terms fixed; table minima of what is pushed; the pushes, in order
struct SuboptCtx {
    MfeTabHbm tb;
    const SmallT *T;
    const BigT *B;
    const uint8_t *S;
    const int *F;                   // F[x]: exterior energy of 0..x-1
    int L;
};

__device__ __forceinline__ uint32_t subopt_word(int i, int j, int kind) { return (uint32_t)i | (uint32_t)j << 12 | (uint32_t)kind << 24; }
__device__ __forceinline__ uint32_t subopt_f_word(int j) { return j >= 4 ? subopt_word(0, j, SUBOPT_K_F) : SUBOPT_NONE; }

__device__ __forceinline__ int subopt_min(const SuboptCtx &x, int kind, int i, int j)
{
    return kind == SUBOPT_K_F ? x.F[j + 1] : kind == MFE_K_C ? x.tb.c(i, j) : kind == MFE_K_M ? x.tb.m(i, j) : x.tb.m1(i, j);
}
__device__ __forceinline__ int subopt_n_cand(int kind, int i, int j)
{
    return kind == SUBOPT_K_F ? j - 2 : kind == MFE_K_C ? 1 + MFE_NIL + max(0, j - i - 10) : kind == MFE_K_M ? j - 3 - i : 2;
}

// candidates (c, 0) and (c, 1) of the segment (i, j, kind); t: the type of (i,j) for a C.  Bit 0 / 1 of the result: a / b exists
__device__ __forceinline__ int subopt_cands(const SuboptCtx &x, int kind, int i, int j, int t, int c, SuboptCand &a, SuboptCand &b)
{
    a = b = SuboptCand{0, 0, SUBOPT_NONE, SUBOPT_NONE};
    if (kind == SUBOPT_K_F) {
        if (c == 0) { a.pend = x.F[j]; a.w1 = subopt_f_word(j - 1); return 1; }
        const int p = c - 1;
        const int cc = x.tb.c(p, j);
        if (cc >= MFE_INFH) return 0;
        a.e = mfe_stem_ext(x.T, x.S, x.L, p, j);
        a.pend = x.F[p] + cc;
        a.w1 = subopt_f_word(p - 1); a.w2 = subopt_word(p, j, MFE_K_C);
        return 1;
    }
    if (kind == MFE_K_C) {
        if (c == 0) { a.e = e_hairpin(x.T, x.B, j - i - 1, t, x.S, i, j); return 1; }
        if (c <= MFE_NIL) {
            const int n12 = mfe_il.v[c - 1], n1 = n12 >> 8, n2 = n12 & 255, p = i + 1 + n1, q = j - 1 - n2;
            if (q - p < 4) return 0;
            const int t2 = pair_type(x.S[p], x.S[q]);
            if (!t2) return 0;
            const int cc = x.tb.c(p, q);
            if (cc >= MFE_INFH) return 0;
            int g = 0;
            a.e = e_intloop(x.T, x.B, n1, n2, t, rtype(t2), x.S[i + 1], x.S[j - 1], x.S[p - 1], x.S[q + 1], g);
            a.pend = cc;
            a.w1 = subopt_word(p, q, MFE_K_C);
            return 1;
        }
        const int k = i + 6 + (c - MFE_NIL - 1);
        const int m = x.tb.m(i + 1, k - 1), m1 = x.tb.m1(k, j - 1);
        if (m >= MFE_INFH || m1 >= MFE_INFH) return 0;
        a.e = mfe_ml_close(x.T, x.S, i, j, t);
        a.pend = m + m1;
        a.w1 = subopt_word(i + 1, k - 1, MFE_K_M); a.w2 = subopt_word(k, j - 1, MFE_K_M1);
        return 1;
    }
    if (kind == MFE_K_M1) {
        if (c == 0) {
            if (j <= i) return 0;
            const int prev = x.tb.m1(i, j - 1);
            if (prev >= MFE_INFH) return 0;
            a.e = x.T->ml_base; a.pend = prev; a.w1 = subopt_word(i, j - 1, MFE_K_M1);
            return 1;
        }
        const int cc = x.tb.c(i, j);
        if (cc >= MFE_INFH) return 0;
        a.e = mfe_stem_ml(x.T, x.S, x.L, i, j); a.pend = cc; a.w1 = subopt_word(i, j, MFE_K_C);
        return 1;
    }
    const int k = i + c;
    const int m1 = x.tb.m1(k, j);
    if (m1 >= MFE_INFH) return 0;
    a.e = (k - i) * x.T->ml_base; a.pend = m1; a.w1 = subopt_word(k, j, MFE_K_M1);
    if (k - 1 - i < 4) return 1;
    const int m = x.tb.m(i, k - 1);
    if (m >= MFE_INFH) return 1;
    b.pend = m + m1; b.w1 = subopt_word(i, k - 1, MFE_K_M); b.w2 = a.w1;
    return 3;
}

// One wavefront per sequence of the chunk: the exterior energies F (as mfe_traceback forms them) to device memory, the sequence's
// record and its first state - the open chain with the whole exterior loop pending - into buffer 0.
__global__ __launch_bounds__(64) void subopt_init_kernel(const EnergyTables *ET, const SuboptSeq *seqs, const int *order, const uint8_t *codes, int *tabs,
                                                        int *Fg, unsigned char *front, SuboptRec *rec)
{
    __shared__ int F[RAFFT_MFE_MAX_LEN + 1];
    const int s = order[blockIdx.x], lane = (int)threadIdx.x;
    const SuboptSeq q = seqs[s];
    const int L = q.L;
    int *t0 = tabs + q.tab_off;
    const size_t LL = (size_t)L * L;
    const MfeTabHbm tb{t0, t0 + LL, t0 + 2 * LL, L};
    const SmallT *T = &ET->s;
    const uint8_t *S = codes + q.code_off;
    if (lane == 0) F[0] = 0;
    wave_sync();
    for (int j = 0; j < L; j++) {
        int best = MFE_INF;
        for (int i = lane; i <= j - 4; i += 64) {
            const int c = tb.c(i, j);
            if (c < MFE_INFH) best = min(best, F[i] + c + mfe_stem_ext(T, S, L, i, j));
        }
        best = mfe_wave_min(best);
        const int prev = F[j];
        if (lane == 0) F[j + 1] = min(prev, best);
        wave_sync();
    }
    for (int x = lane; x <= L; x += 64) Fg[q.f_off + x] = F[x];
    const int words = subopt_state_bytes(L) / 4, rw0 = 4 + seg_stack_words(L);
    uint32_t *st = (uint32_t *)(front + q.buf_off[0]);
    const uint32_t first = subopt_f_word(L - 1);
    for (int x = lane; x < words; x += 64) {
        uint32_t v = 0;
        if (x == 1) v = first != SUBOPT_NONE ? (uint32_t)F[L] : 0u;
        if (x == 2) v = first != SUBOPT_NONE;
        if (x == 4 && first != SUBOPT_NONE) v = first;
        if (x >= rw0) {
            for (int b = 0; b < 4; b++) {
                const int pos = (x - rw0) * 4 + b;
                if (pos < L) v |= (uint32_t)'.' << (8 * b);
            }
        }
        st[x] = v;
    }
    if (lane == 0) {
        SuboptRec r;
        r.n[0] = 1; r.n[1] = 0; r.state = SUBOPT_ACTIVE; r.bad = 0; r.final_buf = 0; r.levels = 0; r.mfe = F[L]; r.pad = 0; r.n_reached = 0;
        rec[s] = r;
    }
}

// EMIT = false: the number of kept candidates of every state of buffer `src` into cnt (-1: the state is finished).
// EMIT = true: cnt holds the offsets; the children into the other buffer.
template <bool EMIT>
__global__ __launch_bounds__(SUBOPT_NT) void subopt_level_kernel(const EnergyTables *ET, const SuboptSeq *seqs, const int *order, const uint8_t *codes, int *tabs,
                                                                const int *Fg, unsigned char *front, int *cnt, SuboptRec *rec, int src, int delta)
{
    const int s = order[blockIdx.y], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SuboptRec *r = rec + s;
    if (r->state != SUBOPT_ACTIVE) return;
    const SuboptSeq q = seqs[s];
    const int L = q.L, n = r->n[src], limit = r->mfe + delta;
    int *t0 = tabs + q.tab_off;
    const size_t LL = (size_t)L * L;
    const SuboptCtx cx{MfeTabHbm{t0, t0 + LL, t0 + 2 * LL, L}, &ET->s, &ET->b, codes + q.code_off, Fg + q.f_off, L};
    const int words = subopt_state_bytes(L) / 4, rw0 = 4 + seg_stack_words(L), cap = RAFFT_SAMPLE_STACK(L);
    const uint32_t *in = (const uint32_t *)(front + q.buf_off[src]);
    uint32_t *out = (uint32_t *)(front + q.buf_off[src ^ 1]);
    int *cn = cnt + q.cnt_off;
    for (int k = blockIdx.x * (SUBOPT_NT / 64) + wave; k < n; k += gridDim.x * (SUBOPT_NT / 64)) {
        const uint32_t *st = in + (size_t)k * words;
        const int ef = __builtin_amdgcn_readfirstlane((int)st[0]), ep = __builtin_amdgcn_readfirstlane((int)st[1]);
        const int sp = __builtin_amdgcn_readfirstlane((int)st[2]);
        if (sp <= 0) {
            if (!EMIT) {
                if (lane == 0) cn[k] = -1;
            } else {
                uint32_t *d = out + (size_t)cn[k] * words;
                for (int x = lane; x < words; x += 64) d[x] = st[x];
            }
            continue;
        }
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)st[4 + sp - 1]);
        const int i = (int)(w & 4095u), j = (int)((w >> 12) & 4095u), kind = (int)(w >> 24);
        const int t = kind == MFE_K_C ? pair_type(cx.S[i], cx.S[j]) : 0;
        const int ep0 = ep - subopt_min(cx, kind, i, j), base = ef + ep0;
        const int nc = (kind == MFE_K_C && !t) ? 0 : subopt_n_cand(kind, i, j);
        int total = 0, over = 0;
        int at = EMIT ? cn[k] : 0;
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int c = c0 + lane;
            SuboptCand a, b;
            const int have = c < nc ? subopt_cands(cx, kind, i, j, t, c, a, b) : 0;
            const bool ka = (have & 1) && base + a.e + a.pend <= limit, kb = (have & 2) && base + b.e + b.pend <= limit;
            const unsigned long long bal_a = __ballot(ka), bal_b = __ballot(kb);
            if (!EMIT) {
                total += __popcll(bal_a) + __popcll(bal_b);
                const bool deep = (ka && sp - 1 + (a.w1 != SUBOPT_NONE) + (a.w2 != SUBOPT_NONE) > cap) || (kb && sp + 1 > cap);
                if (__ballot(deep)) over = 1;
                continue;
            }
            unsigned long long any = bal_a | bal_b;
            while (any) {
                const int l = __ffsll((long long)any) - 1;
                any &= any - 1;
                for (int h = 0; h < 2; h++) {
                    if (!(((h ? bal_b : bal_a) >> l) & 1)) continue;
                    const int ce = __shfl(h ? b.e : a.e, l, 64), cp = __shfl(h ? b.pend : a.pend, l, 64);
                    const uint32_t w1 = (uint32_t)__shfl((int)(h ? b.w1 : a.w1), l, 64), w2 = (uint32_t)__shfl((int)(h ? b.w2 : a.w2), l, 64);
                    // the pushes, without the ones that are none
                    const uint32_t p1 = w1 != SUBOPT_NONE ? w1 : w2, p2 = w1 != SUBOPT_NONE ? w2 : SUBOPT_NONE;
                    const int np = (p1 != SUBOPT_NONE) + (p2 != SUBOPT_NONE);
                    uint32_t *d = out + (size_t)at * words;
                    at++;
                    for (int x = lane; x < words; x += 64) {
                        uint32_t v = st[x];
                        if (x == 0) v = (uint32_t)(ef + ce);
                        else if (x == 1) v = (uint32_t)(ep0 + cp);
                        else if (x == 2) v = (uint32_t)(sp - 1 + np);
                        else if (x == 4 + sp - 1 && np >= 1) v = p1;
                        else if (x == 4 + sp && np >= 2) v = p2;
                        else if (kind == MFE_K_C && x >= rw0) {
                            if (x == rw0 + (i >> 2)) v = (v & ~(0xffu << (8 * (i & 3)))) | (uint32_t)'(' << (8 * (i & 3));
                            if (x == rw0 + (j >> 2)) v = (v & ~(0xffu << (8 * (j & 3)))) | (uint32_t)')' << (8 * (j & 3));
                        }
                        d[x] = v;
                    }
                }
            }
        }
        if (!EMIT && lane == 0) {
            cn[k] = total;
            if (!total) atomicMax(&r->bad, (int)SUBOPT_BAD_CELL);
            else if (over) atomicMax(&r->bad, (int)SUBOPT_BAD_STACK);
        }
    }
}

// One workgroup per sequence of the chunk: the counts of its states become their exclusive prefix sums (tiles of 4096 in ascending
// order under a 64-bit running total), and the sequence's record is settled - broken (a state without a candidate, a stack that
// would overflow), over max_structs (n_reached: the total that exceeded it), finished (no state has a pending segment), or the
// number of states of the next level.  *open counts the sequences of the chunk that go on.
__global__ __launch_bounds__(SUBOPT_SCAN_NT) void subopt_scan_kernel(const SuboptSeq *seqs, const int *order, int *cnt, SuboptRec *rec, int src, int max_structs,
                                                                     int *open)
{
    __shared__ long long wsum[SUBOPT_SCAN_NT / 64];
    __shared__ int n_unfinished;
    const int s = order[blockIdx.x], tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SuboptRec *r = rec + s;
    const int state0 = r->state, bad0 = r->bad, n = r->n[src];
    if (tid == 0) n_unfinished = 0;
    __syncthreads();
    if (state0 != SUBOPT_ACTIVE) return;
    if (bad0) {
        if (tid == 0) { r->state = SUBOPT_BROKEN; atomicSub(open, 1); }
        return;
    }
    int *cn = cnt + seqs[s].cnt_off;
    long long carry = 0;
    int unfinished = 0;
    for (int base = 0; base < n; base += SUBOPT_SCAN_NT * SUBOPT_SCAN_ITEMS) {
        const int x0 = base + tid * SUBOPT_SCAN_ITEMS;
        int v[SUBOPT_SCAN_ITEMS];
        long long local = 0;
        for (int u = 0; u < SUBOPT_SCAN_ITEMS; u++) {
            const int raw = x0 + u < n ? cn[x0 + u] : -2;
            unfinished += raw >= 0;
            v[u] = raw == -1 ? 1 : raw < 0 ? 0 : raw;
            local += v[u];
        }
        long long incl = local;
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = 0, tile = 0;
        for (int u = 0; u < SUBOPT_SCAN_NT / 64; u++) {
            if (u < wave) before += wsum[u];
            tile += wsum[u];
        }
        long long at = carry + before + incl - local;
        for (int u = 0; u < SUBOPT_SCAN_ITEMS; u++) {
            if (x0 + u < n) cn[x0 + u] = (int)(at < 0x7fffffffLL ? at : 0x7fffffffLL);
            at += v[u];
        }
        carry += tile;
        __syncthreads();
    }
    if (unfinished) atomicAdd(&n_unfinished, unfinished);
    __syncthreads();
    if (tid != 0) return;
    if (carry > (long long)max_structs) { r->state = SUBOPT_OVER; r->n_reached = carry; atomicSub(open, 1); }
    else if (n_unfinished == 0) { r->state = SUBOPT_DONE; r->final_buf = src; atomicSub(open, 1); }
    else { r->n[src ^ 1] = (int)carry; r->levels++; }
}

// The finished states of a sequence, packed for the copy to the host: rows (L + 1 bytes apart) from byte 0 of the buffer the last
// level did not write, the energies behind them (at the next multiple of 16).  One wavefront per state.
__global__ __launch_bounds__(SUBOPT_NT) void subopt_pack_kernel(const SuboptSeq *seqs, const int *order, unsigned char *front, const SuboptRec *rec)
{
    const int s = order[blockIdx.y], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SuboptRec r = rec[s];
    if (r.state != SUBOPT_DONE) return;
    const SuboptSeq q = seqs[s];
    const int L = q.L, n = r.final_buf ? r.n[1] : r.n[0], words = subopt_state_bytes(L) / 4, rw0 = 4 + seg_stack_words(L);
    const uint32_t *in = (const uint32_t *)(front + (r.final_buf ? q.buf_off[1] : q.buf_off[0]));
    unsigned char *rows = front + (r.final_buf ? q.buf_off[0] : q.buf_off[1]);
    int *dcal = (int *)(rows + subopt_pack_dcal_off(n, L));
    for (int k = blockIdx.x * (SUBOPT_NT / 64) + wave; k < n; k += gridDim.x * (SUBOPT_NT / 64)) {
        const uint32_t *st = in + (size_t)k * words;
        const unsigned char *row = (const unsigned char *)(st + rw0);
        unsigned char *d = rows + (size_t)k * (L + 1);
        for (int x = lane; x <= L; x += 64) d[x] = x < L ? row[x] : 0;
        if (lane == 0) dcal[k] = (int)st[0];
    }
}
