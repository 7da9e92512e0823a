// rafft_barriers.hip - exact barrier trees of energy bands (gfx950): the parallel part of rafft_barriers_batch, defined exactly in
// DESIGN.md section 15 and include/rafft_hip.h.  The landscape is a list of rows with their ranks; nothing here evaluates an
// energy.  Included by rafft_kernels.hip, after rafft_descend.hip.
//
// A row is known by the 128-bit commutative hash of its pair set (pair_hash, rafft_device.h), so the key of a neighbour - one pair
// removed or added - is the row's key -/+ pair_hash(i, j), and "is that neighbour in the list, and at which rank" is one look-up in
// an open-addressing table in HBM.  Five launches per chunk of whole sequences, stream order being the only synchronisation, so no
// kernel reads what the same launch writes:
//   barriers_keys_kernel    one wavefront per row: the key, summed over the lanes
//   barriers_insert_kernel  one thread per row: claims a slot (tag << 32 | rank) with one 64-bit compare-and-swap
//   barriers_scan_kernel<BAR_DOWN>   one wavefront per row, the pair table in LDS: down[x], the lowest-ranked neighbour
//   barriers_basin_kernel   one thread per row: the end of the chain of down
//   barriers_scan_kernel<BAR_EDGES>  the same enumeration: a neighbour of lower rank in another basin is an edge; the smallest
//                           rank per pair of basins is kept by an unsigned minimum, which is order-free - same bits every run
// The neighbours of a row are rafft_moves.h's, less what an energy needs (barriers_neighbours, on next_partner).  Every probe loop is bounded by its table's slot count: a full or corrupt table ends as a flag in BarRec, never as a spin.
#pragma once

#include "rafft_batch_layout.h"     // BarSeq, BarRec, the barriers_* sizes

#define BAR_DOWN 0
#define BAR_EDGES 1
#define BAR_NO_RANK 0xffffffffu

// the sequence of a chunk that holds row g of the chunk (qs in row order; nq >= 1)
__device__ __forceinline__ int barriers_seq_of(const BarSeq *qs, int nq, unsigned g)
{
    int lo = 0, hi = nq - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((unsigned)qs[mid].row0 <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned barriers_tag(uint64_t k1) { return (unsigned)(k1 >> 32); }

// The rank of the row with key (k1, k2) in the row table of q, BAR_NO_RANK when there is none.  `lowest`: go on to the free slot
// that ends the probe sequence and return the lowest rank among equal keys (how a duplicate row is told); otherwise the first.
__device__ __forceinline__ unsigned barriers_find(const BarSeq &q, const unsigned long long *tab, const uint64_t *keys, uint64_t k1, uint64_t k2,
                                                  bool lowest, unsigned *flags)
{
    const unsigned long long *t = tab + q.tab_off;
    const uint64_t *kk = keys + 2ull * (unsigned long long)q.row0;
    const unsigned tag = barriers_tag(k1);
    unsigned slot = (unsigned)k1 & q.tab_mask, found = BAR_NO_RANK;
    for (unsigned n = 0; n <= q.tab_mask; n++, slot = (slot + 1) & q.tab_mask) {
        const unsigned long long e = t[slot];
        if (e == BAR_EMPTY) return found;
        if ((unsigned)(e >> 32) != tag) continue;
        const unsigned r = (unsigned)e;
        if (r >= (unsigned)q.n_rows) { *flags |= BAR_TABLE_BAD; return found; }
        if (kk[2ull * r] == k1 && kk[2ull * r + 1] == k2) {
            if (!lowest) return r;
            found = r < found ? r : found;
        }
    }
    *flags |= BAR_TABLE_BAD;            // (no free slot in a table that is at most half full)
    return found;
}

// Every neighbour of the row whose pair table is pt (LDS) and whose key is (k1, k2): visit(rank) for those the table holds.
// Returns the number of them this lane found.
template <class Visit>
__device__ __forceinline__ unsigned barriers_neighbours(const BarSeq &q, const uint8_t *S, const int16_t *pt, int lane, const unsigned long long *tab,
                                                        const uint64_t *keys, uint64_t k1, uint64_t k2, unsigned *flags, Visit visit)
{
    const int L = q.L;
    unsigned hits = 0;
#pragma unroll 1
    for (int x = lane; x < L; x += 64) {
        const int y = pt[x];
        if (y >= 0 && y < x) continue;
        uint64_t h1, h2;
        if (y > x) {
            pair_hash(x, y, &h1, &h2);
            const unsigned r = barriers_find(q, tab, keys, k1 - h1, k2 - h2, false, flags);
            if (r != BAR_NO_RANK) { hits++; visit(r); }
            continue;
        }
        // x is unpaired: its partners to the right (end = L: the walk ends at the 3' end of the enclosing pair by itself)
#pragma unroll 1
        for (int p = x;;) {
            p = next_partner(pt, S, x, p, L);
            if (p >= L) break;
            pair_hash(x, p, &h1, &h2);
            const unsigned r = barriers_find(q, tab, keys, k1 + h1, k2 + h2, false, flags);
            if (r != BAR_NO_RANK) { hits++; visit(r); }
        }
    }
    return hits;
}

// (templates for the sake of where their code lies, as descend_kernel is: emitted where they are first used, in barriers_batch,
//  the last driver of the translation unit, so every older kernel keeps its place in the code object)
template <int BAR_EMIT_LAST>
__global__ __launch_bounds__(64) void barriers_keys_kernel(const BarSeq *qs, int nq, const unsigned char *d_pt, uint64_t *keys)
{
    const unsigned g = blockIdx.x;
    const BarSeq q = qs[barriers_seq_of(qs, nq, g)];
    const int lane = threadIdx.x;
    const int16_t *pt = (const int16_t *)(d_pt + q.pt_off + (unsigned long long)(g - (unsigned)q.row0) * (unsigned long long)q.pt_stride);
    uint64_t k1 = 0, k2 = 0;
    for (int x = lane; x < q.L; x += 64) {
        const int y = pt[x];
        if (y > x) {
            uint64_t h1, h2;
            pair_hash(x, y, &h1, &h2);
            k1 += h1; k2 += h2;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { k1 += __shfl_xor(k1, o, 64); k2 += __shfl_xor(k2, o, 64); }
    if (lane == 0) { keys[2ull * g] = k1; keys[2ull * g + 1] = k2; }
}

template <int BAR_EMIT_LAST>
__global__ __launch_bounds__(256) void barriers_insert_kernel(const BarSeq *qs, int nq, unsigned n_rows, const uint64_t *keys, unsigned long long *tab,
                                                              BarRec *rec)
{
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_rows) return;
    const int qi = barriers_seq_of(qs, nq, g);
    const BarSeq q = qs[qi];
    const uint64_t k1 = keys[2ull * g];
    const unsigned long long mine = ((unsigned long long)barriers_tag(k1) << 32) | (unsigned long long)(g - (unsigned)q.row0);
    unsigned long long *t = tab + q.tab_off;
    unsigned slot = (unsigned)k1 & q.tab_mask;
    for (unsigned n = 0; n <= q.tab_mask; n++, slot = (slot + 1) & q.tab_mask)
        if (atomicCAS(&t[slot], BAR_EMPTY, mine) == BAR_EMPTY) return;
    atomicOr(&rec[qi].flags, (unsigned)BAR_TABLE_BAD);
}

template <int MODE>
__global__ __launch_bounds__(64) void barriers_scan_kernel(const BarSeq *qs, int nq, const uint8_t *codes, const unsigned char *d_pt, const uint64_t *keys,
                                                           const unsigned long long *tab, int *down, const int *basin, unsigned long long *ekeys,
                                                           unsigned *evals, BarRec *rec)
{
    extern __shared__ __align__(16) unsigned char bar_lds[];
    const unsigned g = blockIdx.x;
    const int qi = barriers_seq_of(qs, nq, g);
    const BarSeq q = qs[qi];
    const int lane = threadIdx.x;
    const unsigned x = g - (unsigned)q.row0;
    const int16_t *src = (const int16_t *)(d_pt + q.pt_off + (unsigned long long)x * (unsigned long long)q.pt_stride);
    int16_t *pt = (int16_t *)bar_lds;
    for (int p = lane; p < q.L; p += 64) pt[p] = src[p];
    __syncthreads();
    const uint8_t *S = codes + q.code_off;
    const uint64_t k1 = keys[2ull * g], k2 = keys[2ull * g + 1];
    unsigned flags = 0;
    if (MODE == BAR_DOWN) {
        unsigned best = BAR_NO_RANK;
        unsigned hits = barriers_neighbours(q, S, pt, lane, tab, keys, k1, k2, &flags, [&](unsigned r) { best = r < best ? r : best; });
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
            hits += __shfl_xor(hits, o, 64);
            flags |= __shfl_xor(flags, o, 64);
        }
        if (lane == 0) {
            down[g] = (int)(best < x ? best : x);
            // a twin of this row at a lower rank: the lowest-ranked row that has one is reported, with its lowest twin
            const unsigned twin = barriers_find(q, tab, keys, k1, k2, true, &flags);
            if (twin < x) atomicMin(&rec[qi].dup, ((unsigned long long)x << 32) | (unsigned long long)twin);
            if (hits) atomicAdd(&rec[qi].hits, (unsigned long long)hits);
            if (flags) atomicOr(&rec[qi].flags, flags);
        }
    } else {
        const int *bs = basin + q.row0;
        const unsigned mine = (unsigned)bs[x];
        unsigned long long *ek = ekeys + q.edge_off;
        unsigned *ev = evals + q.edge_off;
        BarRec *rc = rec + qi;
        barriers_neighbours(q, S, pt, lane, tab, keys, k1, k2, &flags, [&](unsigned r) {
            if (r >= x) return;
            const unsigned other = (unsigned)bs[r];
            if (other == mine) return;
            const unsigned long long key = other < mine ? ((unsigned long long)other << 32) | mine : ((unsigned long long)mine << 32) | other;
            unsigned slot = (unsigned)mix64(key) & q.edge_mask;
            for (unsigned n = 0; n <= q.edge_mask; n++, slot = (slot + 1) & q.edge_mask) {
                const unsigned long long old = atomicCAS(&ek[slot], BAR_EMPTY, key);
                if (old == BAR_EMPTY && atomicAdd(&rc->claims, 1u) >= q.edge_cap) flags |= BAR_EDGES_FULL;
                if (old == BAR_EMPTY || old == key) { atomicMin(&ev[slot], x); return; }
            }
            flags |= BAR_EDGES_FULL;
        });
        if (flags) atomicOr(&rc->flags, flags);
    }
}

template <int BAR_EMIT_LAST>
__global__ __launch_bounds__(256) void barriers_basin_kernel(const BarSeq *qs, int nq, unsigned n_rows, const int *down, int *basin, BarRec *rec)
{
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_rows) return;
    const int qi = barriers_seq_of(qs, nq, g);
    const BarSeq q = qs[qi];
    const int *dn = down + q.row0;
    int x = (int)(g - (unsigned)q.row0);
    // down[x] <= x, so the chain ends; the bound holds against anything else
    for (int n = 0; n < q.n_rows; n++) {
        const int y = dn[x];
        if (y >= x || y < 0) { if (y != x) atomicOr(&rec[qi].flags, (unsigned)BAR_TABLE_BAD); break; }
        x = y;
    }
    basin[g] = x;
}
