// rafft_expand_common.h - what expand_kernel (both its one-wavefront and its wide-team branch) and expand_small_kernel must
// agree on bit for bit, written once: the value of a lag, the eligible prefix of a half-diagonal, the record of a kept candidate
// and the statistics lines.  The kernels keep what differs
// between team shapes and call these.  Everything here is inlined into its caller: the expand kernels have no registers to
// spare for a call.
#pragma once
#include "rafft_kernels.h"

// The record of a kept candidate, written to slot `slot` of the candidate arena: the stem, the hash of its pairs, where it cuts
// the region's branch list; both child slots empty.
__device__ __forceinline__ void emit_cand(const Dev &d, const uint32_t *brl, int nbr, const uint16_t *pos, int mi, int mj, int nb, int ddcal,
                                          unsigned long long slot)
{
    const int a0 = pos[mi], b0 = pos[mj], ao = pos[mi - nb + 1], bo = pos[mj + nb - 1];
    uint64_t h1 = 0, h2 = 0;
    if (a0 - ao == nb - 1 && bo - b0 == nb - 1) stem_hash(a0, b0, ao, bo, &h1, &h2);      // contiguous: the pair hashes telescope
    else
        for (int t = 0; t < nb; t++) {
            uint64_t a, b;
            pair_hash(pos[mi - t], pos[mj + t], &a, &b);
            h1 += a; h2 += b;
        }
    Cand cd;
    cd.ddcal = ddcal; cd.mi = (uint16_t)mi; cd.mj = (uint16_t)mj; cd.nb = (uint16_t)nb;
    { int c0, c1, c2, c3; br_lower4(brl, nbr, a0, b0, ao, bo, c0, c1, c2, c3); cd.set_cuts(c0, c1, c2, c3); }
    cd.h1 = h1; cd.h2 = h2;
    d.cand[slot] = cd;
    d.cslot[slot] = 0ULL;      // (both child slots: nobody has asked yet)
}

// The value of lag k of a region with 2n-1 = m lags, from its three exact pair counts (rafft/utils.py:125-132): the weighted pairs of
// the diagonal, both strands, over the length of the shorter arm + 1.  IEEE fp64, the same operations in the same order everywhere.
__device__ __forceinline__ double lag_value(double cAU, double cGC, double cGU, int k, int m, const Dev &d)
{
    const double raw = (2.0 * cAU) * d.au + (2.0 * cGC) * d.gc + (2.0 * cGU) * d.gu;
    const int nk = k < m - 1 - k ? k : m - 1 - k;
    return raw / ((double)nk + 1.0);
}

// Eligible cells of a half-diagonal (pos[jp] - pos[ip] > min_hp; cell i is (ip0 + i, jp0 - i), i < len2) form a prefix: its length.
// Positions are strictly increasing, so pos[jp] - pos[ip] >= jp - ip = len - 1 - 2 i: every cell with len - 1 - 2 i > min_hp is
// eligible without looking, and the search only covers the (min_hp + 3) / 2 cells that remain at the inner end of the half-diagonal
// (two steps for min_hp = 3 where the search over all of it took log2(len / 2) dependent pairs of LDS reads)
__device__ __forceinline__ int eligible_prefix(const uint16_t *pos, int len, int len2, int ip0, int jp0, int min_hp)
{
    const int csure = len - 1 - min_hp;
    int lo = csure > 0 ? min((csure + 1) >> 1, len2) : 0, hi = len2;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)pos[jp0 - mid] - (int)pos[ip0 + mid] > min_hp) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A team's share of the launch's statistics, added to its line: regions expanded, their positions, lags and branches ...
__device__ __forceinline__ void flush_stats(Counters::StatLine *sl, unsigned long long items, unsigned long long n, unsigned long long lags, unsigned long long nbr)
{
    atomicAdd(&sl->items, items);
    atomicAdd(&sl->n, n);
    atomicAdd(&sl->lags, lags);
    atomicAdd(&sl->nbr, nbr);
}
// ... and, with the built-in tables: stem energies evaluated / involving a rule or model value / kept ones that do.  (By reference:
// expand_kernel counts them in LDS and reads a count when it is needed, expand_small_kernel holds them in registers.)
template <class I>
__device__ __forceinline__ void flush_guess_stats(Counters::StatLine *sl, const I &evals, const I &guessed, const I &kept_guessed)
{
    atomicAdd(&sl->evals, (unsigned long long)(unsigned)evals);
    if (guessed) atomicAdd(&sl->guessed, (unsigned long long)(unsigned)guessed);
    if (kept_guessed) atomicAdd(&sl->kept_guessed, (unsigned long long)(unsigned)kept_guessed);
}
