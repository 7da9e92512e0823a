// rafft_descend.hip - gradient walks to local minima (gfx950): from every start row the steepest descent over ViennaRNA's default
// move set (insertion and deletion of one pair, lonely pairs allowed), defined exactly in DESIGN.md section 14 and
// include/rafft_hip.h.  Every loop term comes from loop_energy (rafft_device.h) through FpView (rafft_findpath.hip), the pair
// table with one move applied: the energy model is not stated again.  Included by rafft_kernels.hip, after rafft_findpath.hip.
//
// One WAVEFRONT per walk, one launch per chunk of walks, the whole walk inside it.  Why a wavefront and not a workgroup: the calls
// this is for bring thousands to millions of walks over some tens to hundreds of positions, so the device is filled by walks, not by
// the lanes of one; a step is a handful of candidates per lane and one minimum over the team, which 64 lanes form with six
// cross-lane exchanges and no barrier between waves, where a workgroup would wait at an LDS barrier twice a step for a step that
// short; and a walk holds 2 L bytes of LDS (8 KiB at the longest), so a CU keeps as many walks resident as it has wave slots.  The
// price is the single long walk, which has 64 lanes however long it is (section 14: what it costs).
//
// A step.  Lane l takes the positions x = l, l + 64, ...: a 5' end of a pair is that pair's removal, an unpaired position the 5' end
// of additions, a 3' end nothing.  The pair that encloses x is found by the walk to the left over whole helices (as in
// findpath_expand_kernel); an unpaired x then walks j to the right over unpaired positions and whole helices up to the enclosing
// pair's 3' end, which visits exactly the positions of its own loop.  dE of a candidate is
//     loop(enclosing, after the move) - loop(enclosing, as it is) -/+ loop(the moved pair's own: before a removal, after an addition)
// from ONE call site of loop_energy, driven by a small phase counter (the start row's energy, summed once as eval_kernel sums it, is
// the kernel's only other one); the enclosing loop as it is is evaluated once per x, not per (x, j).  The candidates below 0
// compete with the key (dE + 2^31) << 32 | i << 16 | j; the minimum over the wave is the step, which lane 0 applies to the table in
// LDS.  No candidate below 0: the row is a local minimum.
#pragma once

#include "rafft_batch_layout.h"     // DsWalk, DsRec, the descend_* sizes

#define DS_NO_KEY (~0ull)

// (a template for the sake of where its code lies, as the findpath kernels are: emitted where it is first used, in descend_batch,
//  the last driver of the translation unit, so every older kernel keeps its place in the code object)
template <int DS_EMIT_LAST>
__global__ __launch_bounds__(64) void descend_kernel(const EnergyTables *ET, const DsWalk *ws, const uint8_t *codes, unsigned char *d_io,
                                                     unsigned char *d_mv, DsRec *rec)
{
    extern __shared__ __align__(16) unsigned char ds_lds[];
    const int lane = threadIdx.x;
    const DsWalk q = ws[blockIdx.x];
    const int L = q.L;
    const uint8_t *S = codes + q.code_off;
    int16_t *pt = (int16_t *)ds_lds;
    unsigned char *io = d_io + q.io_off;
    int *mv = q.mv_off == DESCEND_NO_MOVES ? nullptr : (int *)(d_mv + q.mv_off);

    for (int x = lane; x < L; x += 64) pt[x] = ((const int16_t *)io)[x];
    __syncthreads();

    // the energy of the start row: all its loops (index L: the exterior loop), as eval_kernel sums them
    int e = 0, bad = 0;
    {
        const FpView v{pt, -1, -1, -1, -1};
#pragma unroll 1
        for (int i = lane; i <= L; i += 64) {
            const int j = i < L ? (int)pt[i] : L;
            if (j > i || i == L) e += loop_energy(&ET->s, &ET->b, S, L, v, i < L ? i : -1, j, &bad);
        }
    }
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    const int start = e;

    int steps = 0, flags = 0;
#pragma unroll 1
    for (;;) {
        unsigned long long best = DS_NO_KEY;
#pragma unroll 1
        for (int x = lane; x < L; x += 64) {
            const int y = pt[x];
            if (y >= 0 && y < x) continue;
            const bool rem = y > x;
            // the pair that encloses x: leftwards, over whole helices
            int ci = -1, cj = L;
            for (int p = x - 1; p >= 0; p--) {
                const int z = pt[p];
                if (z < 0) continue;
                if (z < p) { p = z; continue; }
                ci = p; cj = z;
                break;
            }
            int j = rem ? y : x, phase = 0, e0 = 0, e1 = 0;
            bool need = !rem;
#pragma unroll 1
            for (;;) {
                if (need) {
                    // the next position of x's loop to the right that x may pair with
                    int p = j + 1;
                    while (p < cj) {
                        const int z = pt[p];
                        if (z < 0) {
                            if (p - x > 3 && pair_type(S[x], S[p])) break;
                            p++;
                        } else p = z > p ? z + 1 : cj;
                    }
                    if (p >= cj) break;
                    j = p;
                    need = false;
                }
                // phase 0: the enclosing loop as it is; 1: after the move; 2: the loop of (x, j) itself
                const bool moved = phase == 1 || (phase == 2 && !rem);
                const FpView v{pt, moved ? x : -1, moved ? j : -1, rem ? -1 : j, rem ? -1 : x};
                const int le = loop_energy(&ET->s, &ET->b, S, L, v, phase == 2 ? x : ci, phase == 2 ? j : cj, &bad);
                if (phase == 0) { e0 = le; phase = 1; }
                else if (phase == 1) { e1 = le; phase = 2; }
                else {
                    const int dE = e1 - e0 + (rem ? -le : le);
                    if (dE < 0) {
                        const unsigned long long key = ((unsigned long long)((unsigned)dE + 0x80000000u) << 32) | ((unsigned long long)x << 16) | (unsigned long long)j;
                        best = key < best ? key : best;
                    }
                    if (rem) break;
                    need = true;
                    phase = 1;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        if (best == DS_NO_KEY) break;
        if (steps == q.bound) { flags |= DS_MORE; break; }
        const int i = (int)((best >> 16) & 0xffffull), j = (int)(best & 0xffffull);
        const bool rem = (int)pt[i] == j;
        __syncthreads();                // (every lane has read the table this step)
        if (lane == 0) {
            pt[i] = (int16_t)(rem ? -1 : j);
            pt[j] = (int16_t)(rem ? -1 : i);
            if (mv) { mv[2 * steps] = rem ? -i - 1 : i; mv[2 * steps + 1] = rem ? -j - 1 : j; }
        }
        e += (int)((unsigned)(best >> 32) - 0x80000000u);
        steps++;
        __syncthreads();
    }

    // the end row over the bytes the pair table came in, and the record
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    for (int x = lane; x < L; x += 64) { const int y = pt[x]; io[x] = y < 0 ? '.' : y > x ? '(' : ')'; }
    if (lane == 0) {
        io[L] = 0;
        rec[blockIdx.x] = DsRec{flags | ((bad & 1) ? DS_BAD_PAIR : 0), steps, start, e};
    }
}
