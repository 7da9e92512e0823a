// rafft_descend.hip - gradient walks to local minima (gfx950): from every start row the steepest descent over the single-pair move
// set, defined exactly in DESIGN.md section 14 and include/rafft_hip.h.  The neighbours of a row and their dE are rafft_moves.h's
// (moves_at); nothing of the enumeration is stated here.  Included by rafft_kernels.hip, after rafft_findpath.hip.
//
// One WAVEFRONT per walk, one launch per chunk of walks, the whole walk inside it.  Why a wavefront and not a workgroup: the calls
// this is for bring thousands to millions of walks over some tens to hundreds of positions, so the device is filled by walks, not by
// the lanes of one; a step is a handful of candidates per lane and one minimum over the team, which 64 lanes form with six
// cross-lane exchanges and no barrier between waves, where a workgroup would wait at an LDS barrier twice a step for a step that
// short; and a walk holds 2 L bytes of LDS (8 KiB at the longest), so a CU keeps as many walks resident as it has wave slots.  The
// price is the single long walk, which has 64 lanes however long it is (section 14: what it costs).
//
// A step.  Lane l takes the positions x = l, l + 64, ...; their candidates below 0 compete with the key
// (dE + 2^31) << 32 | i << 16 | j; the minimum over the wave is the step, which lane 0 applies to the table in LDS.  No candidate
// below 0: the row is a local minimum.
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

    int bad = 0;
    int e = structure_energy(ET, S, L, pt, lane, &bad);
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    const int start = e;

    int steps = 0, flags = 0;
#pragma unroll 1
    for (;;) {
        unsigned long long best = DS_NO_KEY;
#pragma unroll 1
        for (int x = lane; x < L; x += 64)
            moves_at(ET, S, L, pt, x, &bad, [&](int j, int dE) {
                if (dE < 0) {
                    const unsigned long long key = ((unsigned long long)((unsigned)dE + 0x80000000u) << 32) | ((unsigned long long)x << 16) | (unsigned long long)j;
                    best = key < best ? key : best;
                }
                return false;
            });
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        if (best == DS_NO_KEY) break;
        if (steps == q.bound) { flags |= DS_MORE; break; }
        const int i = (int)((best >> 16) & 0xffffull), j = (int)(best & 0xffffull);
        const bool rem = (int)pt[i] == j;
        __syncthreads();                // (every lane has read the table this step)
        if (lane == 0) apply_move(pt, i, j, rem, mv, steps);
        e += (int)((unsigned)(best >> 32) - 0x80000000u);
        steps++;
        __syncthreads();
    }

    // the end row over the bytes the pair table came in, and the record
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    write_row(io, pt, L, lane);
    if (lane == 0) rec[blockIdx.x] = DsRec{flags | ((bad & 1) ? DS_BAD_PAIR : 0), steps, start, e};
}
