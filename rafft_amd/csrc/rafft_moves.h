// rafft_moves.h - the single-pair move set (ViennaRNA's default: insertion and deletion of one pair, lonely pairs allowed), stated
// once for the kernels that stand on it: findpath_*_kernel, descend_kernel, barriers_scan_kernel, kinfold_kernel.  Everything here
// is force-inlined, so the header emits no code of its own.  DESIGN.md section 14, "The move set is stated once".
//
// The neighbours of a structure, by position x of its pair table pt (pt[x]: the partner, -1 unpaired):
//   x is a 5' end    one neighbour: its pair (x, pt[x]) removed
//   x is unpaired    one neighbour per j > x that is unpaired, lies in the same loop as x, has j - x > 3 and bases that pair
//                    (pair_type: N pairs with nothing): the pair (x, j) added
//   x is a 3' end    nothing (its pair belongs to its 5' end)
// so every neighbour is met exactly once, at its 5' end.  The positions of x's loop to the right of x are reached by a walk over
// unpaired positions and whole helices (next_partner); it ends at the 3' end of the pair that encloses x, which the walk to the
// left over whole helices finds (enclosing_pair) and which the walk to the right meets by itself as the first 3' end it sees.
// The positions x = lane, lane + 64, ... are the share of one lane of a wavefront.
//
// dE of a candidate (moves_at) is
//     loop(enclosing, after the move) - loop(enclosing, as it is) -/+ loop(the moved pair's own: before a removal, after an addition)
// from ONE call site of loop_energy (rafft_device.h), driven by a small phase counter: the energy model is not stated again, and
// the enclosing loop as it is is evaluated once per x, not per (x, j).  The loops are read through FpView, the pair table with one
// move applied.  The pure position logic (enclosing_pair, next_partner, apply_move) is host-callable and checked on the CPU
// against a brute-force enumeration (tests/hostcheck/moves_check.cpp); dE is device code and tested on the GPU only.
#pragma once

#include "rafft_device.h"

// the pair table `pt` with the partners of i and j replaced (i < 0: as it is)
struct FpView {
    const int16_t *pt;
    int i, j, vi, vj;
    __device__ __forceinline__ int operator()(int x) const { return x == i ? vi : x == j ? vj : (int)pt[x]; }
};

// the pair (ci, cj) that encloses x (ci = -1, cj = L: none, x lies in the exterior loop): leftwards, over whole helices
__device__ __host__ __forceinline__ void enclosing_pair(const int16_t *pt, int x, int L, int &ci, int &cj)
{
    ci = -1; cj = L;
    for (int p = x - 1; p >= 0; p--) {
        const int z = pt[p];
        if (z < 0) continue;
        if (z < p) { p = z; continue; }
        ci = p; cj = z;
        break;
    }
}

// The first position p of (j, end) that x may pair with - unpaired, p - x > 3, pair_type(S[x], S[p]) - on the walk from j to the
// right over unpaired positions and whole helices; `end` when there is none or a 3' end is met (the end of x's loop).  `end` is
// the 3' end of the enclosing pair or, for a caller that has not looked for it, L: the positions visited are the same.
__device__ __host__ __forceinline__ int next_partner(const int16_t *pt, const uint8_t *S, int x, int j, int end)
{
    int p = j + 1;
    while (p < end) {
        const int z = pt[p];
        if (z < 0) {
            if (p - x > 3 && pair_type(S[x], S[p])) break;
            p++;
        } else p = z > p ? z + 1 : end;
    }
    return p < end ? p : end;
}

// The candidates of position x: visit(j, dE) for the removal of x's pair (x, j), or for the additions (x, j) with x as 5' end in
// ascending j; it stops when visit returns true.  A 3' end yields nothing.
template <class Visit>
__device__ __forceinline__ void moves_at(const EnergyTables *ET, const uint8_t *S, int L, const int16_t *pt, int x, int *bad, Visit visit)
{
    const int y = pt[x];
    if (y >= 0 && y < x) return;
    const bool rem = y > x;
    int ci, cj;
    enclosing_pair(pt, x, L, ci, cj);
    int j = rem ? y : x, phase = 0, e0 = 0, e1 = 0;
    bool need = !rem;
#pragma unroll 1
    for (;;) {
        if (need) {
            j = next_partner(pt, S, x, j, cj);
            if (j >= cj) break;
            need = false;
        }
        // phase 0: the enclosing loop as it is; 1: after the move; 2: the loop of (x, j) itself
        const bool moved = phase == 1 || (phase == 2 && !rem);
        const FpView v{pt, moved ? x : -1, moved ? j : -1, rem ? -1 : j, rem ? -1 : x};
        const int le = loop_energy(&ET->s, &ET->b, S, L, v, phase == 2 ? x : ci, phase == 2 ? j : cj, bad);
        if (phase == 0) { e0 = le; phase = 1; }
        else if (phase == 1) { e1 = le; phase = 2; }
        else {
            if (visit(j, e1 - e0 + (rem ? -le : le)) || rem) break;
            need = true;
            phase = 1;
        }
    }
}

// One lane's share of the energy of a whole row: its loops i = lane, lane + 64, ... (index L: the exterior loop), as eval_kernel
// sums them.  The caller adds the lanes up.
__device__ __forceinline__ int structure_energy(const EnergyTables *ET, const uint8_t *S, int L, const int16_t *pt, int lane, int *bad)
{
    const FpView v{pt, -1, -1, -1, -1};
    int e = 0;
#pragma unroll 1
    for (int i = lane; i <= L; i += 64) {
        const int j = i < L ? (int)pt[i] : L;
        if (j > i || i == L) e += loop_energy(&ET->s, &ET->b, S, L, v, i < L ? i : -1, j, bad);
    }
    return e;
}

// The move (i, j) on the table - `rem`: the pair is there and goes, otherwise it comes - and, when the caller keeps them, in the
// list of moves as the library reports it: (i, j) for an added pair, (-i-1, -j-1) for a removed one.  One lane's work.
__device__ __host__ __forceinline__ void apply_move(int16_t *pt, int i, int j, bool rem, int *mv, int step)
{
    pt[i] = (int16_t)(rem ? -1 : j);
    pt[j] = (int16_t)(rem ? -1 : i);
    if (mv) { mv[2 * step] = rem ? -i - 1 : i; mv[2 * step + 1] = rem ? -j - 1 : j; }
}

// the row of the table as text and its NUL, over the bytes the table came in (io[0 .. L]); the whole wavefront
__device__ __forceinline__ void write_row(unsigned char *io, const int16_t *pt, int L, int lane)
{
    for (int x = lane; x < L; x += 64) { const int y = pt[x]; io[x] = y < 0 ? '.' : y > x ? '(' : ')'; }
    if (lane == 0) io[L] = 0;
}
