// rafft_kinfold.hip - stochastic folding trajectories (gfx950): continuous-time Monte Carlo (Gillespie) over insertion and deletion
// of single pairs with Metropolis rates, what ViennaRNA's Kinfold simulates, defined exactly in DESIGN.md section 16 and
// include/rafft_hip.h.  The neighbours and their dE are those of rafft_moves.h, but this kernel keeps ITS OWN COPY of moves_at's
// body (enclosing pair, next partner, phase machine) and of the start energy: built on moves_at it kept its 108-110 VGPRs but went
// from 29 to 43 spilled SGPRs - in three shapes of the visitor alike - and its calls took 3.4 % longer on the MI355X
// (profiles/move_set_refactor_ab.txt).  A change to the move set in rafft_moves.h must be made here as well; the bit-for-bit
// comparisons of tests/test_gpu_kinfold.py with the mirror would show a disagreement.  Included by rafft_kernels.hip, after
// rafft_descend.hip.
//
// One WAVEFRONT per trajectory, one launch per chunk, the whole trajectory inside it, for the reasons rafft_descend.hip gives: a
// call brings thousands of trajectories over tens to hundreds of positions, each a long chain of short steps.  A trajectory holds
// 2 L bytes of pair table and 8 L bytes of weight subtotals in LDS (40 KiB at the longest).
//
// A step is descend's enumeration with a sum where descend takes a minimum, in two passes through ONE call site of loop_energy.
//   pass 0  lane l takes the positions x = l, l + 64, ...: the weights of x's candidates (the removal of its pair, or the additions
//           with x as 5' end) add up to wx[x] in LDS.  Weights are integers (the host's table, section 16), so the sum over the
//           wave, Wtot, does not depend on the order of the lanes.
//   between the Philox block of (trajectory, step) gives the waiting time and the number r < Wtot; a scan of wx in blocks of 64
//           positions (every lane reads what it wrote itself) finds the first x whose inclusive cumulative weight exceeds r.
//   pass 1  the lane that owns that x enumerates its candidates again, in ascending j, up to the one that passes the residue.
// Lane 0 applies the move to the table.  Lane w < n_watch keeps the distance of the state to watched row w - the number of pairs
// one has and the other has not - in a register: formed once from the two tables, then one read of watch_w[i] per move.  Distance 0
// is identity.
#pragma once

#include "rafft_batch_layout.h"     // KfTraj, KfRec, KfSample, the kinfold_* sizes
#include "rafft_rng.h"

// (a template for the sake of where its code lies, as descend_kernel is: emitted where it is first used, in kinfold_batch, the
//  last driver of the translation unit, so every older kernel keeps its place in the code object)
template <int KF_EMIT_LAST>
__global__ __launch_bounds__(64) void kinfold_kernel(const EnergyTables *ET, const KfTraj *ws, const uint8_t *codes, unsigned char *d_io,
                                                     unsigned char *d_log, const int16_t *d_watch, const unsigned long long *wtab,
                                                     const double *times, int n_times, double t_max, KfSample *d_smp, KfRec *rec)
{
    extern __shared__ __align__(16) unsigned char kf_lds[];
    const int lane = threadIdx.x;
    const KfTraj q = ws[blockIdx.x];
    const int L = q.L;
    const uint8_t *S = codes + q.code_off;
    int16_t *pt = (int16_t *)kf_lds;
    unsigned long long *wx = (unsigned long long *)(kf_lds + kinfold_pt_bytes(L));
    unsigned char *io = d_io + q.io_off;
    int *mv = q.log_off == KINFOLD_NO_LOG ? nullptr : (int *)(d_log + q.log_off);
    double *jt = q.log_off == KINFOLD_NO_LOG ? nullptr : (double *)(d_log + q.log_off + 8ull * (unsigned long long)q.bound);
    KfSample *smp = d_smp + (size_t)blockIdx.x * (size_t)n_times;
    const int16_t *wrow = d_watch + q.wt_off + (size_t)lane * (size_t)L;
    const bool watching = lane < q.n_watch;
    const unsigned long long stop_mask = q.n_stop >= 64 ? ~0ull : (1ull << q.n_stop) - 1ull;

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

    // the distance of the start row to this lane's watched row (a lane without one never reaches 0)
    int dist = 0x40000000;
    if (watching) {
        dist = 0;
        for (int x = 0; x < L; x++) {
            const int y = pt[x], z = wrow[x];
            dist += (y > x && z != y) + (z > x && z != y);
        }
    }

    int steps = 0, flags = 0, stop = -1, ti = 0;
    double time = 0.0;
    {
        const unsigned long long at = __ballot(dist == 0) & stop_mask;
        if (at) { flags = KF_STOP; stop = __ffsll((long long)at) - 1; }
    }
#pragma unroll 1
    while (!flags) {
        unsigned long long tot = 0, resid = 0;
        int xs = -1, mj = -1, mdE = 0;
        double T = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {
#pragma unroll 1
            for (int x = pass ? (lane == (xs & 63) ? xs : L) : lane; x < L; x += pass ? L : 64) {
                const int y = pt[x];
                if (y >= 0 && y < x) { if (!pass) wx[x] = 0; continue; }
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
                unsigned long long acc = 0;
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
                        acc += dE <= 0 ? KINFOLD_W0 : dE < RAFFT_KINFOLD_NW ? wtab[dE] : 0ull;
                        if (pass && acc > resid) { mj = j; mdE = dE; break; }
                        if (rem) break;
                        need = true;
                        phase = 1;
                    }
                }
                if (!pass) { wx[x] = acc; tot += acc; }
            }
            if (pass) break;

            // between the passes: the sum of the weights, the waiting time, the ends, the samples, the position of the move
            for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
            if (tot == 0) { flags = KF_ABSORBED; break; }
            uint32_t w[4];
            philox4x32_10((uint32_t)q.seed, (uint32_t)(q.seed >> 32), q.k, (uint32_t)steps, 0u, 0u, w);
            const double u = (double)(((uint64_t)w[0] << 32 | w[1]) >> 11) * 0x1.0p-53;
            const unsigned long long v = (unsigned long long)w[2] << 32 | w[3];
            T = time + -log(1.0 - u) * 4294967296.0 / (double)tot;
            if (T > t_max) { flags = KF_TIME; break; }
            // the state holds until T: the sample times before it see it
            if (ti < n_times && times[ti] < T) {
                const unsigned long long same = __ballot(dist == 0);
                const int widx = same ? __ffsll((long long)same) - 1 : -1;
                for (; ti < n_times && times[ti] < T; ti++) if (lane == 0) smp[ti] = KfSample{e, widx};
            }
            if (steps == q.bound) { flags = KF_MORE; break; }
            const unsigned long long r = __umul64hi(v, tot);
            unsigned long long run = 0;
            for (int base = 0; base < L && xs < 0; base += 64) {
                const unsigned long long own = base + lane < L ? wx[base + lane] : 0ull;
                unsigned long long c = own;
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned long long below = __shfl_up(c, o, 64);
                    if (lane >= o) c += below;
                }
                c += run;
                const unsigned long long hit = __ballot(c > r);
                if (hit) {
                    const int l = __ffsll((long long)hit) - 1;
                    xs = base + l;
                    resid = r - (__shfl(c, l, 64) - __shfl(own, l, 64));
                }
                run = __shfl(c, 63, 64);
            }
            if (xs < 0) { flags = KF_STUCK; break; }
        }
        if (flags) break;
        mj = __shfl(mj, xs & 63, 64);
        mdE = __shfl(mdE, xs & 63, 64);
        if (mj < 0) { flags = KF_STUCK; break; }
        const int i = xs, j = mj;
        const bool rem = (int)pt[i] == j;
        if (watching) dist += ((int)wrow[i] == j) != rem ? -1 : 1;      // (an added pair the row has, a removed one it has not: closer)
        __syncthreads();                // (every lane has read the table this step)
        if (lane == 0) {
            pt[i] = (int16_t)(rem ? -1 : j);
            pt[j] = (int16_t)(rem ? -1 : i);
            if (mv) { mv[2 * steps] = rem ? -i - 1 : i; mv[2 * steps + 1] = rem ? -j - 1 : j; jt[steps] = T; }
        }
        e += mdE;
        time = T;
        steps++;
        __syncthreads();
        const unsigned long long at = __ballot(dist == 0) & stop_mask;
        if (at) { flags = KF_STOP; stop = __ffsll((long long)at) - 1; }
    }

    // the sample times that are left: the state the trajectory ended in, or - the step bound ended it - nothing
    if (ti < n_times) {
        const unsigned long long same = __ballot(dist == 0);
        const int widx = same ? __ffsll((long long)same) - 1 : -1;
        if (lane == 0)
            for (; ti < n_times; ti++) smp[ti] = (flags & KF_MORE) ? KfSample{INT32_MIN, -2} : KfSample{e, widx};
    }
    // the end row over the bytes the pair table came in, and the record
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    for (int x = lane; x < L; x += 64) { const int y = pt[x]; io[x] = y < 0 ? '.' : y > x ? '(' : ')'; }
    if (lane == 0) {
        io[L] = 0;
        rec[blockIdx.x] = KfRec{flags | ((bad & 1) ? KF_BAD_PAIR : 0), steps, start, e, stop, 0, (flags & (KF_TIME | KF_ABSORBED)) ? t_max : time};
    }
}
