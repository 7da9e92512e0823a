// rafft_kernels.hip - the HIP kernels of the fold hot path (gfx950 / MI355X only): the helpers they share, then one file per kernel.
//
//   expand_kernel       (rafft_expand.hip) persistent workgroups (one wavefront for the common size class)
//                       fetch unpaired regions from a work list: correlation of the region
//                       with itself (rafft/utils.py:115-132; popcounts on bit masks for short
//                       regions, LDS-resident packed complex FFTs otherwise), selection of the
//                       nb_mode best lags (rafft/rafft.py:117-118,92), window_slide
//                       (rafft/rafft.py:36-83), local Turner dE of every candidate stem from
//                       prefix sums over the loop's branch list + filter/sort
//                       (rafft/rafft.py:86-109)
//                       Template switch PROD: production builds with the debug seam and - for
//                       the classes whose regions all take the popcount correlation - the FFT
//                       compiled out (no register spills).
//                       The body is the fetch loop and a list of phases (load_region ... emit_wave /
//                       emit_team, inlined); RegionA is the one view of its time-shared LDS region.
//   expand_small_kernel  (rafft_expand_small.hip) the same for regions of up to 16 / 32 positions:
//                       teams of 16 / 32 lanes, four or two regions per wavefront
//   beam_step_kernel    (rafft_beam.hip) one workgroup per sequence: helix combination in product order, flat
//                       over all parents of the beam, with `seen` dedupe and the max_branch
//                       rule, stable energy sort and beam cut (rafft/rafft.py:176-214)
//   materialize_team_kernel / materialize_kernel  (rafft_materialize.hip) a team of 16 / 64 lanes per new beam member:
//                       child regions (rafft/rafft.py:127-152, rafft/utils.py:141-152)
//   dedupe_kernel       (rafft_materialize.hip) identical loops reached through different structures share one
//                       expansion (no counterpart in the reference, which recomputes)
//   output_kernel       (rafft_io_kernels.hip, with stage_in_kernel and init_roots_kernel) gathers dot-bracket rows (rafft/utils.py:42-50)
//   eval_kernel         (rafft_io_kernels.hip) whole-structure energy (rafft/utils.py:135-138), C-ABI hook
//   findpath_*_kernel   (rafft_findpath.hip) folding barriers between structure pairs: not part of the fold, but built on
//                       loop_energy, PlainView's kin and the radix select below
//   descend_kernel      (rafft_descend.hip) gradient walks to local minima over the move set of rafft_moves.h
//   barriers_*_kernel   (rafft_barriers.hip) exact barrier trees of energy bands: keys, a hash table of the rows, neighbours looked up
//                       in it; no energy is evaluated
//   kinfold_kernel      (rafft_kinfold.hip) stochastic folding trajectories: the same move set (its own copy), summed weights, Philox
//
// This is bandwidth/latency-bound small-FFT + integer table work: no MFMA.
#include "rafft_kernels.h"

// ---------------------------------------------------------------- helpers

__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) // a * conj(b)
{
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// "this value is needed HERE": keeps the compiler from sinking a load below a branch that may not need it.  Loads issued back to
// back are one round trip; a load sunk to its first use, behind an early exit, is a dependent round trip of its own.
__device__ __forceinline__ void pin(unsigned int &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(int &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(unsigned long long &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(ulonglong2 &x) { asm volatile("" : "+v"(x.x), "+v"(x.y)); }
__device__ __forceinline__ void pin(uint4 &x) { asm volatile("" : "+v"(x.x), "+v"(x.y), "+v"(x.z), "+v"(x.w)); }

// exclusive prefix sum of one int per thread over the workgroup; returns total in *tot.
// `scratch` needs (NT/64 + 1) ints of LDS.
template <int NT>
__device__ inline int block_exscan(int v, int *scratch, int *tot)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = wave_incl_scan(v);           // (round 5: six DPP additions - every caller has the whole wavefront active - instead of six __shfl_up)
    if (NT == 64) {
        *tot = __builtin_amdgcn_readlane(x, 63);
        return x - v;
    }
    __syncthreads();
    if (lane == 63) scratch[wv] = x;
    __syncthreads();
    int base = 0, t = 0;
    for (int i = 0; i < NT / 64; i++) {
        int s = scratch[i];
        if (i < wv) base += s;
        t += s;
    }
    *tot = t;
    return base + x - v;
}

// The same for a 0/1 flag: a ballot and two bit counts instead of six shuffle steps per wavefront.
template <int NT>
__device__ inline int block_exscan_flag(int f, int *scratch, int *tot)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f != 0);
    const int pre = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));   // set bits below my lane
    const int wtot = __popcll(bal);
    (void)lane;
    if (NT == 64) {
        *tot = wtot;
        return pre;
    }
    __syncthreads();
    if (lane == 0) scratch[wv] = wtot;
    __syncthreads();
    int base = 0, t = 0;
    for (int i = 0; i < NT / 64; i++) {
        int s = scratch[i];
        if (i < wv) base += s;
        t += s;
    }
    *tot = t;
    return base + pre;
}

// Exact top-K selection for a workgroup: moves the K smallest of the N DISTINCT 64-bit keys in LDS to
// keys[0..K) (unordered).  Byte-wise radix select from the most significant byte: 8 passes over the
// keys with a 256-bin LDS histogram instead of sorting all N.  `hist` needs 256 ints, `sh` 32 ints.
template <int NT>
__device__ inline void select_smallest_inplace(unsigned long long *keys, int N, int K, int *hist, int *sh)
{
    const int tid = threadIdx.x;
    if (K >= N) return;
    // bytes in which no two keys differ need no pass (the keys of the beam step are (energy + bias) << 32 | generation order: of
    // their eight bytes three or four vary) - one OR-reduction of key ^ keys[0] finds them
    unsigned long long diff = 0;
    const unsigned long long key0 = keys[0];
    for (int i = tid; i < N; i += NT) diff |= keys[i] ^ key0;
    for (int o = 32; o > 0; o >>= 1) diff |= __shfl_xor(diff, o, 64);
    if (tid < 2) sh[26 + tid] = 0;
    __syncthreads();
    if ((tid & 63) == 0) { atomicOr((unsigned int *)&sh[26], (unsigned int)diff); atomicOr((unsigned int *)&sh[27], (unsigned int)(diff >> 32)); }
    __syncthreads();
    diff = ((unsigned long long)(unsigned int)sh[27] << 32) | (unsigned int)sh[26];
    unsigned long long prefix = 0;
    int kk = K;
    bool take_le = false;              // every key of the threshold bin is wanted: nothing below that byte needs looking at
    for (int pass = 7; pass >= 0 && !take_le; pass--) {
        if (((diff >> (8 * pass)) & 255ULL) == 0) { prefix |= key0 & (255ULL << (8 * pass)); continue; }
        for (int i = tid; i < 256; i += NT) hist[i] = 0;
        __syncthreads();
        const int sh_hi = 8 * (pass + 1);
        for (int i = tid; i < N; i += NT) {
            const unsigned long long key = keys[i];
            if (pass == 7 || (key >> sh_hi) == (prefix >> sh_hi)) atomicAdd(&hist[(int)((key >> (8 * pass)) & 255ULL)], 1);
        }
        __syncthreads();
        // bucket holding the kk-th smallest key of the current group
        int run = 0;
        for (int base = 0; base < 256; base += NT) {
            const int b = base + tid;
            const int h = b < 256 ? hist[b] : 0;
            int tot, ex = block_exscan<NT>(h, sh, &tot);
            if (b < 256 && run + ex < kk && kk <= run + ex + h) { sh[28] = b; sh[29] = kk - (run + ex); sh[30] = h; }
            run += tot;
            __syncthreads();
        }
        prefix |= (unsigned long long)(unsigned)sh[28] << (8 * pass);
        kk = sh[29];
        take_le = kk == sh[30];
        __syncthreads();
        if (take_le) prefix |= (pass > 0) ? ((1ULL << (8 * pass)) - 1ULL) : 0ULL;      // (the largest key the bin can hold)
    }
    // `prefix` is now the K-th smallest key (or, stopped early, an upper bound of the wanted bin that no unwanted key reaches):
    // keep every key <= prefix - exactly K, keys are distinct
    int outn = 0;
    for (int base = 0; base < N; base += NT) {
        const int i = base + tid;
        unsigned long long key = 0;
        int f = 0;
        if (i < N) { key = keys[i]; f = key <= prefix ? 1 : 0; }
        int tot, ex = block_exscan_flag<NT>(f, sh, &tot);     // (barriers inside: all reads of this slab are done)
        if (f) keys[outn + ex] = key;                     // outn + ex <= i: never clobbers an unread key
        outn += tot;
        __syncthreads();
    }
}

struct PlainView {
    const int16_t *pt;
    __device__ __forceinline__ int operator()(int x) const { return pt[x]; }
};

// ---------------------------------------------------------------- kernels, one file each, in the order they need each other

#include "rafft_expand_common.h"       // what the two expand kernels must agree on: lag value, eligible prefix, candidate records, statistics lines
#include "rafft_expand.hip"             // fetch_plan / fetch_chunk, wave_sync; RegionA, the phases, expand_kernel
#include "rafft_expand_small.hip"       // expand_small_kernel
#include "rafft_beam.hip"               // beam_step_kernel, the seen table
#include "rafft_materialize.hip"        // materialize_kernel, materialize_team_kernel, dedupe_kernel
#include "rafft_io_kernels.hip"         // stage_in_kernel, init_roots_kernel, output_kernel, eval_kernel
#include "rafft_moves.h"                // the single-pair move set of the four below: FpView, enclosing_pair, next_partner, moves_at, structure_energy
#include "rafft_findpath.hip"           // findpath_init_kernel, findpath_expand_kernel, findpath_select_kernel, findpath_trace_kernel
#include "rafft_descend.hip"            // descend_kernel
#include "rafft_barriers.hip"           // barriers_keys_kernel, barriers_insert_kernel, barriers_scan_kernel, barriers_basin_kernel
#include "rafft_kinfold.hip"            // kinfold_kernel
