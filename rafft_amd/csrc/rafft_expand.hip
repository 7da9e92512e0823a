// rafft_expand.hip - expand_kernel: the general expand kernel of the fold hot path (gfx950), and what it shares with
// expand_small_kernel: the work-list fetch (fetch_plan / fetch_chunk) and wave_sync.  Included by rafft_kernels.hip.
// In this order: mask_window / build_masks, the fetch, the synchronisation; RegionA, the one view of the time-shared LDS region
// (with the table of its tenants), and ExpandRegion, what a phase needs of team and region; the phases of one region in execution
// order - load_region, fft_correlate, lag_values_masks / _wave / _fft, select_lags, sort_lags_inplace, report_ranking,
// window_slide_cells (the masks form stands in the kernel), branch_prefix_sums, stems_dE, emit_wave / emit_team - every one
// __forceinline__; then expand_kernel: the fetch loop, the region header, the decisions, and the list of calls.
#pragma once

// ------------------------------------------------------------ expand kernel

// 64 bits of the bit string X (W words) starting at bit `start` (may be negative / past the end -> zeros)
__device__ __forceinline__ unsigned long long mask_window(const unsigned long long *X, int W, int start)
{
    if (start >= 64 * W || start <= -64) return 0ULL;
    const int q = start >> 6, bsh = start & 63;           // arithmetic shift: floor division
    const unsigned long long lo = (q >= 0 && q < W) ? X[q] : 0ULL;
    const unsigned long long hi = (q + 1 >= 0 && q + 1 < W) ? X[q + 1] : 0ULL;
    return bsh ? (lo >> bsh) | (hi << (64 - bsh)) : lo;
}

// Bit masks of a region: forward masks F[0..3] = positions holding A, C, G, U, F[4] = contiguity with the previous
// position; R[0..3] = the base strings reversed (bit j of R = bit n-1-j of F), R[4] = "contiguous with the NEXT position" reversed
// (bit j of R[4] = bit n-j of F[4]) - so that for the cell (ip, jp = lag - ip) of a diagonal all five reversed strings are read at
// the same bit n - 1 - lag + ip.  W words each, F first, then R.  One synchronisation inside (the caller adds the one behind).
// (`code_at(t)`: the base code of the region's position t - an LDS array, or the sequence's codes read through `pos` for the class
//  whose regions are too big for an LDS copy)
template <int NT, class CodeAt>
__device__ inline void build_masks(unsigned long long *F, unsigned long long *R, int W, int n, const CodeAt &code_at, const uint16_t *pos, int tid)
{
    for (int wq = tid >> 6; wq < W; wq += NT / 64) {       // each wavefront ballots whole 64-bit words
        const int t = wq * 64 + (tid & 63);
        const int c0 = t < n ? code_at(t) : 0;
        const unsigned long long bA = __ballot(c0 == 1), bC = __ballot(c0 == 2), bG = __ballot(c0 == 3), bU = __ballot(c0 == 4);
        const unsigned long long bg = __ballot(t >= 1 && t < n && (int)pos[t] - (int)pos[t > 0 ? t - 1 : 0] == 1);
        if ((tid & 63) == 0) { F[0 * W + wq] = bA; F[1 * W + wq] = bC; F[2 * W + wq] = bG; F[3 * W + wq] = bU; F[4 * W + wq] = bg; }
    }
    if (NT == 64) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } else __syncthreads();
    // reverse the whole 64 W-bit string (word order and bit order), then shift the n live bits down:
    // R bit j = T bit (j + 64 W - n) with T[w] = brev(F[W-1-w]); bits of F past n are zero.  The contiguity string is shifted one
    // bit less (bit j = F[4] bit n - j = T bit j + 64 W - n - 1; its bit 0 is F[4] bit n: zero)
    for (int idx = tid; idx < 5 * W; idx += NT) {
        const int which = idx / W, w = idx - which * W;
        const int s0 = 64 * w + 64 * W - n - (which == 4 ? 1 : 0), q = s0 >> 6, bsh = s0 & 63;      // (arithmetic shift: q = -1 for s0 = -1)
        const unsigned long long lo = q >= 0 && q < W ? __brevll(F[which * W + W - 1 - q]) : 0ULL;
        const unsigned long long hi = q + 1 < W ? __brevll(F[which * W + W - 2 - q]) : 0ULL;
        R[which * W + w] = bsh ? (lo >> bsh) | (hi << (64 - bsh)) : lo;
    }
}

// Next chunk of CH work items of class `cls` for this wavefront (all 64 lanes call it; `shard` is the wavefront's current
// shard, `failed` the shards it has found empty - both kept between calls): returns the first item of the chunk, or ~0u
// when every chunk of the list has been handed out.  Chunk c belongs to shard c % NSHARD; the fast path is ONE returning
// atomic on the wavefront's own shard (64 cursors, 64 bytes apart: 0.56 ns per atomic chip-wide against 11.4 ns on a
// single cursor, tools/micro/atomic_spacing.hip).  Whoever claims the last chunk of a shard sets its bit in wdone[cls];
// a wavefront that finds its shard empty reads that ONE word and moves to a shard that still has chunks.
// Chunks taper: the first Dev::taper_pct percent of a list go out CH items at a time, the rest CT at a time (`count` says which) -
// the wavefronts that finish a launch are then a fraction of a big chunk apart, not a whole one.
struct FetchPlan { unsigned cA, nA, chunks_total, CH, CT; unsigned long long exist; };      // (what fetch_chunk needs of a list: computed once per launch)
__device__ inline FetchPlan fetch_plan(const Dev &d, unsigned n_items, unsigned CH, unsigned CT)
{
    FetchPlan f;
    f.CH = CH; f.CT = CT;
    f.cA = CH > CT ? (unsigned)(((unsigned long long)n_items * (unsigned long long)d.taper_pct / 100ULL) / CH) : n_items / CH;      // big chunks
    f.nA = f.cA * CH;                                                                                                            // items in them
    f.chunks_total = f.cA + (n_items - f.nA + CT - 1) / CT;
    f.exist = f.chunks_total >= NSHARD ? ~0ULL : ((1ULL << f.chunks_total) - 1ULL);      // shards that hold any chunk
    return f;
}
__device__ inline unsigned fetch_chunk(const Dev &d, int cls, const FetchPlan &f, int &shard, unsigned long long &failed, unsigned &count)
{
    const int lane = threadIdx.x & 63;
    const unsigned cA = f.cA, nA = f.nA, chunks_total = f.chunks_total, CH = f.CH, CT = f.CT;
    const unsigned long long exist = f.exist;
    for (;;) {
        if ((exist >> shard) & ~(failed >> shard) & 1ULL) {
            const unsigned cnt = (chunks_total - (unsigned)shard + (NSHARD - 1)) / NSHARD;                     // chunks of this shard
            unsigned k = 0;
            if (lane == 0) k = (unsigned)atomicAdd(&d.c->wcur[cls][shard].v, 1ULL);
            k = (unsigned)__builtin_amdgcn_readfirstlane((int)k);
            if (k < cnt) {
                if (k == cnt - 1 && lane == 0) atomicOr(&d.c->wdone[cls], 1ULL << shard);
                const unsigned c = (unsigned)shard + NSHARD * k;
                if (c < cA) { count = CH; return c * CH; }
                count = CT;
                return nA + (c - cA) * CT;
            }
            failed |= 1ULL << shard;
        }
        unsigned long long done = 0;
        if (lane == 0) done = __hip_atomic_load(&d.c->wdone[cls], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        done = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(done >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)done);
        const unsigned long long live = exist & ~(done | failed);
        if (!live) return ~0u;
        const unsigned long long rot = shard ? ((live >> shard) | (live << (64 - shard))) : live;
        shard = (shard + __ffsll((long long)rot) - 1) & (NSHARD - 1);
    }
}
static_assert(NSHARD == 64, "fetch_chunk reads one work cursor per lane");

#ifndef RAFFT_EXPAND256_PROD_WAVES
#define RAFFT_EXPAND256_PROD_WAVES 4
#endif
#ifndef RAFFT_EXPAND64_WAVES
#define RAFFT_EXPAND64_WAVES 3        // <= 168 VGPRs (12 B/lane of scratch): its LDS allows three wavefronts per SIMD anyway; a cap of 128 spilled 152 B/lane
#endif
// Synchronisation inside one region's work.  The one-wavefront class needs no s_barrier: the LDS operations of a
// wavefront execute in program order, so a compiler fence at wavefront scope is all it takes - and, unlike
// __syncthreads(), it does not wait for the global loads in flight.  That also lets WPB wavefronts share a workgroup
// (each with its own slice of LDS and its own regions, never waiting for each other) and with it ONE copy of the hot
// energy tables in LDS.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
#define ESYNC() do { if (NT == 64) wave_sync(); else __syncthreads(); } while (0)

// ------------------------------------------------------------ region A of a team's LDS

struct WsPart { double score; int nb, mi, mj, any; };      // what one chunk of a chunked diagonal found (window_slide)

// Region A - the bytes [lay.offA, lay.offA + lay.szA) of a team's LDS (expand_lds) - is time-shared.  This struct is the one place in the
// kernel that spells the addresses of the tenants below; it is built once per region.  W = ceil(n / 64) mask words; K8 = 8 Pk, the bytes of the lag values
// (Pk = P, or 0 when they live in HBM: LONGSEQ 2); tail = 0 when the lag values were sorted in place and are dead, else K8.
//
//   tenant          offset              bytes         written by          last read by         aliases, on purpose
//   z1()            0                   8 P           fft_correlate       lag_values_fft       keyv: keyv[k] replaces z1[k] byte for byte, written by
//                                                                                              the thread that read it
//   z2()            8 P                 8 P           fft_correlate       lag_values_fft       every tenant below: all written after its last read
//   keyv()          0 (HBM: `big`)      8 P           lag_values_*        emit_* (dE ties)     z1
//   lagk()          8 P (HBM: big + P)  2 P           store_lag_values,   sort_lags_inplace    head of z2 (filled behind a barrier); the masks of
//                                                     when `inplace`                           the correlation (window_slide rebuilds them)
//   masks()         K8                  80 W          lag_values_masks    window_slide, masks  - (one build serves both unless `inplace`)
//   slide_masks()   tail                80 W          window_slide, masks window_slide, masks  keyv and lagk when `inplace` (dead by then)
//   hist()          9 P; no FFT buffers: 1024 + 128   select_lags         select_lags          - (80 W <= 0.69 P: the masks end below 9 P; without
//                   8 P + 80 ceil(nmax / 64);                                                  FFT buffers it follows the largest masks; beyond 4096
//                   LONGSEQ 2: szA - 2048                                                      positions the plan keeps the last 2 KiB for it)
//   slide_parts()   tail + 80 W         24 Kp C       window_slide, masks merge_slide_parts    hist (select_lags is over)
//   cell_parts()    K8                  24 Kp C       window_slide_cells  merge_slide_parts    masks, hist (the cell-by-cell form builds no masks)
//   prefix_sums()   tail                10 (nbr + 1)  branch_prefix_sums  stems_dE             slide masks and parts (window_slide is over)
//   sort_keys()     tail                8 nkept       emit_team           emit_team            the prefix sums (stems_dE is over)
//
//   per-lag arrays  8 Pmax + 24 KiB     14 B per lag  (rk, wnb, wmi, widx, dd, keep: through the pointers of ExpandTeam, not through this struct)
//                   only when expand_lds's `lag_in_A` holds (Pmax = MAX_P, Kmax > 256): written from select_lags on, read to the end; they
//                   alias the upper part of z2 (dead by then) and nothing else - masks (<= 5 KiB), prefix sums (<= 10 KiB) and the
//                   histogram (at 9 P, 1.2 KiB) all end below 8 P + 24 KiB, and diagonals are not chunked for Kmax > 256 (no parts)
//
// expand_lds (rafft_kernels.h) sizes region A for these tenants and the fit checks of class_cfg (rafft_plan.h) bound them per size class.
template <int LONGSEQ>
struct RegionA {
    unsigned char *a;          // lds + lay.offA
    double *big;               // LONGSEQ 2: this team's lag values in HBM
    int P, Pk, n, nmax, szA;
    bool nofft;
    bool selected, inplace;    // the Kp best lags are selected / all keys are sorted in place (neither: every lag is searched)
    __device__ __forceinline__ RegionA(unsigned char *lds, const ExpandLds &lay, int P_, int Pk_, int n_, int nmax_, bool selected_, bool inplace_, bool nofft_, const Dev &d, unsigned gteam)
        : a(lds + lay.offA), big(LONGSEQ == 2 ? d.big_keyv + (size_t)gteam * d.big_stride : nullptr), P(P_), Pk(Pk_), n(n_), nmax(nmax_), szA(lay.szA),
          nofft(nofft_), selected(selected_), inplace(inplace_) {}
    // (every address is worked out where it is used, from values the kernel holds anyway: none occupies a register between phases)
    __device__ __forceinline__ int W() const { return (n + 63) >> 6; }
    __device__ __forceinline__ int tail() const { return inplace ? 0 : 8 * Pk; }
    __device__ __forceinline__ float2 *z1() const { return (float2 *)a; }
    __device__ __forceinline__ float2 *z2() const { return (float2 *)a + P; }
    __device__ __forceinline__ double *keyv() const { return LONGSEQ == 2 ? big : (double *)a; }
    __device__ __forceinline__ uint16_t *lagk() const { return LONGSEQ == 2 ? (uint16_t *)(big + P) : (uint16_t *)(a + 8 * P); }
    // forward masks F (MASK_F_WORDS strings of W words), the reversed ones R behind them (build_masks)
    __device__ __forceinline__ unsigned long long *masks() const { return (unsigned long long *)(a + 8 * Pk); }
    __device__ __forceinline__ unsigned long long *slide_masks() const { return (unsigned long long *)(a + tail()); }
    __device__ __forceinline__ int *hist() const { return (int *)(a + (LONGSEQ == 2 ? szA - 2048 : nofft ? 8 * P + 8 * MASK_WORDS * ((nmax + 63) >> 6) : 9 * P)); }   // 256 bins, then the scan scratch shs[32]
    __device__ __forceinline__ WsPart *slide_parts() const { return (WsPart *)((slide_masks() + MASK_F_WORDS * W()) + (MASK_WORDS - MASK_F_WORDS) * W()); }   // behind R
    __device__ __forceinline__ WsPart *cell_parts() const { return (WsPart *)(a + 8 * Pk); }
    __device__ __forceinline__ int *prefix_sums() const { return (int *)(a + tail()); }                   // pe_ext[nbr + 1], pe_ml[nbr + 1], psp[nbr + 1]
    __device__ __forceinline__ unsigned long long *sort_keys() const { return (unsigned long long *)(a + tail()); }
};

// What the phases need: of the team - its arrays in region B of the LDS, the energy tables, the seam; filled once per launch - and of
// the region in hand, filled by name per region.  Every phase takes it by const reference and is inlined: no copy is made.
struct ExpandTeam {
    int tid;                   // position inside the region's team
    uint16_t *pos; uint8_t *code; uint32_t *P2; uint32_t *brl;
    uint16_t *rk, *wnb, *wmi, *widx; int *dd; uint16_t *keep; const double *wtab; int *misc;
    const SmallT *T; const BigT *B;
    DebugOut dbg;
};
template <bool CODE_LDS_>
struct ExpandRegion : ExpandTeam {
    static constexpr bool CODE_LDS = CODE_LDS_;
    int nid, n, m, P, logP, Kp, nbr, ci, cj, L, par_dcal;
    const uint8_t *codes, *Sl;
    // the base code of the region's position t - an LDS array, or the sequence's codes read through `pos`
    __device__ __forceinline__ int code_at(int t) const { return CODE_LDS ? (int)code[t] : (int)codes[pos[t]]; }
};

// ------------------------------------------------------------ the phases of one region, in execution order

// The loop: unpaired positions, their base codes (bytes, and 2 bits each in P2), the span of bases it looks at, the branch words.
template <int NT, int LONGSEQ, class G>
__device__ __forceinline__ void load_region(const Dev &d, const G &g, const uint16_t *posg, const uint32_t *brg, uint8_t *Sl_lds, int sx0, int sx1, int spad)
{
    const int tid = g.tid, n = g.n;
    // (every lane of the team walks the loop, so that the rows of 16 lanes that pack the bases - 2 bits each, SmallT::stk4 - are whole)
    for (int t0 = 0; t0 < n; t0 += NT) {
        const int t = t0 + tid;
        int c = 0;
        if (t < n) {
            const int p = posg[t];
            if (d.pos_packed) { g.pos[t] = (uint16_t)(p & 0x0FFF); c = p >> 12; g.code[t] = (uint8_t)c; }   // (Dev::pos_packed: no sequence beyond 4096 nt in this wave)
            else { g.pos[t] = (uint16_t)p; if (G::CODE_LDS) { c = g.codes[p]; g.code[t] = (uint8_t)c; } }
        }
        if (G::CODE_LDS) {
            const uint32_t x = row16_or((uint32_t)((c + 3) & 3) << (2 * (t & 15)));
            if ((t & 15) == 15 && t - 15 < n) g.P2[t >> 4] = x;
        }
    }
    if (G::CODE_LDS && tid == 0) g.P2[(n + 15) >> 4] = 0u;       // (the word of slack behind the last: strand_window reads two)
    if (LONGSEQ == 0) {   // bases: only the span of this loop is ever looked at (closing pair, its neighbours inside, branches)
        const uint32_t *src4 = (const uint32_t *)(g.codes + sx0 - spad);
        const int nw4 = (sx1 - sx0 + spad + 3) >> 2;
        for (int x = tid; x < nw4; x += NT) ((uint32_t *)Sl_lds)[x] = src4[x];
    }
    for (int t = tid; t < g.nbr; t += NT) g.brl[t] = d.pos_packed ? (brg[t] & 0x0FFF0FFFu) : brg[t];   // (Dev::pos_packed: the codes ride along)
    ESYNC();
}

__device__ __forceinline__ float2 add2(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 sub2(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// Forward (DIF) butterflies on one buffer: two radix-2 stages (spans s and s/2 = h) on four elements held in registers, and the
// last stage alone when the number of stages is odd ...
__device__ __forceinline__ void dif_radix4(float2 *z, int j, int h, int s, float2 w1a, float2 w1b, float2 w2)
{
    const float2 x0 = z[j], x1 = z[j + h], x2 = z[j + s], x3 = z[j + s + h];
    const float2 a0 = add2(x0, x2), a2 = cmul(sub2(x0, x2), w1a), a1 = add2(x1, x3), a3 = cmul(sub2(x1, x3), w1b);
    z[j] = add2(a0, a1); z[j + h] = cmul(sub2(a0, a1), w2);
    z[j + s] = add2(a2, a3); z[j + s + h] = cmul(sub2(a2, a3), w2);
}
__device__ __forceinline__ void dif_radix2(float2 *z, int j, float2 w)
{
    const float2 a = z[j], bb = z[j + 1];
    z[j] = add2(a, bb); z[j + 1] = cmul(sub2(a, bb), w);
}
// ... and the inverse (DIT) ones: spans s1 and s2 = 2 s1, the first stage alone when the number of stages is odd
__device__ __forceinline__ void dit_radix4(float2 *z, int j, int s1, int s2, float2 w1, float2 w2a, float2 w2b)
{
    const float2 x0 = z[j], x2 = z[j + s2];
    const float2 t1 = cmulc(z[j + s1], w1), t3 = cmulc(z[j + s2 + s1], w1);
    const float2 y0 = add2(x0, t1), y1 = sub2(x0, t1), y2 = add2(x2, t3), y3 = sub2(x2, t3);
    const float2 u2 = cmulc(y2, w2a), u3 = cmulc(y3, w2b);
    z[j] = add2(y0, u2); z[j + s2] = sub2(y0, u2); z[j + s1] = add2(y1, u3); z[j + s2 + s1] = sub2(y1, u3);
}
__device__ __forceinline__ void dit_radix2(float2 *z, int j, float2 w)
{
    const float2 a = z[j], bb = cmulc(z[j + 1], w);
    z[j] = add2(a, bb); z[j + 1] = sub2(a, bb);
}

// conv(A,U), conv(G,C), conv(G,U) of the region with itself by two packed complex FFTs in LDS: on return z1[k] = (AU, GC) pair
// counts of lag k times P, z2[k].x = GU (`tw`: exp(-2 pi i m / twN), m < twN / 2)
template <int NT, class G, class RA>
__device__ __forceinline__ void fft_correlate(const G &g, const RA &A, const float2 *tw, int twN)
{
    const int tid = g.tid, n = g.n, P = g.P, logP = g.logP;
    float2 *z1 = A.z1(), *z2 = A.z2();
    for (int t = tid; t < P; t += NT) {
        int c = t < n ? g.code[t] : 0;
        z1[t] = make_float2(c == 1 ? 1.f : 0.f, c == 3 ? 1.f : 0.f); // A + iG
        z2[t] = make_float2(c == 4 ? 1.f : 0.f, c == 2 ? 1.f : 0.f); // U + iC
    }
    ESYNC();
    // DIF, natural in -> bit-reversed out.  Two radix-2 stages (spans s and s/2) are done per pass on four
    // elements held in registers: the same operations in the same order as stage by stage (bit-identical
    // results), half the LDS traffic and barriers.
    int s = P >> 1;
    for (; s >= 2; s >>= 2) {
        const int h = s >> 1, tws = (twN / 2) / s;
        for (int b = tid; b < (P >> 2); b += NT) {
            const int off = b & (h - 1);
            const int j = ((b - off) << 2) + off;          // j mod 2s < s/2
            const float2 w1a = tw[off * tws], w1b = tw[(off + h) * tws], w2 = tw[off * 2 * tws];
            dif_radix4(z1, j, h, s, w1a, w1b, w2);
            dif_radix4(z2, j, h, s, w1a, w1b, w2);
        }
        ESYNC();
    }
    if (s == 1) {                                           // odd number of stages: the last one alone
        for (int b = tid; b < (P >> 1); b += NT) {
            const int j = b << 1;
            dif_radix2(z1, j, tw[0]);
            dif_radix2(z2, j, tw[0]);
        }
        ESYNC();
    }
    // separate the packed real spectra, multiply.  The spectra sit in bit-reversed order: walking k = 0, 1, 2 ... would
    // send the 64 lanes of a wavefront to addresses P/2, P/4 ... apart - one LDS bank for all of them.  So the walk is
    // over the POSITIONS: the even ones hold exactly the k < P/2 (top bit of k = lowest bit of the position), position 1
    // holds k = P/2; neighbours in the walk are neighbours in LDS, and the mirror position of -k runs the other way.
    for (int t = tid; t <= (P >> 1); t += NT) {
        const int jk = t == (P >> 1) ? 1 : 2 * t;
        const int k = (int)(__brev((unsigned)jk) >> (32 - logP));
        const int km = (P - k) & (P - 1);
        const int jm = (int)(__brev((unsigned)km) >> (32 - logP));
        float2 A1 = z1[jk], B1 = z1[jm], A2 = z2[jk], B2 = z2[jm];
        float2 Fa = make_float2(0.5f * (A1.x + B1.x), 0.5f * (A1.y - B1.y));
        float2 Fg = make_float2(0.5f * (A1.y + B1.y), -0.5f * (A1.x - B1.x));
        float2 Fu = make_float2(0.5f * (A2.x + B2.x), 0.5f * (A2.y - B2.y));
        float2 Fc = make_float2(0.5f * (A2.y + B2.y), -0.5f * (A2.x - B2.x));
        float2 X = cmul(Fa, Fu), Y = cmul(Fg, Fc), Z = cmul(Fg, Fu);
        z1[jk] = make_float2(X.x - Y.y, X.y + Y.x);
        z2[jk] = Z;
        if (jm != jk) {
            z1[jm] = make_float2(X.x + Y.y, Y.x - X.y);
            z2[jm] = make_float2(Z.x, -Z.y);
        }
    }
    ESYNC();
    // DIT inverse, bit-reversed in -> natural out; again two stages (spans s and 2s) per pass
    int si = 1;
    if (logP & 1) {                                         // odd number of stages: the first one alone
        for (int b = tid; b < (P >> 1); b += NT) {
            const int j = b << 1;
            dit_radix2(z1, j, tw[0]);
            dit_radix2(z2, j, tw[0]);
        }
        ESYNC();
        si = 2;
    }
    for (; si < P; si <<= 2) {
        const int s1 = si, s2 = si << 1, tws = (twN / 2) / s1;
        for (int b = tid; b < (P >> 2); b += NT) {
            const int off = b & (s1 - 1);
            const int j = ((b - off) << 2) + off;          // j mod 4 s1 < s1
            const float2 w1 = tw[off * tws], w2a = tw[off * (tws >> 1)], w2b = tw[(off + s1) * (tws >> 1)];
            dit_radix4(z1, j, s1, s2, w1, w2a, w2b);
            dit_radix4(z2, j, s1, s2, w1, w2a, w2b);
        }
        ESYNC();
    }
}

// ---- lag values (exact integer pair counts, IEEE fp64 divide) in three forms, one per form of the correlation.
// (round 5, production builds - weights >= 0) The top byte of the order-preserving key of a lag value - sign and the upper seven
// bits of the exponent - only says whether the value is 0, below 2 or at least 2: counted while the values are stored with three
// ballots per 64 lags (wavefront-uniform counters: scalar registers), which is the radix select's first pass without a pass over the
// keys - for the class whose lag values live in HBM one read of them less.  Values outside [2^-15, 2^17) (user weights of another
// scale) or a negative one: `c_odd`, and the select starts at the top byte as before.
struct LagTally { int c_hi = 0, c_lo = 0, c_odd = 0; };

// What the three forms share: every lag k < P gets its value (value_of(k); -inf behind the 2n-1 real ones) stored and tallied;
// then, for the in-place sort, the lag column.  (With FFT buffers keyv[k] aliases z1[k] byte for byte and is written by the thread
// that read it; lagk aliases the head of z2 - or the masks of the correlation, rebuilt for window_slide - so it is filled only
// behind the barrier.)
template <int NT, int PROD, class G, class RA, class ValueOf>
__device__ __forceinline__ void store_lag_values(const G &g, const RA &A, LagTally &ty, const ValueOf &value_of)
{
    double *keyv = A.keyv();
    for (int k = g.tid; k < g.P; k += NT) {
        const bool valid = k < g.m;
        const double v = valid ? value_of(k) : -INFINITY;
        keyv[k] = v;
        if (PROD && A.selected) {
            ty.c_hi += __popcll(__ballot(valid && v >= 2.0));
            ty.c_lo += __popcll(__ballot(valid && v > 0.0 && v < 2.0));
            ty.c_odd |= __ballot(valid && (v >= 131072.0 || v < 0.0 || (v > 0.0 && v < 0x1p-15))) != 0ULL ? 1 : 0;
        }
    }
    ESYNC();
    if (A.inplace) {
        uint16_t *lagk = A.lagk();
        for (int k = g.tid; k < g.P; k += NT) lagk[k] = (uint16_t)k;
        ESYNC();
    }
}

// Multi-word bit masks (the wide classes up to Dev::direct_n positions, always beyond 4096): the base masks of the region - the
// same arrays the masks form of window_slide uses, built once here - and the three pair counts of every lag: bit ip of
// window(R_x, sft + 64 w) = base x at position k - ip
template <int NT, int PROD, class G, class RA>
__device__ __forceinline__ void lag_values_masks(const Dev &d, const G &g, const RA &A, LagTally &ty)
{
    const int n = g.n, m = g.m, W = A.W();
    unsigned long long *F = A.masks(), *R = F + MASK_F_WORDS * W;
    build_masks<NT>(F, R, W, n, [&](int t) -> int { return g.code_at(t); }, g.pos, g.tid);
    ESYNC();
    store_lag_values<NT, PROD>(g, A, ty, [&](int k) -> double {
        // Only the words that hold cells of this diagonal - positions ip with 0 <= k - ip < n - are visited (half of them on
        // average: the lags near either end have short diagonals), and the 64-bit window of the reversed masks slides: every
        // step loads ONE new word per mask and reuses the high word of the step before (mask_window would load two and
        // range-check both).  Same bits, same counts.
        const int sft = n - 1 - k;
        const int ip_lo = k > n - 1 ? k - (n - 1) : 0, ip_hi = k < n - 1 ? k : n - 1;
        const int w0 = ip_lo >> 6, w1 = ip_hi >> 6;
        const int start = (w0 << 6) + sft;                 // first bit of the window of word w0 (negative: bits before the string are zeros)
        int q = start >> 6;                                 // (arithmetic shift: floor)
        const int bsh = start & 63;
        const unsigned long long *RU = R + 3 * W, *RC = R + 1 * W;
        unsigned long long loU = (q >= 0 && q < W) ? RU[q] : 0ULL, loC = (q >= 0 && q < W) ? RC[q] : 0ULL;
        int cAU = 0, cGC = 0, cGU = 0;
        for (int w = w0; w <= w1; w++, q++) {
            const bool in = q + 1 >= 0 && q + 1 < W;
            const unsigned long long hiU = in ? RU[q + 1] : 0ULL, hiC = in ? RC[q + 1] : 0ULL;
            const unsigned long long xU = bsh ? (loU >> bsh) | (hiU << (64 - bsh)) : loU, xC = bsh ? (loC >> bsh) | (hiC << (64 - bsh)) : loC;
            const unsigned long long fA = F[0 * W + w], fG = F[2 * W + w];
            cAU += __popcll(fA & xU); cGC += __popcll(fG & xC); cGU += __popcll(fG & xU);
            loU = hiU; loC = hiC;
        }
        return lag_value((double)cAU, (double)cGC, (double)cGU, k, m, d);
    });
}

// One wavefront, regions of <= 64 positions: the whole strand is one 64-bit mask per base, in registers
template <int NT, int PROD, class G, class RA>
__device__ __forceinline__ void lag_values_wave(const Dev &d, const G &g, const RA &A, LagTally &ty)
{
    const int n = g.n, m = g.m;
    const int c = g.tid < n ? g.code[g.tid] : 0;
    const unsigned long long mA = __ballot(c == 1), mC = __ballot(c == 2), mG = __ballot(c == 3), mU = __ballot(c == 4);
    const unsigned long long rU = __brevll(mU) >> (64 - n), rC = __brevll(mC) >> (64 - n);   // strand reversed
    store_lag_values<NT, PROD>(g, A, ty, [&](int k) -> double {
        const int sft = n - 1 - k;                     // bit i of x* = base at position k - i
        const unsigned long long xU = sft >= 0 ? (rU >> sft) : (rU << -sft);
        const unsigned long long xC = sft >= 0 ? (rC >> sft) : (rC << -sft);
        return lag_value((double)__popcll(mA & xU), (double)__popcll(mG & xC), (double)__popcll(mG & xU), k, m, d);
    });
}

// From the FFT: the pair counts are the rounded real and imaginary parts of z1, z2 over P
template <int NT, int PROD, class G, class RA>
__device__ __forceinline__ void lag_values_fft(const Dev &d, const G &g, const RA &A, LagTally &ty)
{
    const float2 *z1 = A.z1(), *z2 = A.z2();
    const float invP = 1.0f / (float)g.P;
    store_lag_values<NT, PROD>(g, A, ty, [&](int k) -> double {
        // (+ 0.0: a lag without a pair comes out of the FFT as +-1e-7 and rintf keeps the sign - three counts of -0.0f made
        //  the value -0.0, which the bit-pattern keys of the ranking put BELOW the +0.0 of the other empty lags, where the
        //  reference's exact 0.0 ties with them and the larger lag wins.  Seen on a 65-nt CUG repeat, whose top 100 reach into
        //  the empty lags: tests/test_gpu_ties.py.  -0.0 + 0.0 = +0.0; every other value is unchanged.)
        return lag_value((double)rintf(z1[k].x * invP), (double)rintf(z1[k].y * invP), (double)rintf(z2[k].x * invP), k, g.m, d) + 0.0;
    });
}

// ---- ranking.  Which lags are searched (rafft/rafft.py:117-118 takes the nb_mode best by (value desc, lag desc)):
//  - all of them when 2n-1 <= nb_mode: nothing to rank;
//  - otherwise the best nb_mode are SELECTED exactly (byte-wise radix select on the order-preserving bit
//    pattern of the fp64 value, ties: larger lag first) - their order is not needed, because the only
//    place it shows is the stable dE sort of the candidates, and that breaks ties from (value, lag) itself;
//  - tiny FFT sizes (P <= 128) and the debug seam, which reports the ranking, sort all keys in place.

// order-preserving unsigned key of a lag value
__device__ __forceinline__ unsigned long long lag_ukey(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}

// rk[0..Kp) = the Kp best lags, in no particular order.  (Production builds start from the tally of the top byte.)
template <int NT, int PROD, class G, class RA>
__device__ __forceinline__ void select_lags(const G &g, const RA &A, LagTally ty)
{
    const int tid = g.tid, m = g.m, P = g.P;
    const double *keyv = A.keyv();
    int *hist = A.hist();
    int *shs = hist + 256;                                   // scan scratch [32]
    unsigned long long prefix = 0;
    int kk = g.Kp;
    bool take_ge = false;          // every key >= prefix is selected (the threshold fell between two values)
    int pass0 = 7;
    if (PROD) {
        if (NT > 64) {             // (the counters are per wavefront: summed over the team)
            if (tid < 3) shs[20 + tid] = 0;
            ESYNC();
            if ((tid & 63) == 0) { atomicAdd(&shs[20], ty.c_hi); atomicAdd(&shs[21], ty.c_lo); atomicOr(&shs[22], ty.c_odd); }
            ESYNC();
            ty.c_hi = shs[20]; ty.c_lo = shs[21]; ty.c_odd = shs[22];
        }
        if (!ty.c_odd) {           // byte 7 of the keys: 0xC0 for [2, 2^17), 0xBF for [2^-15, 2), 0x80 for 0
            const int c_zero = m - ty.c_hi - ty.c_lo;
            int binc;
            if (kk <= ty.c_hi) { prefix = 0xC0ULL << 56; binc = ty.c_hi; }
            else if (kk <= ty.c_hi + ty.c_lo) { prefix = 0xBFULL << 56; kk -= ty.c_hi; binc = ty.c_lo; }
            else { prefix = 0x80ULL << 56; kk -= ty.c_hi + ty.c_lo; binc = c_zero; }
            pass0 = kk == binc ? -1 : 6;       // (the whole bin is wanted: nothing below that byte needs looking at)
            take_ge = kk == binc;
        }
    }
    for (int pass = pass0; pass >= 0; pass--) {
        for (int i = tid; i < 256; i += NT) hist[i] = 0;
        ESYNC();
        const int sh_hi = 8 * (pass + 1);
        for (int i = tid; i < m; i += NT) {
            const unsigned long long u = lag_ukey(keyv[i]);
            if (pass == 7 || (u >> sh_hi) == (prefix >> sh_hi)) atomicAdd(&hist[(int)((u >> (8 * pass)) & 255ULL)], 1);
        }
        ESYNC();
        // largest byte b with count(bytes > b) < kk <= count(bytes >= b): suffix scan over the bins
        {
            constexpr int BPT = NT >= 256 ? 1 : 256 / NT;      // bins per thread, from the top bin down
            int hs[BPT], mine = 0;
#pragma unroll
            for (int j = 0; j < BPT; j++) { const int bi = tid * BPT + j; hs[j] = bi < 256 ? hist[255 - bi] : 0; mine += hs[j]; }
            int tot, ex = block_exscan<NT>(mine, shs, &tot);
#pragma unroll
            for (int j = 0; j < BPT; j++) {
                if (ex < kk && kk <= ex + hs[j] && hs[j] > 0) { shs[28] = 255 - (tid * BPT + j); shs[29] = kk - ex; shs[30] = hs[j]; }
                ex += hs[j];
            }
            ESYNC();
        }
        prefix |= (unsigned long long)(unsigned)shs[28] << (8 * pass);
        kk = shs[29];
        const bool whole_bin = kk == shs[30];      // all keys of the threshold bin are wanted: no need to look
        ESYNC();                           // at the lower bytes (the usual case after two or three passes)
        if (whole_bin) { take_ge = true; break; }
    }
    // take every lag with key > prefix and the kk largest lags among key == prefix (sweep from the top)
    int outn = 0, tie_run = 0;
    for (int base = 0; base < P; base += NT) {
        const int i = P - 1 - (base + tid);
        unsigned long long u = 0;
        int tie = 0;
        if (i >= 0 && i < m) { u = lag_ukey(keyv[i]); tie = (u == prefix) ? 1 : 0; }
        int ttot = 0, tex = 0;
        if (!take_ge) tex = block_exscan_flag<NT>(tie, shs, &ttot);     // (the order among ties only matters when the cut falls inside them)
        const int gf = (i >= 0 && i < m) && (take_ge ? u >= prefix : (u > prefix || (tie && tie_run + tex < kk))) ? 1 : 0;
        int gtot, gex = block_exscan_flag<NT>(gf, shs, &gtot);
        if (gf) g.rk[outn + gex] = (uint16_t)i;
        outn += gtot; tie_run += ttot;
        ESYNC();
    }
}

// Bitonic network over N = 2^x elements in place: load(i) fetches an element, before(a, b) says whether a belongs in front of b,
// store(i, e) puts one back.  The one compare-exchange of both sorts below.
template <int NT, class Load, class Before, class Store>
__device__ __forceinline__ void bitonic_sort(int N, int tid, const Load &load, const Before &before, const Store &store)
{
    for (int k2 = 2; k2 <= N; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const auto ea = load(i), eb = load(ixj);
                    const bool a_first = before(ea, eb);
                    const bool up = (i & k2) == 0;
                    if (up ? !a_first : a_first) { store(i, eb); store(ixj, ea); }
                }
            }
            ESYNC();
        }
}

// Regions that are not ranked by selection: all keys sorted in place by (value desc, lag desc) when they must be ranked (or
// the seam reports the ranking), rk[] = the searched lags in rank order - or simply every lag.
template <int NT, class G, class RA>
__device__ __forceinline__ void sort_lags_inplace(const G &g, const RA &A)
{
    double *keyv = A.keyv();
    uint16_t *lagk = A.lagk();
    struct KeyLag { double v; uint16_t l; };
    if (A.inplace)
        bitonic_sort<NT>(g.P, g.tid, [&](int i) { return KeyLag{keyv[i], lagk[i]}; },
                         [](const KeyLag &a, const KeyLag &b) { return (a.v > b.v) || (a.v == b.v && a.l > b.l); },
                         [&](int i, const KeyLag &e) { keyv[i] = e.v; lagk[i] = e.l; });
    for (int r = g.tid; r < g.Kp; r += NT) {
        g.rk[r] = A.inplace ? lagk[r] : (uint16_t)r;
        if (g.dbg.lag) { g.dbg.lag[r] = lagk[r]; g.dbg.corval[r] = keyv[r]; }   // (debug seam always sorts)
    }
    if (g.tid == 0 && g.dbg.n_ranked) *g.dbg.n_ranked = g.Kp;
    ESYNC();
}

// The debug seam reports the ranking: sort the selected lags by (value desc, lag desc) and hand them out
template <int NT, class G, class RA>
__device__ __forceinline__ void report_ranking(const G &g, const RA &A)
{
    const int tid = g.tid, Kp = g.Kp;
    const double *keyv = A.keyv();
    uint16_t *rk = g.rk;
    if (g.dbg.lag != nullptr) {
        int M2 = 2; while (M2 < Kp) M2 <<= 1;
        for (int i = Kp + tid; i < M2; i += NT) rk[i] = 0xFFFF;      // (padding: behind every lag)
        ESYNC();
        bitonic_sort<NT>(M2, tid, [&](int i) { return rk[i]; },
                         [&](uint16_t la, uint16_t lb) {
                             if (la == 0xFFFF) return false;
                             if (lb == 0xFFFF) return true;
                             const double va = keyv[la], vb = keyv[lb];
                             return (va > vb) || (va == vb && la > lb);
                         },
                         [&](int i, uint16_t l) { rk[i] = l; });
    }
    for (int r = tid; r < Kp; r += NT)
        if (g.dbg.lag) { g.dbg.lag[r] = rk[r]; g.dbg.corval[r] = keyv[rk[r]]; }
    if (tid == 0 && g.dbg.n_ranked) *g.dbg.n_ranked = Kp;
    ESYNC();
}

// ---- window_slide (rafft/rafft.py:36-83).  Small regions: one lane per ranked lag.  Big regions: each diagonal is cut into C
// chunks handled by different lanes; a lane first walks back to the last zero cell before its chunk and replays the recurrence
// from there (same fp64 operation order, so values are bit-identical), then the chunk results are merged with the reference's
// `>=` rule.  (Chunking only for regions ranked by selection.)

// The half-diagonal of a lag: cell i is (ip0 + i, jp0 - i), i < len2
struct Diag { int len, len2, ip0, jp0; };
__device__ __forceinline__ Diag diag_of(int lagp, int n)
{
    Diag dg;
    dg.len = lagp < n ? lagp + 1 : 2 * n - lagp - 1;
    dg.len2 = (dg.len >> 1) + (dg.len & 1);
    dg.ip0 = lagp < n ? 0 : lagp - n + 1; dg.jp0 = lagp < n ? lagp : n - 1;
    return dg;
}
// what window_slide found for the lag of rank r
template <class G>
__device__ __forceinline__ void store_slide(const G &g, int r, int mx_nb, int mx_i, int mx_j, double mx_s)
{
    g.wnb[r] = (uint16_t)mx_nb; g.wmi[r] = (uint16_t)mx_i;      // (mj = lag - mi)
    if (g.dbg.nb) { g.dbg.nb[r] = mx_nb; g.dbg.mi[r] = mx_i; g.dbg.mj[r] = mx_j; g.dbg.score[r] = mx_s; }
}
// ... and the same from the C chunks of a chunked diagonal
template <int NT, class G>
__device__ __forceinline__ void merge_slide_parts(const G &g, const WsPart *parts, int C)
{
    ESYNC();
    for (int r = g.tid; r < g.Kp; r += NT) {
        double mx_s = 0.0;
        int mx_nb = 0, mx_i = 0, mx_j = 0;
        for (int c = 0; c < C; c++) {
            const WsPart wp = parts[r * C + c];
            if (wp.any && wp.score >= mx_s) { mx_s = wp.score; mx_nb = wp.nb; mx_i = wp.mi; mx_j = wp.mj; }
        }
        store_slide(g, r, mx_nb, mx_i, mx_j, mx_s);
    }
}

// Cell by cell, weights from the table by base codes: negative weights, or the forced-FFT test mode
template <int NT, class G, class RA>
__device__ __forceinline__ void window_slide_cells(const Dev &d, const G &g, const RA &A, int C)
{
    const uint16_t *pos = g.pos;
    const double *wtab = g.wtab;
    WsPart *parts = A.cell_parts();
    for (int q = g.tid; q < g.Kp * C; q += NT) {
        const int r = q / C, c = q - r * C;
        const Diag dg = diag_of(g.rk[r], g.n);
        const int ip0 = dg.ip0, jp0 = dg.jp0;
        const int a = (int)((long long)dg.len2 * c / C), e = (int)((long long)dg.len2 * (c + 1) / C);
        int z = a;                                  // replay start: just after the last zero cell before `a`
        while (z > 0 && wtab[g.code_at(ip0 + z - 1) * 5 + g.code_at(jp0 - (z - 1))] != 0.0) z--;
        double prev = 0.0, mx_s = 0.0;
        int tmp = 0, mx_nb = 0, mx_i = 0, mx_j = 0, any = 0;
        for (int i = z; i < e; i++) {
            const int ip = ip0 + i, jp = jp0 - i;
            double t = wtab[g.code_at(ip) * 5 + g.code_at(jp)];
            if (i > 0 && (int)pos[ip] - (int)pos[ip - 1] == 1 && (int)pos[jp + 1] - (int)pos[jp] == 1)
                t = (prev + t) * t;
            tmp = (t == 0.0) ? 0 : tmp + 1;
            if (i >= a && t >= mx_s && (int)pos[jp] - (int)pos[ip] > d.min_hp) {
                mx_s = t; mx_nb = tmp; mx_i = ip; mx_j = jp; any = 1;
            }
            prev = t;
        }
        if (C == 1) store_slide(g, r, mx_nb, mx_i, mx_j, mx_s);
        else { WsPart w; w.score = mx_s; w.nb = mx_nb; w.mi = mx_i; w.mj = mx_j; w.any = any; parts[q] = w; }
    }
    if (C > 1) merge_slide_parts<NT>(g, parts, C);
}

// ---- dE of every candidate stem: only the loops it changes, from the branch list

// Prefix sums of the branches' stem terms, so that every loop of stems_dE costs O(1) whatever its number of branches
template <int NT, class G, class RA>
__device__ __forceinline__ BrPrefix branch_prefix_sums(const G &g, const RA &A)
{
    const int tid = g.tid, nbr = g.nbr, ci = g.ci, L = g.L;
    const uint8_t *Sl = g.Sl;
    int *pe_ext = A.prefix_sums();
    int *pe_ml = pe_ext + (nbr + 1);
    uint16_t *psp = (uint16_t *)(pe_ml + (nbr + 1));
    if (tid < 64) {
        int c_e = 0, c_m = 0, c_s = 0;
        for (int base = 0; base < nbr; base += 64) {
            const int i = base + tid;
            int ve = 0, vm = 0, vs = 0;
            if (i < nbr) {
                const uint32_t u = g.brl[i];
                const int p = (int)(u & 0xffffu), q = (int)(u >> 16);
                const int tt = pair_type(Sl[p], Sl[q]);
                if (ci < 0) ve = e_stem(g.T, tt, p > 0 ? (int)Sl[p - 1] : -1, q < L - 1 ? (int)Sl[q + 1] : -1, true);
                vm = e_stem(g.T, tt, p > 0 ? (int)Sl[p - 1] : 0, q < L - 1 ? (int)Sl[q + 1] : 0, false);
                vs = q - p + 1;
            }
            const int xe = wave_incl_scan(ve), xm = wave_incl_scan(vm), xs = wave_incl_scan(vs);
            if (i < nbr) { pe_ext[i] = c_e + xe - ve; pe_ml[i] = c_m + xm - vm; psp[i] = (uint16_t)(c_s + xs - vs); }
            c_e += __builtin_amdgcn_readlane(xe, 63); c_m += __builtin_amdgcn_readlane(xm, 63); c_s += __builtin_amdgcn_readlane(xs, 63);
        }
        if (tid == 0) { pe_ext[nbr] = c_e; pe_ml[nbr] = c_m; psp[nbr] = (uint16_t)c_s; }
    }
    ESYNC();
    return BrPrefix{pe_ext, pe_ml, psp};
}

// dd[r] = the energy a stem adds, keep[r] = its flags (bit 0 kept, bit 1 involves a rule / model value, bit 2 evaluated), for
// every searched lag r that gave a stem
template <int NT, class G>
__device__ __forceinline__ void stems_dE(const Dev &d, const G &g, const BrPrefix &pf)
{
    const int tid = g.tid, Kp = g.Kp, nbr = g.nbr, ci = g.ci, cj = g.cj, L = g.L, par_dcal = g.par_dcal;
    const SmallT *T = g.T;
    const BigT *B = g.B;
    const uint8_t *Sl = g.Sl;
    const uint16_t *pos = g.pos;
    const uint32_t *brl = g.brl;
    const double par_e = dcal_to_energy(par_dcal);
    const BrList all_br{brl, 0, nbr, 0, 0, 0, 0, 0};
    int g_old = 0;           // (g: the energy involves a rule / model value of the built-in tables - SmallT::lsb)
    const int e_old = loop_energy_pre(T, B, Sl, L, ci, cj, all_br, pf, g_old);      // the loop as it is (same for every stem)
    // (round 5) the lags that gave a stem, compacted: two lags in three do, and the loop below - a lane per stem, every lane on
    // its own path through the loop energies - takes ceil(stems / 64) rounds instead of ceil(lags / 64): one instead of two for
    // half of the regions of the one-wavefront class
    int nst = 0;
    for (int base = 0; base < Kp; base += NT) {
        const int r = base + tid;
        const int f = (r < Kp && g.wnb[r] > 0) ? 1 : 0;
        if (r < Kp) g.keep[r] = 0;
        int tot, ex = block_exscan_flag<NT>(f, g.misc + 16, &tot);
        if (f) g.widx[nst + ex] = (uint16_t)r;
        nst += tot;
    }
    ESYNC();
    for (int si = tid; si < nst; si += NT) {
        const int r = g.widx[si];
        const int nb = g.wnb[r];
        {
            int gm = g_old;
            const int mi = g.wmi[r], mj = (int)g.rk[r] - mi;
            const int a0 = pos[mi], b0 = pos[mj], ao = pos[mi - nb + 1], bo = pos[mj + nb - 1];
            int lo, hi, lo_o, hi_o;
            br_lower4(brl, nbr, a0, b0, ao, bo, lo, hi, lo_o, hi_o);
            BrList outer{brl, 0, lo_o, hi_o, nbr, 1, ao, bo};
            int e_new = loop_energy_pre(T, B, Sl, L, ci, cj, outer, pf, gm);
            BrList inner{brl, lo, hi, 0, 0, 0, 0, 0};
            e_new += loop_energy_pre(T, B, Sl, L, a0, b0, inner, pf, gm);
            // the stem itself: a contiguous one (both strands without a gap - nearly all of them) of up to 16 pairs takes its
            // stacking energies from the packed strands, one look-up per pair (stem_stack_windows); the others pair by pair
            if (G::CODE_LDS && nb <= 16 && a0 - ao == nb - 1 && bo - b0 == nb - 1)
                e_new += stem_stack_windows(T, strand_window(g.P2, mi - nb + 1), strand_window(g.P2, mj), nb);
            else {
                int pa = a0, pb = b0, ty_in = pair_type(Sl[a0], Sl[b0]);
                for (int t = 1; t < nb; t++) {
                    const int a = pos[mi - t], b = pos[mj + t];
                    const int ty = pair_type(Sl[a], Sl[b]);
                    if (pa == a + 1 && pb == b - 1)
                        e_new += T->stack[ty][rtype(ty_in)];
                    else {
                        const int lo2 = br_lower(brl, nbr, a), hi2 = br_lower(brl, nbr, b);
                        BrList mid{brl, lo2, lo, hi, hi2, 1, pa, pb};
                        e_new += loop_energy_pre(T, B, Sl, L, a, b, mid, pf, gm);
                        lo = lo2; hi = hi2;
                    }
                    pa = a; pb = b; ty_in = ty;
                }
            }
            const int ddc = e_new - e_old;
            g.dd[r] = ddc;
            const double dE = dcal_to_energy(par_dcal + ddc) - par_e;
            g.keep[r] = (uint16_t)(((dE < d.min_nrj) ? 1 : 0) | (gm ? 2 : 0) | 4);     // bit 0 kept, bit 1 involves a rule / model value, bit 2 evaluated
            if (g.dbg.ddcal) g.dbg.ddcal[r] = ddc;
        }
    }
    if (g.dbg.ddcal) for (int r = tid; r < Kp; r += NT) if (g.wnb[r] == 0) g.dbg.ddcal[r] = INT_MIN;
    ESYNC();
}

// ---- stable sort of the kept candidates by dE (ties keep lag-rank order), emit

// A team's share of the launch's statistics (uniform over a wavefront team: scalar registers; thread 0's alone in a wider team; a
// team's share of one launch fits 32 bits)
struct TeamStats {
    unsigned items = 0, n = 0, lags = 0, nbr = 0;
    template <class G> __device__ __forceinline__ void count(const G &g) { items++; n += g.n; lags += g.Kp; nbr += g.nbr; }
};

// Candidate slots are reserved in slabs (one returning atomic per several regions): how many to ask for when `nkept` do not fit
// what is left of the team's slab
__device__ __forceinline__ unsigned cand_slab_want(const Dev &d, int nkept)
{
    const unsigned slab = d.cand_shard_cap >= 64u * (unsigned)d.cand_slab ? (unsigned)d.cand_slab : 16u;
    return (unsigned)nkept > slab ? (unsigned)nkept : slab;
}
// how many stem energies of this launch involved a rule / model value (built-in tables): counted in the team's LDS, not in
// registers that would live across the whole region loop.  `kf`: the flags of this lane's lag; called by whole wavefronts.
__device__ __forceinline__ void count_guessed(int *misc, int kf, bool first_lane)
{
    const int ne = __popcll(__ballot((kf & 4) != 0)), ng = __popcll(__ballot((kf & 6) == 6)), nk = __popcll(__ballot((kf & 3) == 3));
    if (first_lane) { atomicAdd(&misc[24], ne); if (ng) atomicAdd(&misc[25], ng); if (nk) atomicAdd(&misc[26], nk); }
}

// (round 5) One wavefront: no key array is built.  The kept flags of every slab of 64 lags are a ballot (kept in the team's
// LDS: nb_mode may ask for up to eight slabs) and the kept lags are compacted in place; the candidate slots are handed out
// by lane 0 and reach the other lanes through readfirstlane instead of an LDS word and a fence; a kept candidate finds its
// rank by walking the ballots - a scalar loop over the handful of kept lags, their dE read as LDS broadcasts - and only
// a dE tie looks at (value, lag).  (Rounds 1-4: packed keys in region A, three fences, two of them around a one-lane
// section - a quarter of the kernel's cycles for five candidates per region.)
// (slab_base, slab_left: the team's reserved candidate slots, uniform over the wavefront)
template <class G, class RA>
__device__ __forceinline__ void emit_wave(const Dev &d, const G &g, const RA &A, int shard, unsigned long long &slab_base, unsigned &slab_left, TeamStats &st)
{
    const int tid = g.tid, Kp = g.Kp;
    uint16_t *keep = g.keep;
    const int *dd = g.dd;
    const uint16_t *rk = g.rk;
    const double *keyv = A.keyv();
    int nkept = 0;
    unsigned long long *kbs = (unsigned long long *)&g.misc[8];      // [8] kept ballots by slab
    for (int base = 0; base < Kp; base += 64) {
        const int r = base + tid;
        const int kf = (r < Kp) ? keep[r] : 0;
        const unsigned long long bal = __ballot((kf & 1) != 0);
        if (g.T->lsb) count_guessed(g.misc, kf, tid == 0);
        if (tid == 0) kbs[base >> 6] = bal;
        // (the kept lags, compacted in place: one pass of the emit body below serves them all, whichever slab they came from;
        //  nkept + pre <= r - a flag that has not been read yet is never overwritten)
        if (kf & 1) keep[nkept + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u))] = (uint16_t)r;
        nkept += __popcll(bal);
    }
    st.count(g);
    unsigned long long cbase = 0;
    int ovf_i = 0;
    if (nkept) {
        unsigned long long b0 = 0;
        const bool fresh = (unsigned)nkept > slab_left;      // reserve a new slab of candidate slots (the rest of the old one is dropped)
        const unsigned want = cand_slab_want(d, nkept);
        if (fresh) {
            if (tid == 0) b0 = atomicAdd(&d.c->cand[shard].v, (unsigned long long)want);
            b0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(b0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)b0);
            if (b0 + want > d.cand_shard_cap) { if (tid == 0) atomicOr(&d.c->overflow, OVF_CAND); ovf_i = 1; slab_left = 0; }
            else { slab_base = (unsigned long long)shard * d.cand_shard_cap + b0; slab_left = want; }
        }
        if (!ovf_i) { cbase = slab_base; slab_base += nkept; slab_left -= nkept; }
    }
    wave_sync();                      // the ballots are in LDS
    if (nkept && !ovf_i)
        for (int x = tid; x < nkept; x += 64) {
            const int r = keep[x];
            const int my = dd[r];
            int rank = 0;
            for (int b2 = 0; b2 < Kp; b2 += 64) {
                const unsigned long long mv = kbs[b2 >> 6];
                unsigned long long mb = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(mv >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)mv);
                while (mb) {
                    const int y = b2 + __ffsll((long long)mb) - 1;
                    mb &= mb - 1;
                    const int dy = dd[y];
                    if (dy < my) rank++;
                    else if (dy == my && y != r) {               // dE tie: lag-rank order, i.e. (value desc, lag desc)
                        if (A.inplace) rank += y < r ? 1 : 0;    // (sorted in place: the index IS the lag's rank)
                        else {
                            const int lagq = rk[y], lagr = rk[r];
                            const double qv = keyv[lagq], myv = keyv[lagr];
                            rank += ((qv > myv) || (qv == myv && lagq > lagr)) ? 1 : 0;
                        }
                    }
                }
            }
            const int mi = g.wmi[r], mj = (int)rk[r] - mi, nb = g.wnb[r];
            emit_cand(d, g.brl, g.nbr, g.pos, mi, mj, nb, my, cbase + rank);
            if (g.dbg.kept) g.dbg.kept[rank] = r;
        }
    if (tid == 0) {
        d.nd[g.nid].cand = cbase;
        d.nd[g.nid].ncand = ovf_i ? 0 : nkept;
        if (g.dbg.n_ranked) g.dbg.n_ranked[1] = nkept;
    }
}

// Wider teams: the kept lags are compacted (keep[] becomes the list of their indices), thread 0 reserves the slots (slab_base,
// slab_left are its alone), and every kept candidate ranks its packed key - (dE biased to unsigned) << 32 | lag rank - among all
template <int NT, class G, class RA>
__device__ __forceinline__ void emit_team(const Dev &d, const G &g, const RA &A, int shard, unsigned long long &slab_base, unsigned &slab_left, TeamStats &st)
{
    const int tid = g.tid, Kp = g.Kp;
    uint16_t *keep = g.keep;
    int *misc = g.misc;
    const int *dd = g.dd;
    const uint16_t *rk = g.rk;
    const double *keyv = A.keyv();
    int nkept = 0;
    {
        int *wave_tot = misc + 16;
        const int lane = tid & 63, wv = tid >> 6;
        for (int base = 0; base < Kp; base += NT) {
            const int r = base + tid;
            const int kf = (r < Kp) ? keep[r] : 0;
            const int f = kf & 1;
            ESYNC();                      // everyone has read keep[] of this slab
            const unsigned long long bal = __ballot(f != 0);
            if (g.T->lsb) count_guessed(misc, kf, lane == 0);
            int pre = __popcll(bal & ((1ULL << lane) - 1));
            if (lane == 0) wave_tot[wv] = __popcll(bal);
            ESYNC();
            int tot = 0;
            for (int w = 0; w < NT / 64; w++) { if (w < wv) pre += wave_tot[w]; tot += wave_tot[w]; }
            if (f) keep[nkept + pre] = (uint16_t)r;   // nkept + pre <= r: never clobbers an unread flag
            nkept += tot;
            ESYNC();
        }
        ESYNC();
    }
    if (tid == 0) {
        unsigned long long base = 0;
        misc[2] = 0;
        if (nkept) {
            if ((unsigned)nkept > slab_left) {      // reserve a new slab of candidate slots (the rest of the old one is dropped)
                const unsigned want = cand_slab_want(d, nkept);
                unsigned long long b0 = atomicAdd(&d.c->cand[shard].v, (unsigned long long)want);
                if (b0 + want > d.cand_shard_cap) { atomicOr(&d.c->overflow, OVF_CAND); misc[2] = 1; slab_left = 0; }
                else { slab_base = (unsigned long long)shard * d.cand_shard_cap + b0; slab_left = want; }
            }
            if (!misc[2]) { base = slab_base; slab_base += nkept; slab_left -= nkept; }
        }
        *(unsigned long long *)&misc[4] = base;
        st.count(g);
    }
    ESYNC();
    const unsigned long long cbase = *(unsigned long long *)&misc[4];
    const bool ovf = misc[2] != 0;
    if (!ovf) {
        // (the packed keys take the place of the branch prefix sums in region A, which dE is done with: RegionA)
        unsigned long long *ck = A.sort_keys();
        for (int x = tid; x < nkept; x += NT) {
            const int r = keep[x];
            ck[x] = ((unsigned long long)((unsigned)dd[r] ^ 0x80000000u) << 32) | (unsigned)r;
        }
        ESYNC();
        for (int x = tid; x < nkept; x += NT) {
            const unsigned long long kx = ck[x];
            const int r = (int)(kx & 0xFFFFFFFFu);
            const int my = dd[r];
            int rank = 0;
            if (A.inplace) {                                 // r is the lag's rank
                for (int y = 0; y < nkept; y++) rank += ck[y] < kx ? 1 : 0;
            } else {                                         // rk[] is in no particular order: compare (value, lag)
                const int lagr = rk[r];
                const double myv = keyv[lagr];
                for (int y = 0; y < nkept; y++) {
                    const unsigned long long ky = ck[y];
                    if ((ky >> 32) == (kx >> 32)) {          // dE tie: (value desc, lag desc)
                        const int q = (int)(ky & 0xFFFFFFFFu), lagq = rk[q];
                        const double qv = keyv[lagq];
                        rank += (q != r && ((qv > myv) || (qv == myv && lagq > lagr))) ? 1 : 0;
                    } else
                        rank += ky < kx ? 1 : 0;
                }
            }
            const int mi = g.wmi[r], mj = (int)rk[r] - mi, nb = g.wnb[r];
            emit_cand(d, g.brl, g.nbr, g.pos, mi, mj, nb, my, cbase + rank);
            if (g.dbg.kept) g.dbg.kept[rank] = r;
        }
    }
    if (tid == 0) {
        d.nd[g.nid].cand = cbase;
        d.nd[g.nid].ncand = ovf ? 0 : nkept;
        if (g.dbg.n_ranked) g.dbg.n_ranked[1] = nkept;
    }
}

// LONGSEQ: 0 - the usual case: the bases of the loop are staged in LDS.
//          1 - sequences longer than 4096 nt: the bases are read from HBM/L2 (no room for them beside the FFT buffers).
//          2 - regions of more than 4096 positions (FFT size > 8192, whose two complex buffers exceed the LDS): the
//              correlation is the exact direct form on multi-word bit masks - popcount(base mask AND shifted reversed base
//              mask), the analogue of scipy's own direct branch (rafft/utils.py:121) - and the lag values live in a
//              per-workgroup scratch in HBM instead of LDS.  Same integer pair counts, same fp64 values, same ranking.
// PROD: the production build of a class without FFT buffers (no seam, no forced FFT, no negative weights): the debug-seam
// stores, the FFT and the cell-by-cell window_slide are compiled out - fewer live registers, fewer spills.
// PROD 2: the same for a class that keeps its FFT (regions beyond Dev::direct_n positions): only the seam, forced FFT and negative
//         weights go.
// PROD 3 (with LONGSEQ 2): the same kernel as the class for regions beyond 4096 positions, compiled for FOUR wavefronts per SIMD: it
//         serves the regions of 1025-4096 positions of ordinary sequences when the host routes them here (RAFFT_C3_DIRECT, class_cfg) -
//         ~50 KiB of LDS instead of the 150 KiB of the FFT plan, two or three workgroups per CU instead of one.
template <int NT, bool TAB_LDS, int WPB, int LONGSEQ = 0, int PROD = 0>
__global__ __launch_bounds__(NT * WPB, (NT == 64 ? (WPB == 16 ? 4 : RAFFT_EXPAND64_WAVES) : NT == 256 ? (PROD == 1 ? RAFFT_EXPAND256_PROD_WAVES : 3) : (PROD == 3 ? 4 : 2))) void expand_kernel(Dev d, int cls_arg, int Pmax, int Lmax, int nmax, int brmax, int Kmax)
{
    const int cls = cls_arg & 0xFF;
    const DebugOut dbg = PROD ? DebugOut{} : d.dbg;
    const int force_fft = PROD ? 0 : d.force_fft;

    static_assert(WPB == 1 || NT == 64, "only the one-wavefront class packs several wavefronts into a workgroup");
    static_assert(LONGSEQ == 0 || NT > 64, "long sequences never reach the one-wavefront class");
    extern __shared__ __align__(16) unsigned char lds_all[];
    const bool nofft = PROD == 1 || (cls_arg & 0x2000) != 0;   // the host promises: no seam, no forced FFT, no negative weights, every region within Dev::direct_n
    // (the class for regions beyond 4096 positions - 512 threads, lag values in HBM - keeps no LDS copy of the base codes: 32 768
    //  positions x 2 bytes are 64 KiB of its plan already; the FFT-free class for 1025-4096 positions, 256 threads, does)
    constexpr bool CODE_LDS = !(LONGSEQ == 2 && NT == 512);
    const ExpandLds lay = expand_lds(Pmax, Lmax, nmax, brmax, Kmax, TAB_LDS, WPB, nofft, NT, CODE_LDS);
    const int tid = threadIdx.x % NT;                 // position inside this region's team (a wavefront / the workgroup)
    const int team = threadIdx.x / NT;                // wavefront of the workgroup (0 when the workgroup is the team)
    const unsigned gteam = blockIdx.x * WPB + team, n_teams = gridDim.x * WPB;
    unsigned char *const lds = lds_all + team * lay.per_team;
    const SmallT *T = &d.T->s;
    const BigT *B = &d.T->b;
    const float2 *tw = d.tw;
    int twN = MAX_P;          // the twiddle table holds exp(-2 pi i m / twN), m < twN/2
    if (TAB_LDS) {            // persistent workgroup: hot energy tables and twiddles live in LDS, one copy per workgroup
        unsigned char *shared = lds_all + WPB * lay.per_team;
        int *dst = (int *)(shared + lay.off_tab);
        const int *src = (const int *)&d.T->s;
        for (int i = threadIdx.x; i < (int)(sizeof(SmallT) / 4); i += NT * WPB) dst[i] = src[i];
        T = (const SmallT *)dst;
        {   // (always, so that the compiler knows `tw` for an LDS pointer: a pointer that may be either makes every twiddle
            //  read a FLAT load, and a flat load waits for every global load in flight; the host keeps Pmax <= CLS2_P here)
            float2 *twl = (float2 *)(shared + lay.off_tw);
            if (!nofft) for (int m = threadIdx.x; m < Pmax / 2; m += NT * WPB) twl[m] = d.tw[m * (MAX_P / Pmax)];
            tw = twl;
            twN = Pmax;
        }
        __syncthreads();      // the only workgroup-wide barrier of the packed form
    }
    uint16_t *pos = (uint16_t *)(lds + lay.off_pos);
    uint8_t *code = lds + lay.off_code;
    uint32_t *P2 = (uint32_t *)(lds + lay.off_p2);      // the bases again, 2 bits per position (stem_stack_windows); only with CODE_LDS
    uint8_t *Sl_lds = lds + lay.off_S;
    uint32_t *brl = (uint32_t *)(lds + lay.off_br);
    uint16_t *rk = (uint16_t *)(lds + lay.off_rk);
    uint16_t *wnb = (uint16_t *)(lds + lay.off_nb);
    uint16_t *wmi = (uint16_t *)(lds + lay.off_mi);
    uint16_t *widx = (uint16_t *)(lds + lay.off_mj);    // the lags that gave a stem, compacted (the stem's mj is lag - mi: not stored)
    int *dd = (int *)(lds + lay.off_dd);
    uint16_t *keep = (uint16_t *)(lds + lay.off_keep);
    double *wtab = (double *)(lds + lay.off_w);
    int *misc = (int *)(lds + lay.off_misc);
    ExpandTeam tm;
    tm.tid = tid; tm.pos = pos; tm.code = code; tm.P2 = P2; tm.brl = brl; tm.rk = rk; tm.wnb = wnb; tm.wmi = wmi; tm.widx = widx;
    tm.dd = dd; tm.keep = keep; tm.wtab = wtab; tm.misc = misc; tm.T = T; tm.B = B; tm.dbg = dbg;

    if (!nofft && tid < 25) {      // (a class without FFT buffers has no such table: expand_lds)
        int a = tid / 5, b = tid % 5;
        int tp = pair_type(a, b);
        wtab[tid] = (tp == 5 || tp == 6) ? d.au : (tp == 1 || tp == 2) ? d.gc : (tp == 3 || tp == 4) ? d.gu : 0.0;
    }
    // an arena overflowed in an earlier kernel of this wave: the host regrows and folds the wave again, whatever is queued behind
    // that kernel (the rest of its step) finds records that were never written - and does nothing
    if (d.c->overflow) return;
    const unsigned n_items = d.c->n_work[cls].v;
    if (gteam == 0 && tid == 0) d.c->n_mat = 0;                // the beam step that follows counts its new structures here
    // (class 3 is served by two kernels on one work list: the list's length says which of them works - launch_expand_cls)
    if (((cls_arg & 0x4000) && n_items > (unsigned)d.c3_switch) || ((cls_arg & 0x8000) && n_items <= (unsigned)d.c3_switch)) return;
    const int shard = gteam & (NSHARD - 1);
    TeamStats st;               // this team's regions, their positions, lags and branches (counted by emit_*)
    if (tid < 3) misc[24 + tid] = 0;         // per team: stem energies evaluated / involving a rule or model value / kept ones that do

    // Work items are fetched FETCH at a time and candidate slots are reserved in slabs, so that the
    // two atomics with a returned value (a full L2 round trip each) are paid once per several regions.
    // (only when there is plenty of work: with fewer regions than workgroups every region gets its own)
    const unsigned FETCH = (NT == 64 && n_items > 4u * n_teams) ? (unsigned)d.fetch_bulk : 1u;
    const FetchPlan fplan = fetch_plan(d, n_items, NT == 64 ? FETCH : 1u, 1u);
    unsigned fetch_base = 0, fetch_left = 0;                 // uniform across the workgroup
    int fshard = (int)(gteam & (NSHARD - 1));                // work-cursor shard this team claims from next (fetch_chunk)
    unsigned long long ffailed = 0;
    unsigned long long slab_base = 0; unsigned slab_left = 0;   // reserved candidate slots (NT == 64: uniform over the wavefront; wider teams: thread 0 only)

    for (;;) {
        ESYNC();                       // previous region's LDS use is over
        if (fetch_left == 0) {
            unsigned fcount = 1;
            if (NT == 64) fetch_base = fetch_chunk(d, cls, fplan, fshard, ffailed, fcount);
            else {
                if (tid < 64) { const unsigned b_ = fetch_chunk(d, cls, fplan, fshard, ffailed, fcount); if (tid == 0) misc[8] = (int)b_; }
                ESYNC();
                fetch_base = (unsigned)misc[8];
            }
            if (fetch_base == ~0u) break;
            fetch_left = fcount;
        }
        // (the work item is the same for the whole team: saying so - readfirstlane - turns the header loads below into scalar
        //  loads, off the vector memory queue and out of the vector registers; only for the one-wavefront class, where a
        //  team IS a wavefront)
        const unsigned item = NT == 64 ? (unsigned)__builtin_amdgcn_readfirstlane((int)fetch_base) : fetch_base;
        fetch_base++; fetch_left--;
        if (item >= n_items) { fetch_left = 0; continue; }       // (tail of the list's last chunk; other shards may still hold chunks)
        const int nid = NT == 64 ? __builtin_amdgcn_readfirstlane(d.work[cls][item]) : d.work[cls][item];
        const int L = d.nd[nid].L;                 // (the record carries its sequence's length and offset: no look-up keyed on `seq`)
        const int n = d.nd[nid].n, ci = d.nd[nid].ci, cj = d.nd[nid].cj, nbr = d.nd[nid].nbr;
        const int par_dcal = d.nd[nid].pdcal;
        const uint16_t *posg = d.pos + d.nd[nid].pos;
        const uint32_t *brg = d.br + d.nd[nid].br;
        const uint8_t *codes = d.codes + d.nd[nid].soff;
        // (LDS copy of the bases: only the loop's span [sx0, sx1) is staged, at Sl_lds[x - sx0]; the pointer is shifted so
        //  that it still takes sequence positions - sx0 < 4096 never exceeds the offset of that area, the shifted pointer stays
        //  inside the LDS.  The address space is known at compile time either way.)
        const int sx0 = ci < 0 ? 0 : ci, sx1 = ci < 0 ? L : cj + 1;
        // (the copy goes four bases at a time, whole aligned words of the sequence: the LDS copy starts `spad` bytes in, so that it
        //  is aligned like its source; the 8 bytes of slack in front of and behind the area hold the up to three bases too many)
        const int spad = LONGSEQ ? 0 : (int)((uintptr_t)(codes + sx0) & 3u);
        const uint8_t *Sl = LONGSEQ ? codes : (const uint8_t *)Sl_lds + spad - sx0;
        const int m = 2 * n - 1;
        const int P = next_pow2_ge(m);
        const int logP = 31 - __clz(P);
        const int Pk = LONGSEQ == 2 ? 0 : P;       // the lag values occupy 8 P bytes of region A - unless they live in HBM
        const int Kp = d.K < m ? (d.K > 0 ? d.K : 0) : m;
        ExpandRegion<CODE_LDS> g{tm};
        g.nid = nid; g.n = n; g.m = m; g.P = P; g.logP = logP; g.Kp = Kp; g.nbr = nbr; g.ci = ci; g.cj = cj; g.L = L; g.par_dcal = par_dcal;
        g.codes = codes; g.Sl = Sl;

        load_region<NT, LONGSEQ>(d, g, posg, brg, Sl_lds, sx0, sx1, spad);

        // ---- correlation: conv(A,U), conv(G,C), conv(G,U), and the lag values from it.
        // Regions of <= 64 positions (one wavefront holds the whole strand in 64-bit masks) use the exact
        // direct form: popcount(mask & shifted reversed mask) per lag - the analogue of scipy's own
        // method="auto" picking direct convolution for short inputs (rafft/utils.py:121).  Longer regions
        // go through two packed complex FFTs in LDS.  Both give the same exact integer pair counts.
        const bool direct = (NT == 64) && n <= 64 && !force_fft;
        // The wide classes correlate regions of up to Dev::direct_n positions by the exact direct form on multi-word bit masks -
        // what the class for regions beyond 4096 positions always does - and longer ones by the FFT (rafft/utils.py:115-122:
        // scipy's convolve makes the same kind of choice); same integer pair counts either way.
        const bool mw = !direct && LONGSEQ != 2 && (nofft || (n <= d.direct_n && P >= 128 && dbg.lag == nullptr && !force_fft &&
                        d.gc >= 0.0 && d.au >= 0.0 && d.gu >= 0.0));
        // how the lags are ranked (select_lags, sort_lags_inplace): selected exactly, sorted in place (tiny FFT sizes, and the debug
        // seam, which reports the ranking), or - when 2n-1 <= nb_mode - not at all
        const bool ranked = m > Kp;
        const bool selected = ranked && P >= 128;
        const bool inplace = (ranked && !selected) || (dbg.lag != nullptr && !selected);    // keys sorted in place, rk[] in rank order
        const RegionA<LONGSEQ> A(lds, lay, P, Pk, n, nmax, selected, inplace, nofft, d, gteam);
        LagTally tally;
        if (LONGSEQ == 2 || mw) lag_values_masks<NT, PROD>(d, g, A, tally);
        else if (direct) lag_values_wave<NT, PROD>(d, g, A, tally);
        else {
            fft_correlate<NT>(g, A, tw, twN);
            lag_values_fft<NT, PROD>(d, g, A, tally);
        }

        // ---- ranking: rk[0..Kp) = the lags that are searched
        if (selected) {
            select_lags<NT, PROD>(g, A, tally);
            report_ranking<NT>(g, A);
        } else sort_lags_inplace<NT>(g, A);

        // ---- window_slide: the best stem of every searched lag (wnb, wmi), diagonals cut into C chunks in big regions.
        // The diagonal of a lag as bit masks: pairing cells per pair type (base masks AND shifted reversed base
        // masks, 64 cells per word), contiguity with the previous cell as a mask too.  Only the pairing cells
        // are visited - zero cells never change the result: same fp64 recurrence on the visited cells in the
        // same order, same `>=` rule.  A chunk first walks back over the run of pairing cells that ends just
        // before it and replays the recurrence over that run (zero cells reset it, so nothing older matters).
        // (Negative weights or the forced-FFT test mode take the cell-by-cell form.  The masks form stands here, not in a phase function:
        //  as a function it spills two more vector registers in the 256-thread production class - DESIGN.md 3.10.)
        const int C = (NT >= 256 && selected) ? max(1, min(8, NT / max(Kp, 1))) : 1;
        const bool ws_masks = PROD || (d.gc >= 0.0 && d.au >= 0.0 && d.gu >= 0.0 && !force_fft);
        if (ws_masks) {
            const int W = A.W();
            // forward masks F[0..3] = A,C,G,U, F[4] = contiguity with the previous position; R[] = reversed strings (build_masks)
            unsigned long long *F = A.slide_masks(), *R = F + MASK_F_WORDS * W;
            WsPart *parts = A.slide_parts();
            if (LONGSEQ != 2 && (!mw || A.inplace)) {   // (the direct correlation on multi-word masks has built them already - behind the lag values)
                build_masks<NT>(F, R, W, n, [&](int t) -> int { return g.code_at(t); }, pos, tid);
                ESYNC();
            }
            // (round 5) The cells of a diagonal are taken 32 at a time, counted from the diagonal's FIRST cell: chunk k holds the cells
            // ip0 + 32 k .. of the forward strings and - the reversed strings all being read at bit n - 1 - lag + ip - the bits
            // n - 1 - lag + ip0 + 32 k .. of the reversed ones; a window of 32 bits at any bit offset is two adjacent words and one
            // v_alignbit.  Half a diagonal of a region of up to 64 positions is ONE chunk, and the loop over its pairing cells runs on
            // 32-bit masks (rounds 1-4: 64-bit words aligned to the region, 64-bit shifts and tests per cell, windows assembled from
            // range-checked loads: 38 % of the kernel's vector instructions, tools/pmc_phases.sh).  Bits read past a string's end are
            // cells past the half-diagonal's eligible prefix: masked.
            const uint32_t *F32 = (const uint32_t *)F, *R32 = (const uint32_t *)R;
            const int W2 = 2 * W;
            // (the three pair weights in vector registers of their own: a select between two scalar operands is not encodable, and
            //  the compiler would rather copy them into vector registers again for every cell of the loop below - 6 of its 42 instructions)
            double wgc = d.gc, wau = d.au, wgu = d.gu;
            asm volatile("" : "+v"(wgc), "+v"(wau), "+v"(wgu));
            auto win = [](const uint32_t *X, int start) -> uint32_t { const int q_ = start >> 5; return __builtin_amdgcn_alignbit(X[q_ + 1], X[q_], (uint32_t)(start & 31)); };
            for (int q = tid; q < Kp * C; q += NT) {
                const int r = q / C, c = q - r * C;
                const int lagp = rk[r];
                const Diag dg = diag_of(lagp, n);
                const int ip0 = dg.ip0;
                const int lim = eligible_prefix(pos, dg.len, dg.len2, ip0, dg.jp0, d.min_hp);
                // this lane's share of the eligible cells [ca, ce), counted from the diagonal's first cell
                const int ca = (int)((long long)lim * c / C), ce = (int)((long long)lim * (c + 1) / C);
                const int rs0 = n - 1 - lagp + ip0;          // bit of the reversed strings that belongs to the first cell (>= 0)
                // pairing cells of chunk k by pair type, and the cells contiguous with their predecessor
                auto cells = [&](int k, uint32_t &pGC, uint32_t &pAU, uint32_t &pGU, uint32_t &cm) {
                    const int cs = ip0 + 32 * k, rs = rs0 + 32 * k;
                    const uint32_t fA = win(F32 + 0 * W2, cs), fC = win(F32 + 1 * W2, cs), fG = win(F32 + 2 * W2, cs), fU = win(F32 + 3 * W2, cs);
                    const uint32_t xA = win(R32 + 0 * W2, rs), xC = win(R32 + 1 * W2, rs), xG = win(R32 + 2 * W2, rs), xU = win(R32 + 3 * W2, rs);
                    pGC = d.gc != 0.0 ? ((fG & xC) | (fC & xG)) : 0u;
                    pAU = d.au != 0.0 ? ((fA & xU) | (fU & xA)) : 0u;
                    pGU = d.gu != 0.0 ? ((fG & xU) | (fU & xG)) : 0u;
                    cm = win(F32 + 4 * W2, cs) & win(R32 + 4 * W2, rs);       // contiguous with the previous cell on both strands
                    if (k == 0) cm &= ~1u;                                    // never for the first cell
                };
                auto span = [](int lo_, int hi_, int cb) -> uint32_t {                       // bits of cells [lo_, hi_) inside the chunk that starts at cell cb
                    uint32_t m_ = ~0u;
                    if (lo_ > cb) m_ &= ~0u << (lo_ - cb);
                    if (hi_ < cb + 32) m_ &= (1u << (hi_ - cb)) - 1u;
                    return m_;
                };
                double mx_s = 0.0, prev = 0.0;
                int mx_nb = 0, mx_c = 0, last_c = -2, runlen = 0, mx_i = 0, mx_j = 0;
                if (ce > ca) {
                    int z = ca;                              // replay start: first cell of the run of pairing cells ending at ca - 1
                    if (ca > 0) {
                        for (int kz = (ca - 1) >> 5;; kz--) {
                            const int cb = kz << 5;
                            uint32_t pGC, pAU, pGU, cm;
                            cells(kz, pGC, pAU, pGU, cm);
                            const uint32_t zeros = ~(pGC | pAU | pGU) & span(0, ca, cb);
                            if (zeros) { z = cb + 32 - __clz((int)zeros); break; }
                            if (cb == 0) { z = 0; break; }
                        }
                    }
                    for (int k = z >> 5; k <= (ce - 1) >> 5; k++) {
                        const int cb = k << 5;
                        uint32_t pGC, pAU, pGU, cm;
                        cells(k, pGC, pAU, pGU, cm);
                        uint32_t any = (pGC | pAU | pGU) & span(z, ce, cb);
                        while (any) {
                            const int bi = __ffs((int)any) - 1;
                            any &= any - 1u;
                            const int cc = cb + bi;
                            const double w8 = ((pGC >> bi) & 1u) ? wgc : ((pAU >> bi) & 1u) ? wau : wgu;
                            if (cc != last_c + 1) { prev = 0.0; runlen = 0; }   // previous cell was a zero cell
                            double t = w8;
                            if ((cm >> bi) & 1u) t = (prev + w8) * w8;
                            runlen++;
                            if ((C == 1 || cc >= ca) && t >= mx_s) { mx_s = t; mx_nb = runlen; mx_c = cc; }
                            prev = t; last_c = cc;
                        }
                    }
                    if (mx_nb == 0) mx_c = ce - 1;           // no pairing cell in the share: its last eligible (zero) cell, nb = 0
                    mx_i = ip0 + mx_c; mx_j = lagp - mx_i;
                }
                if (C == 1) store_slide(g, r, mx_nb, mx_i, mx_j, mx_s);
                else { WsPart wp; wp.score = mx_s; wp.nb = mx_nb; wp.mi = mx_i; wp.mj = mx_j; wp.any = ce > ca ? 1 : 0; parts[q] = wp; }
            }
            if (C > 1) merge_slide_parts<NT>(g, parts, C);
        } else window_slide_cells<NT>(d, g, A, C);
        ESYNC();

        // ---- dE of every candidate stem (dd, keep), then the kept ones in stable dE order into the candidate arena
        const BrPrefix pf = branch_prefix_sums<NT>(g, A);
        stems_dE<NT>(d, g, pf);
        if constexpr (NT == 64) emit_wave(d, g, A, shard, slab_base, slab_left, st);
        else emit_team<NT>(d, g, A, shard, slab_base, slab_left, st);
    }
    if (tid == 0 && st.items) {
        Counters::StatLine *sl = &d.c->xstat[cls][gteam & (NSHARD - 1)];
        flush_stats(sl, st.items, st.n, st.lags, st.nbr);
    }
    if (tid == 0 && misc[24]) {
        Counters::StatLine *sl = &d.c->xstat[cls][gteam & (NSHARD - 1)];
        flush_guess_stats(sl, misc[24], misc[25], misc[26]);
    }
}
