// rafft_plan.h - what a wave needs before it runs: the size classes of the expand kernel with their LDS plans and launches,
// and the HBM arenas of a job (plan_job: the one plan that both Wave::setup and the scheduler's admission test use).
// Part of the single translation unit of rafft_api.hip (included there, after rafft_host_ctx.h).
#pragma once

namespace {

struct ClsCfg { int nt, Pmax, Lmax, nmax, brmax, Kmax, lds, grid; int wpb; bool nofft; bool direct3 = false; };   // grid: teams (wavefronts of the packed one-wavefront class, workgroups otherwise)

// limits of the one-wavefront class: its LDS per wavefront (hence its occupancy) follows from them
// (not below 256: the kernel addresses the staged bases through a pointer shifted back by up to 4095 positions, which must stay
//  inside the LDS - the 16 * P bytes in front of that area see to it)
static int cls1_P(const Config &cfg) { return std::max(256, std::min(next_pow2_ge(cfg.cls1_p), CLS1_P)); }
static int cls1_br(const Config &cfg) { return std::min(CLS1_BR, (8 * cls1_P(cfg) - 16) / 10 - 1); }

// `nofft1`: the one-wavefront class correlates every region by popcounts (production mode: no seam, no forced FFT, no negative
// weights, Dev::direct_n >= 256): its FFT buffers and twiddles go, its branch lists shrink to 128 entries, and a workgroup of twelve
// wavefronts leaves ~32 KiB of a CU's LDS - room for a workgroup of the small-region kernel beside it.
// `nofft2`: the same for the 256-thread class when Dev::direct_n covers all of its regions (<= 1024 positions): 46 -> 39 KiB, four
// workgroups per CU instead of three.
int class_cfg(const Config &cfg, int K, int maxL, ClsCfg out[NGEN + 1], bool nofft1 = false, bool nofft2 = false, bool direct3_ok = false)
{
    // sequences longer than LDS_SEQ: classes 2 and 3 read the bases of a loop from HBM/L2 (no LDS copy), class 0 takes the
    // regions beyond 4096 positions, whose FFT would not fit (node_class)
    const bool longseq = maxL > LDS_SEQ;
    const int P[NGEN] = {CLS0_P, cls1_P(cfg), CLS2_P, MAX_P}, LM[NGEN] = {0, CLS01_L, longseq ? 0 : LDS_SEQ, longseq ? 0 : LDS_SEQ};
    const int NT[NGEN] = {512, 64, 256, 512}, BR[NGEN] = {BIG_BR + 1, nofft1 ? 128 : cls1_br(cfg), MAX_BR, MAX_BR};
    // The one-wavefront class packs 12 wavefronts - what a CU holds of them anyway - into one workgroup that shares ONE LDS
    // copy of the energy tables and twiddles: the table look-ups of the dE phase stop being dependent L2 round trips
    // (measured: 5.9 -> 5.4 ms per benchmark batch in this kernel; with 4 or 8 per workgroup a CU holds fewer wavefronts
    // and loses more than it gains); sixteen without FFT buffers.  Falls back to twelve, then to one wavefront per workgroup,
    // tables in L2, when nb_mode makes the per-wavefront arrays too big to fit.
    int wpb1 = nofft1 ? 16 : 12;
    {
        const int Kmax1 = std::max(1, std::min(K, cls1_P(cfg) - 1));
        if (wpb1 == 16 && expand_lds(cls1_P(cfg), CLS01_L, cls1_P(cfg) / 2, BR[1], Kmax1, true, wpb1, nofft1, 64).total > 160 * 1024) wpb1 = 12;
        if (expand_lds(cls1_P(cfg), CLS01_L, cls1_P(cfg) / 2, BR[1], Kmax1, true, wpb1, nofft1, 64).total > 160 * 1024) wpb1 = 1;
    }
    const int WPB[NGEN] = {1, wpb1, 1, 1};
    const bool TAB[NGEN] = {false, WPB[1] > 1, false, false};    // energy tables in LDS: one copy shared by the wavefronts of a packed workgroup
    for (int c = 0; c < NGEN; c++) {
        // (class 0 is planned for 16 384 positions unless a sequence of the wave is longer: the 64 KiB of 32 768 positions leave
        //  its scratch room for nb_mode <= 106 only, where the plan for 16 384 takes ~400)
        const int big_n = maxL > 16384 ? BIG_N : 16384;
        int nmax = c == 0 ? big_n : P[c] / 2;
        int Kmax = std::max(1, std::min(K, c == 0 ? 2 * big_n - 1 : P[c] - 1));
        const bool nf = (c == 1 && nofft1 && WPB[1] > 1) || (c == 2 && nofft2);
        ExpandLds l = expand_lds(P[c], LM[c], nmax, BR[c], Kmax, TAB[c], WPB[c], nf, NT[c], c != 0);      // (class 0: no LDS copy of the base codes - expand_kernel's CODE_LDS)
        // region A is time-shared (its tenants, their offsets and sizes: the table above RegionA in rafft_expand.hip, which these
        // checks bound per class): behind the fp64 lag values (8 P bytes) it must still hold the branch prefix sums
        // (10 bytes per branch), the select histogram and the window_slide scratch of this class
        // (the partial results of chunked diagonals: C chunks per ranked lag, C = min(8, NT / lags) - 512 records of 24 bytes
        //  at the most until there are more lags than threads, not 8 per lag: that bound refused nb_mode 214-399 on sequences
        //  of 4097-16384 nt, which the message below and DESIGN.md 5 promise - tests/test_gpu_ties.py asks for 399 at 4097 nt.
        //  The plan for 32 768 positions keeps the bound of 8 per lag it has been tested with: nb_mode <= 106.)
        const int ws_parts = maxL > 16384 ? 8 * std::max(Kmax, 1) : std::max(std::min(8 * std::max(Kmax, 1), NT[c]), Kmax);
        if (c == 0 && longseq && (8 * MASK_WORDS * (big_n / 64) + 24 * ws_parts + 4096 > 16 * P[c] || 10 * (BR[c] + 1) + 16 + 24 * Kmax + 2048 > 16 * P[c]))
            return fail(RAFFT_ERR_PARAM, std::string("nb_mode too large for the LDS scratch of the class for regions beyond 4096 positions: with a sequence of ") +
                                         (maxL > 16384 ? "more than 16384 nt it must stay at or below 106" : "more than 4096 nt it must stay below ~400") +
                                         " (this wave: nb_mode " + std::to_string(K) + ", longest sequence " + std::to_string(maxL) + " nt)");
        if (c >= 1 && (10 * (BR[c] + 1) + 16 > 8 * P[c] || 2 * P[c] + 1152 + 16 > 8 * P[c] || (NT[c] > 64 && NT[c] * 24 > 8 * P[c])))
            return fail(RAFFT_ERR_PARAM, "internal: expand LDS plan does not fit its size class");
        if (c >= 1 && LM[c] > 0 && l.off_S < LDS_SEQ)      // (expand_kernel's Sl: the staged bases are addressed by sequence position)
            return fail(RAFFT_ERR_PARAM, "internal: the LDS copy of the bases sits too low for its shifted pointer");
        const int per_cu = std::max(1, std::min(32 / (NT[c] / 64), WPB[c] * ((160 * 1024) / l.total)));      // teams per CU
        out[c] = {NT[c], P[c], LM[c], nmax, BR[c], Kmax, l.total, g.n_cu * per_cu, WPB[c], nf};
        // a size class that no region of this batch can reach need not fit (class 3 needs n > 1024, class 0 n > 4096)
        const bool reachable = c == 0 ? longseq : (c < 3 || maxL > CLS2_P / 2);
        if (l.total > 160 * 1024 && reachable)
            return fail(RAFFT_ERR_PARAM, "nb_mode too large for the LDS-resident expand kernel: it must stay below 2048 (below ~400 when a "
                                         "sequence is longer than 4096 nt)");
        if (l.total > 160 * 1024) out[c].lds = 160 * 1024, out[c].Kmax = 1;    // never launched with work
    }
    // Regions of 1025-4096 positions (class 3) without the 128-KiB FFT buffers: the kernel of the class for regions beyond 4096
    // positions - exact direct correlation on multi-word bit masks, lag values in a per-workgroup HBM scratch - with an LDS plan
    // sized for 4096 positions: ~50 KiB, so a CU holds two or three workgroups of it (four wavefronts per SIMD) instead of one.
    // Same integer pair counts, same fp64 values (tests/test_gpu_parity.py::test_gpu_fft_and_direct_correlation_agree).
    // (measured on the configs[3] shard: 202 -> 177 ms per call, the class itself 93 -> 66 ms - its regions cost 330 kcycles each at
    //  three workgroups per CU against 182 at one; the benchmark set, whose two 23S sequences are all it has of such regions, is
    //  unchanged.  RAFFT_C3_DIRECT=0: the FFT plan; read at every call, tests switch it.)
    const int c3_direct = cfg.c3_direct;
    if (c3_direct && direct3_ok && !longseq) {
        const int Kmax = std::max(1, std::min(K, MAX_P - 1)), nmax = MAX_P / 2, Pd = 2048;
        // (256 threads: at the 168 VGPRs the kernel needs without spilling a SIMD holds three wavefronts - three 256-thread
        //  workgroups per CU; a 512-thread workgroup is two wavefronts per SIMD, and two of those would need 128 VGPRs: 44 spilled)
        const int Cc = std::max(1, std::min(8, 256 / std::max(Kmax, 1)));
        // (the tenants of region A with the lag values in HBM: RegionA's table, rafft_expand.hip)
        const bool fits = 8 * MASK_WORDS * (nmax / 64) + 24 * Cc * Kmax + 2048 + 64 <= 16 * Pd && 10 * (MAX_BR + 1) + 16 + 8 * Kmax + 2048 <= 16 * Pd;
        ExpandLds l = expand_lds(Pd, 0, nmax, MAX_BR, Kmax, false, 1, false, 256);
        if (fits && l.total <= 80 * 1024) {
            const int per_cu = std::max(1, std::min(3, (160 * 1024) / l.total));
            out[NGEN] = out[3];          // the FFT plan stays for the steps with few such regions (launch_expand_cls)
            out[3] = {256, Pd, 0, nmax, MAX_BR, Kmax, l.total, g.n_cu * per_cu, 1, false, true};
        }
    }
    return 0;
}

template <int NT, bool TAB, int WPB = 1, int LONGSEQ = 0, int PROD = 0>
int launch_expand(const Dev &d, int cls, const ClsCfg &cf, unsigned n_teams, hipStream_t st)
{
    static int lds_set = 0;
    if (cf.lds > lds_set) {
        HIPCHK(hipFuncSetAttribute((const void *)expand_kernel<NT, TAB, WPB, LONGSEQ, PROD>, hipFuncAttributeMaxDynamicSharedMemorySize, cf.lds));
        lds_set = cf.lds;
    }
    const unsigned n_blocks = (n_teams + WPB - 1) / WPB;
    hipLaunchKernelGGL((expand_kernel<NT, TAB, WPB, LONGSEQ, PROD>), dim3(n_blocks), dim3(NT * WPB), cf.lds, st, d, cls, cf.Pmax, cf.Lmax, cf.nmax, cf.brmax, cf.Kmax);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_expand_cls(const Config &cfg, const Dev &d, int cls, const ClsCfg cf[NGEN + 1], unsigned n_blocks, hipStream_t st)
{
    // the production builds: no diagnostics of any kind asked for (RAFFT_PROD=0: the general builds)
    const bool prod_ok = cfg.prod != 0;
    if (cls >= NGEN) {        // small regions: teams of 16 / 32 lanes, four wavefronts per workgroup (n_blocks = workgroups)
        const bool prod = prod_ok && d.dbg.lag == nullptr;
        if (cls == 4 && prod) hipLaunchKernelGGL((expand_small_kernel<16, true>), dim3(n_blocks), dim3(64 * SM_WG_WAVES), small_lds_bytes<16>(), st, d, cls);
        else if (cls == 4) hipLaunchKernelGGL((expand_small_kernel<16, false>), dim3(n_blocks), dim3(64 * SM_WG_WAVES), small_lds_bytes<16>(), st, d, cls);
        else if (prod) hipLaunchKernelGGL((expand_small_kernel<32, true>), dim3(n_blocks), dim3(64 * SM_WG_WAVES), small_lds_bytes<32>(), st, d, cls);
        else hipLaunchKernelGGL((expand_small_kernel<32, false>), dim3(n_blocks), dim3(64 * SM_WG_WAVES), small_lds_bytes<32>(), st, d, cls);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const bool longseq = cf[2].Lmax == 0;          // (class_cfg: no LDS copy of the bases)
    const int nf = cf[cls].nofft ? 0x2000 : 0;
    const bool nodiag = prod_ok && d.dbg.lag == nullptr && !d.force_fft && d.gc >= 0.0 && d.au >= 0.0 && d.gu >= 0.0;
    const bool prod = nodiag && nf;                // (the classes without FFT buffers)
    if (cls == 0) return nodiag ? launch_expand<512, false, 1, 2, 2>(d, 0, cf[0], n_blocks, st) : launch_expand<512, false, 1, 2>(d, 0, cf[0], n_blocks, st);
    if (longseq && cls == 2) return prod ? launch_expand<256, false, 1, 1, 1>(d, 2 | nf, cf[2], n_blocks, st) : launch_expand<256, false, 1, 1>(d, 2 | nf, cf[2], n_blocks, st);
    if (longseq && cls == 3) return nodiag && !nf ? launch_expand<512, false, 1, 1, 2>(d, 3, cf[3], n_blocks, st) : launch_expand<512, false, 1, 1>(d, 3 | nf, cf[3], n_blocks, st);
    if (cls == 1) {                                // (class_cfg: the energy tables are in LDS exactly when wavefronts are packed)
        if (cf[1].wpb == 16 && prod) return launch_expand<64, true, 16, 0, 1>(d, 1 | nf, cf[1], n_blocks, st);
        if (cf[1].wpb == 16) return launch_expand<64, true, 16>(d, 1 | nf, cf[1], n_blocks, st);
        if (cf[1].wpb == 12) return launch_expand<64, true, 12>(d, 1 | nf, cf[1], n_blocks, st);
        return launch_expand<64, false>(d, 1, cf[1], n_blocks, st);
    }
    if (cls == 2) return prod ? launch_expand<256, false, 1, 0, 1>(d, 2 | nf, cf[2], n_blocks, st) : launch_expand<256, false>(d, 2 | nf, cf[2], n_blocks, st);
    if (cf[3].direct3) {
        // Two kernels share the class's work list; the length of the list decides ON THE DEVICE which of them works (the other one's
        // workgroups leave at once): up to Dev::c3_switch regions - every region has a CU to itself either way - the FFT plan, whose
        // region takes 76 us (182 kcycles) against 137 us without the FFT buffers; beyond that the FFT-free kernel, three workgroups
        // per CU.  (With the FFT-free kernel alone one synchronous call on the benchmark batch took 11.5 ms instead of 10.0: its
        // long-tail wave expands a handful of such regions per step, 24 steps in a row.)
        if (int rc = nodiag ? launch_expand<256, false, 1, 2, 3>(d, 3 | 0x8000, cf[3], n_blocks, st) : launch_expand<256, false, 1, 2>(d, 3 | 0x8000, cf[3], n_blocks, st)) return rc;
        const unsigned nb_fft = std::min<unsigned>(n_blocks, (unsigned)cf[NGEN].grid);
        return nodiag ? launch_expand<512, false, 1, 0, 2>(d, 3 | 0x4000, cf[NGEN], nb_fft, st) : launch_expand<512, false>(d, 3 | 0x4000, cf[NGEN], nb_fft, st);
    }
    return nodiag ? launch_expand<512, false, 1, 0, 2>(d, 3, cf[3], n_blocks, st) : launch_expand<512, false>(d, 3, cf[3], n_blocks, st);
}

struct Caps {
    size_t st, nd, pos, br, sp, cand, seen, trec, tsid, work, mat, looptab;
    int ch_cap, sort_cap;
    size_t bytes;
    bool capped;      // a table hit the limit of its 31-bit ids: the job is folded in halves when it has more than one sequence
};

// Initial slots of a sequence's `seen` set (round 5).  A set that outgrows its table is rehashed into one of twice the size inside
// beam_step_kernel - ~100 us of ONE workgroup (dependent compare-and-swap round trips), i.e. of the whole launch when it is the
// slowest: on the benchmark set every sequence beyond 200 nt grew once or twice (RAFFT_TRACE=2 prints the fill by length) and a
// fixed 65 536 slots took a sixth off both beam-step kernels.  Sized from the length instead: the upper envelope of the entries at
// the end of a fold (measured at max_stack 50, max_branch 1000: 1.9 k at 80 nt, 3.3 k at 130, 5.5 k at 300, 7.6 k at 500, 8.8 k at
// 1000, 20 k at 3000), scaled by the children a step accepts, for a table that is at most half full (the kernel's own growth rule).
// A set that still outgrows it grows as before.
static uint32_t seen_slots0(int L, const rafft_params &p, const Config &cfg)
{
    if (cfg.seen_fixed) return SEEN0;
    const double l = (double)L;
    const double e = l <= 130 ? 26.0 * l : l <= 300 ? 3380.0 + 13.0 * (l - 130) : l <= 500 ? 5590.0 + 10.5 * (l - 300) : l <= 1000 ? 7690.0 + 2.4 * (l - 500) : 8890.0 + 5.6 * (l - 1000);
    const double per_step = p.max_branch > 0 ? std::min((double)p.max_branch, 8.2 * (double)p.max_stack) : (double)p.max_stack;
    const double need = 2.0 * (e * std::max(per_step / 410.0, 0.1) + 384.0);
    uint32_t cap = 2048;
    while ((double)cap < need && cap < (1u << 22)) cap <<= 1;
    return cap;
}
// ... for a wave: per-sequence slots with the big tables halved until the initial tables fit `budget_slots` (the growth path does the rest)
static size_t seen_slots0_wave(const int *len, size_t S, const rafft_params &p, const Config &cfg, size_t budget_slots, uint32_t *out)
{
    uint32_t limit = 1u << 22;
    for (;;) {
        size_t tot = 0;
        for (size_t i = 0; i < S; i++) { const uint32_t c = std::min(seen_slots0(len[i], p, cfg), limit); if (out) out[i] = c; tot += c; }
        if (tot <= budget_slots || limit <= SEEN0) return tot;
        limit >>= 1;
    }
}
#define SEEN0_BUDGET ((size_t)192 << 20)        // slots: 3 GB of initial tables per wave at most

Caps plan_caps(const Config &cfg, size_t S, size_t sumL, const rafft_params &p, double est, double seen0_per_seq)
{
    // Arena sizes from measured usage on the BASELINE workloads (benchmark set, L 28..2968, ms 50;
    // random L 100..3000, ms 200): per surviving structure about 2 + L/100 regions, 0.6 L region
    // positions, one branch per region, ~5 candidates per region, the pairs a structure adds to its parent's
    // (one stem in every productive region - measured on L 100..3000: 30 pairs per structure, 0.02 L; structures of
    // long sequences are over-represented: they fold for more steps).  Factors below carry ~1.5x slack;
    // an overflow is detected on the device and the wave is re-run with doubled arenas.
    Caps c;
    const size_t B = (size_t)p.max_stack;
    double avgL = S ? (double)sumL / (double)S : 1.0;
    double nstruct = (double)S * (1.0 + (double)B * est);
    c.st = (size_t)std::min(nstruct, 2.0e9) + 64;
    double nodes_per = avgL / 60.0 + 4.0;
    c.nd = (size_t)std::min((double)c.st * nodes_per, 2.0e9) + 64;
    c.capped = nstruct > 2.0e9 || (double)c.st * nodes_per > 2.0e9;
    c.pos = (size_t)((double)sumL + (double)(c.st - S) * avgL * 0.9) + 4096;
    c.br = c.nd * 3 + 4096;
    c.sp = (size_t)((double)(c.st - S) * (avgL * 0.05 + 24.0)) + 4096;
    c.cand = c.nd * (size_t)std::min(std::max(p.nb_mode, 1), 8) + 4096;
    // (with memoization a region is created once per wave, whoever picks the stem that makes it: what a structure adds to the candidate
    //  table stops growing with the regions it HAS.  Measured, tools/arena_probe.py, candidates per structure: 10-20 on the benchmark
    //  set, 200-nt and 40-nt random sequences, ms 50 and 400; 15 on L 100..3000 at ms 200 - where the line above plans 238 -; 46 at
    //  ms 1; 50 on G/C-only sequences of 600 nt; 59 and 95 on 2.9-knt and 8-knt sequences at ms 50 and 20)
    const bool memo_on = p.min_nrj == 0.0 && !cfg.no_memo;
    if (memo_on) c.cand = std::min(c.cand, (size_t)((double)c.st * (60.0 + avgL / 40.0)) + 4096);
    c.cand = std::max<size_t>(c.cand, (size_t)NSHARD * 16384);
    // (a child slot is named by 2 x candidate + side in 31 bits - the node lists hold -(slot + 1), rafft_kernels.h - so a wave has
    //  at most 2^30 candidate records; round 4's structure rows used to keep the byte budget of a wave below that by themselves)
    size_t cand_limit = ((size_t)1 << 30) - 4096;
    if (cfg.test_cand_limit > 0) cand_limit = std::min<size_t>(cand_limit, std::max<size_t>((size_t)cfg.test_cand_limit, (size_t)NSHARD * 16384));   // (tests: the split path on small jobs)
    if (c.cand > cand_limit) { c.cand = cand_limit; c.capped = true; }
    // accepted children per sequence ~ steps * min(max_branch, ...); regions double and old ones are dropped
    // (measured, ms 50, max_branch 1000, regions abandoned by rehashing included: the benchmark set's bulk uses 4.6 x est x
    //  (B + max_branch / 4) slots per sequence, its two 2.9-knt sequences 11.6 x.  A factor of 24 used to reserve 1 MB per
    //  sequence - 12 GB for a merged wave of five batches, and a hipMalloc of that size now and then took seconds.)
    // (round 5: the initial tables are sized from the lengths - seen_slots0 - and a table rarely grows any more: the reserve for growth
    //  went from 14 x to 5 x est x (B + max_branch / 4), at least as much again as the initial tables.  At 14 x the arena was 10.6 GB of
    //  a merge-cap plan of 33.7 GB - above the tenth of the HBM up to which a first wave reserves its workspace for the merge cap, so
    //  every bigger wave of a stream re-allocated two dozen buffers; at 5 x the plan is 28.5 GB and the first wave's workspace holds them all.)
    double per_seq_seen = std::min(std::max(std::max(5.0 * est * ((double)B + (double)p.max_branch / 4.0), seen0_per_seq), 16384.0), 16777216.0);
    // (a floor of 4 M slots - 64 MB - whatever the batch: a few long sequences among sixty short ones double their tables twice)
    c.seen = (size_t)((double)S * seen0_per_seq) + std::max((size_t)((double)S * per_seq_seen), (size_t)4 << 20);
    c.trec = p.traj ? S * (size_t)(est * 3 + 16) : S + 16;
    c.tsid = c.trec * B + 16;
    c.mat = S * B + 16;
    // every arena is split into NSHARD sub-arenas: keep a floor per shard so that small batches,
    // whose few structures land on few shards, do not overflow a starved shard
    c.nd = std::max<size_t>(c.nd, S + (size_t)NSHARD * 2048);
    c.pos = std::max<size_t>(c.pos, sumL + (size_t)NSHARD * (16 * (size_t)avgL + 4096));
    c.sp = std::max<size_t>(c.sp, (size_t)NSHARD * (2 * (size_t)avgL + 4096));
    c.br = std::max<size_t>(c.br, (size_t)NSHARD * 8192);
    c.work = c.nd;
    // (the loop table holds the regions CREATED - one per child slot that a beam member picked, ~0.4 of the (structure, region) pairs
    //  `nd` is planned for: a power of two >= nd keeps it at most half full; it is zero-filled for every wave, and a full table is an
    //  overflow like any other - the wave is folded again with doubled arenas)
    c.looptab = 1024; while (c.looptab < c.nd) c.looptab <<= 1;
    c.ch_cap = p.max_branch + p.max_stack + 8;
    int need = p.max_branch + 2 * p.max_stack + 8;
    // keys of one step: children + old beam; only the max_stack selected ones are sorted (padded to a power of two)
    int m2 = 2; while (m2 < p.max_stack) m2 <<= 1;
    c.sort_cap = std::max((need + 1) & ~1, m2);
    c.bytes = c.st * 128 + c.nd * (64 + 4 + 4 + 6 * 4 + 16) + c.pos * 2 + c.br * 4 + c.sp * 4 + c.cand * (32 + 8) + c.seen * 16 + c.seen / 8 /* occupancy bitmaps */ +
              c.looptab * 8 + c.trec * 16 + c.tsid * 4 + c.mat * 48 + S * (size_t)c.ch_cap * 32 + S * B * 4;
    return c;
}

// sequences one merged wave may hold (a wave of the whole benchmark set four times over folds 25 % faster per sequence
// than the set alone: fewer, fuller launches; five times over - with ten batches in flight, so that two such waves run side by
// side - another 4 % in round 3: 288 k sequences/s against 277-282 k over 30 steps; seven times over, three such waves side by side,
// 432-444 k -> 461-464 k in round 4, tools/ab_waves2.sh; beyond that the arenas of a wave pass a tenth of the HBM, where waves run
// one at a time)
static size_t merge_cap()
{
    return (size_t)std::max(1, g.sched_cfg.merge_seqs);
}

// The HBM plan of a job: the initial `seen` tables of its sequences and the arenas sized from them.  Wave::setup allocates by it, the
// scheduler's admission test asks it whether the job fits.
struct JobPlan { Caps caps; std::vector<uint32_t> seen_cap0; size_t seen0_total; double seen0_avg; };
JobPlan plan_job(const Config &cfg, const rafft_params &p, const std::vector<SeqIn> &seqs, double est)
{
    JobPlan jp;
    const size_t S = seqs.size();
    std::vector<int> len(S);
    size_t sumL = 0;
    for (size_t i = 0; i < S; i++) { len[i] = seqs[i].len; sumL += (size_t)seqs[i].len; }
    jp.seen_cap0.resize(S);
    jp.seen0_total = seen_slots0_wave(len.data(), S, p, cfg, SEEN0_BUDGET, jp.seen_cap0.data());
    jp.seen0_avg = (double)jp.seen0_total / (double)std::max<size_t>(S, 1);
    jp.caps = plan_caps(cfg, S, sumL, p, est, jp.seen0_avg);
    return jp;
}

} // namespace
