// rafft_wave.h - one wave: a batch of sequences folded in lock-step folding steps on one workspace, as a small state machine
// (setup / issue_step / ready / after_beam / finish) that the scheduler drives; the jobs and batches it serves, the owner of a
// result, the timing spans, and the seam call that runs one region through the expand kernel.
// Part of the single translation unit of rafft_api.hip (included there, after rafft_plan.h).
#pragma once

namespace {

// timing events: handed out from a free list and returned when their batch has been finalised, so the spans of a
// wave stay valid while later waves (of the same or of another batch) use the same workspace
hipEvent_t next_event(std::vector<hipEvent_t> &used)
{
    hipEvent_t e = nullptr;
    if (!g.ev_free.empty()) { e = g.ev_free.back(); g.ev_free.pop_back(); }
    else if (hipEventCreate(&e) != hipSuccess) return nullptr;
    used.push_back(e);
    return e;
}

struct Span { hipEvent_t a, b; int kind; };
// Timing events are not free: a pair around every kernel costs ~1.3 ms of the 17 ms benchmark batch (the markers
// serialise the queues).  Level 1 (default) times only the dominant kernel - the one-wavefront expand class, what
// the roofline is computed from; level 2 (RAFFT_SPANS=2 or RAFFT_TRACE) times every stage; level 0 none.
static int g_span_level = 1;
static inline bool span_on(int kind) { return g_span_level >= 2 || (g_span_level == 1 && kind == 11); }
#define SPAN_REC(ev, st, kind) do { if (span_on(kind)) HIPCHK(hipEventRecord((ev), (st))); } while (0)

struct HostOut {   // owner of a rafft_result
    std::vector<rafft_seq_result> seq;
    std::vector<std::vector<int>> step_size, step_off;
    std::vector<int> one_size, one_off;     // ... of a sequence with a single step (every sequence without --traj)
    std::vector<const char *> db_ptr;       // rows live in pinned chunks (one per wave): the D2H copy lands
    std::vector<const int *> dcal_ptr;      // directly in the memory the caller reads
    std::vector<std::shared_ptr<struct PinChunk>> chunks;   // a chunk may hold rows of several batches folded as one wave
    rafft_result res;
    void resize(int n) { seq.resize(n); step_size.resize(n); step_off.resize(n); one_size.assign(n, 0); one_off.assign(n, 0); dcal_ptr.assign(n, nullptr); db_ptr.assign(n, nullptr); }
};
void free_out(HostOut *o) { delete o; }      // (its pinned chunks go back to the pool with their last reference)

struct Batch;
// One wave's worth of work.  `members`: the batches its sequences come from - queued jobs with identical parameters
// are merged (continuous batching), so one wave may serve several batches; seqs[i].bi indexes this list.
struct Job { std::vector<SeqIn> seqs; double est; int depth; std::vector<std::shared_ptr<Batch>> members; bool no_merge = false;
             bool big_prod = false; };    // re-run after a structure had more productive regions than the short lists hold

// One rafft_fold_submit(): its sequences (copied), its result under construction, its jobs (lane 0: the long tail of
// the batch, lane 1: the bulk - see cut_lanes, rafft_hostpure.h) and what the scheduler needs to finish it.
struct Batch {
    rafft_params p;
    Config cfg;                               // the environment switches as they were when the batch was submitted (rafft_config.h)
    int n_seq = 0;
    std::vector<char> seqbuf;                 // the caller's sequences, copied at submit
    std::vector<uint8_t> codebuf;             // ... and as base codes, same offsets
    HostOut *ho = nullptr;
    std::deque<Job> lane[2];                  // as submitted; the scheduler moves them to its own queues
    int pending = 0;                          // jobs (queued or running) that still hold sequences of this batch
    int rc = 0;
    std::string err;
    std::vector<Span> spans;
    std::vector<hipEvent_t> events;           // timing events in use by `spans`
    rafft_stats stats{};
    std::chrono::steady_clock::time_point t0;
    bool done = false;                        // under g.qmu
};

struct SeamIn {     // rafft_expand_node: one region of one given structure
    DebugOut dbg;
    std::vector<uint16_t> pos;
    std::vector<uint32_t> br;
    int ci, cj, pdcal;
};

// adds the host time spent in its scope to `a` (trace)
struct HostTimer {
    double &a;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    ~HostTimer() { a += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }
};

// One wave = one batch of sequences folded in lock-step folding steps on one workspace.  It is a small
// state machine so that a single host thread can drive two waves at once (two pipelines): while it waits
// for one wave's 152-byte read-back the kernels of the other keep the GPU busy.
struct Wave {
    Workspace &ws;
    const Config &cfg;            // of the first member batch (batches with other snapshots are never merged into the wave)
    rafft_params p;
    std::vector<SeqIn> seqs;
    double est;
    std::vector<std::shared_ptr<Batch>> members;   // whose sequences this wave folds (seqs[i].bi)
    Batch &bt;                                      // the first of them: carries the wave's timing spans and statistics
    std::vector<Span> &spans;
    const SeamIn *seam;
    size_t S = 0, sumL = 0, B = 0, bs_lds[2] = {0, 0}, bs_bm[2] = {0, 0} /* bitmap budget of the 256- / 1024-thread beam step (bytes) */, mat_lds = RAFFT_MAX_LEN, out_row_lds = RAFFT_MAX_LEN;
    double reserve = 1.0;         // buffers are allocated for a wave this many times bigger (merged batches to come)
    bool longseq = false;         // a sequence longer than LDS_SEQ: its loops' bases are read from HBM, regions beyond 4096 positions exist
    std::vector<int> off, len;
    std::vector<uint32_t> seen_cap0;      // initial slots of every sequence's `seen` set (seen_slots0)
    size_t seen0_total = 0, seen0_zeroed = 0;      // slots of all initial tables; of those beyond the bitmap budget, which come first and start zeroed
    ClsCfg cf[NGEN + 1];          // (cf[NGEN]: the FFT plan of class 3 beside its FFT-free kernel)
    Caps c;
    Dev d;
    Counters hc;
    unsigned n_active = 0, ovf = 0, last_mat = 0;
    int merged_now = 0, merge_target = 0;   // size class that receives every region of the coming expand step (0: by size)
    int steps = 0;
    int depth = 0;                // regrowths of this job so far
    bool big_prod = false, want_big_prod = false;   // long productive-region lists (1024 per structure) for this run / asked for by it
    bool finished = false;
    long long last_rows_bytes = 0;
    std::vector<OutRec> early_recs, late_recs;
    PinBuf stage{};               // pinned staging of the wave's inputs (setup)
    bool draining = false;        // every step is done, the last rows are on their way to the host (finish): ready() tells when they have landed
    struct Tail { double ms_loop = 0, stats = 0, gather = 0; std::chrono::steady_clock::time_point t0; } tail;   // timings of finish_body for finish_done_body's trace line
    ~Wave() { pin_release(stage); }
    size_t harvested = 0;         // trajectory records whose rows already left through the copy stream (early harvest)
    int emit_rows(size_t first, size_t count, bool early, double *t_gather);
    int result = 0;               // valid when finished: 0, RAFFT_ERR_CAPACITY (regrow) or a hard error
    std::chrono::steady_clock::time_point tw0, tw1;
    double ms_setup = 0, ms_issue = 0, ms_after = 0;   // host time inside issue_step / after_beam (trace)

    Wave(Workspace &w, std::vector<std::shared_ptr<Batch>> m, std::vector<SeqIn> s, double e, const SeamIn *sm = nullptr)
        : ws(w), cfg(m[0]->cfg), p(m[0]->p), seqs(std::move(s)), est(e), members(std::move(m)), bt(*members[0]), spans(members[0]->spans), seam(sm) {}
    HostOut &out_of(int local_seq) { return *members[seqs[local_seq].bi]->ho; }

    double since(std::chrono::steady_clock::time_point t) const
    {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    }
    hipEvent_t next_event() { return ::next_event(bt.events); }
    // a wave whose steps still create many structures keeps the whole GPU busy; afterwards it is latency-bound
    bool heavy(unsigned below) const { return S >= 256 && !finished && (steps < 3 || last_mat >= below); }
    int setup();
    int issue_step();
    // 1: the step's read-back has landed, 0: not yet, -1: the device reported an error (sticky: the wave is failed, not polled forever)
    int ready()
    {
        const hipError_t e = hipEventQuery(ws.ev_hot);
        if (e == hipSuccess) return 1;
        if (e == hipErrorNotReady) return 0;
        fail(RAFFT_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
        return -1;
    }
    std::chrono::steady_clock::time_point t_issued;      // when the running step was issued (the scheduler blocks on the oldest)
    int after_beam();
    int issue_materialize(unsigned n_mat);
    // (every error exit of the two leaves `finished` and `result` set: the scheduler reads `result` of a finished wave, and a failure
    //  while the rows are gathered - a device error, a pinned allocation - must not be released as a batch-level success)
    int finish() { const int rc = finish_body(); if (rc) { finished = true; draining = false; if (!result) result = rc; } return rc; }
    int finish_done() { const int rc = finish_done_body(); if (rc) { finished = true; if (!result) result = rc; } return rc; }
    int finish_body();
    int finish_done_body();
};

int Wave::setup()
{
    S = seqs.size();
    tw0 = std::chrono::steady_clock::now();
    // test hook: a wave of exactly this many sequences fails hard (what a structure beyond the kernels' limits does)
    if (cfg.test_hard_fail >= 0 && (int)S == cfg.test_hard_fail) return fail(RAFFT_ERR_PARAM, "test hook: hard failure of this wave");
    off.resize(S); len.resize(S);
    sumL = 0;
    for (size_t i = 0; i < S; i++) { off[i] = (int)sumL; len[i] = seqs[i].len; sumL += seqs[i].len; }
    // the wave's inputs are staged in a pinned chunk (codes | offsets | lengths | counters image): the uploads below are truly
    // asynchronous and the scheduler thread goes on to the other waves' steps at once (it used to wait here, 0.6-0.7 ms per
    // wave of five batches); the chunk goes back to the pool with the wave
    const size_t st_codes = 0, st_off = (sumL + 16 + 63) & ~(size_t)63, st_len = st_off + ((S * 4 + 63) & ~(size_t)63),
                 st_ctr = st_len + ((S * 4 + 63) & ~(size_t)63), st_soff = st_ctr + ((sizeof(Counters) + 63) & ~(size_t)63),
                 st_scap = st_soff + ((S * 8 + 63) & ~(size_t)63), st_bytes = st_scap + S * 4;
    stage = pin_acquire(st_bytes);
    if (!stage.p) return fail(RAFFT_ERR_HIP, "hipHostMalloc failed for the input staging buffer");
    uint8_t *codes = (uint8_t *)stage.p + st_codes;
    for (size_t i = 0; i < S; i++) {
        uint8_t *dst = codes + off[i];
        if (seqs[i].c) memcpy(dst, seqs[i].c, (size_t)seqs[i].len);          // (encoded at submit, on the caller's thread)
        else {
            const unsigned char *src = (const unsigned char *)seqs[i].s;
            for (int x = 0; x < seqs[i].len; x++) dst[x] = kBaseCode[src[x]] & 7;
        }
    }
    memset(codes + sumL, 0, 16);
    memcpy((char *)stage.p + st_off, off.data(), S * 4);
    memcpy((char *)stage.p + st_len, len.data(), S * 4);
    const double ms_enc = since(tw0);
    int maxL = 0;
    for (size_t i = 0; i < S; i++) maxL = std::max(maxL, len[i]);
    const int direct_n_ = cfg.direct_n;
    const bool force_fft_ = cfg.force_fft != 0;
    const bool nofft1 = !seam && !force_fft_ && direct_n_ >= cls1_P(cfg) / 2 && p.gc_wei >= 0.0 && p.au_wei >= 0.0 && p.gu_wei >= 0.0;
    const bool nofft2 = nofft1 && direct_n_ >= CLS2_P / 2;
    if (int rc = class_cfg(cfg, p.nb_mode, maxL, cf, nofft1, nofft2, nofft1)) return rc;      // (direct class 3: the same conditions as the other FFT-free plans)
    if (cfg.trace)
        for (int c = 0; c < NGEN; c++)
            fprintf(stderr, "[rafft] expand class %d: %d threads x %d regions per workgroup, P <= %d, branches <= %d, lags <= %d, LDS %d B%s\n", c, cf[c].nt, cf[c].wpb,
                    cf[c].Pmax, cf[c].brmax, cf[c].Kmax, cf[c].lds, cf[c].nofft ? " (no FFT buffers)" : "");
    merge_target = maxL > CLS2_P / 2 ? 3 : 2;
    JobPlan jp = plan_job(cfg, p, seqs, est);
    seen_cap0 = std::move(jp.seen_cap0);
    seen0_total = jp.seen0_total;
    const double seen0_avg = jp.seen0_avg;
    c = jp.caps;
    if (std::max((size_t)c.sort_cap * 8, (size_t)24 * 1024) + RL_CAP * 12 + (size_t)(p.max_stack + 4) * (sizeof(ParentInfo) + 16) + 1024 > 150 * 1024)
        return fail(RAFFT_ERR_PARAM, "max_branch + 2*max_stack too large for the LDS-resident beam sort");
    B = (size_t)p.max_stack;

    // Buffers are allocated for the wave that queued batches could be merged into (the scheduler folds up to merge_cap()
    // sequences of equal-parameter batches as one wave), not just for this one: a hipFree + hipMalloc of a multi-GB arena
    // in the middle of a stream of batches stalls every queue for tens of ms - and now and then for SECONDS (measured: one
    // hipMalloc of 7 GB took 2.2 s while another wave's kernels were running; a bench run that met it fell from 290 k to 10 k
    // sequences/s).  Only when that reserve is small against the HBM (the benchmark set: 4.4 GB -> 21.6 GB per workspace, two
    // workspaces for bulk waves: 15 % of the card).
    size_t Sr = S;
    Caps cr = c;
    if (S < merge_cap() && !seam) {
        // (a long-tail job has a few sequences per batch: sized once for 64 of them, whatever gets merged later)
        // bulk batches: for the merge cap itself (a stream of small batches is merged up to it whatever their size), or for five of
        // them when that is too much
        const double reserve_frac = cfg.reserve_frac;
        const size_t tries[2] = {S >= 256 ? merge_cap() : std::max<size_t>(S, std::min<size_t>(64, 32 * S)), S >= 256 ? std::min(merge_cap(), 5 * S) : S};
        Sr = S;
        for (size_t want : tries) {
            if (want <= S) continue;
            Caps big = plan_caps(cfg, want, (size_t)((double)sumL * (double)want / (double)S), p, est, seen0_avg);
            if (big.bytes <= (size_t)((double)g.hbm_total * reserve_frac)) { cr = big; Sr = want; break; }
        }
    }
    reserve = (double)Sr / (double)S;
    const size_t sumLr = Sr == S ? sumL : (size_t)((double)sumL * (double)Sr / (double)S);
#define ENS(buf, bytes) do { if (int rc_ = ensure(ws.buf, (bytes))) return rc_; } while (0)
    ENS(codes, sumLr + 16); ENS(seq_off, Sr * 4); ENS(seq_len, Sr * 4);
    ENS(beam, Sr * B * 4); ENS(beam_n, Sr * 4); ENS(done, Sr * 4); ENS(nsteps, Sr * 4);
    ENS(ch_parent, Sr * c.ch_cap * 2); ENS(ch_combo, Sr * c.ch_cap * 8); ENS(ch_dcal, Sr * c.ch_cap * 4); ENS(ch_h, Sr * c.ch_cap * 16);
    ENS(seen, cr.seen * 16); ENS(seen_off, Sr * 8); ENS(seen_cap, Sr * 4); ENS(seen_cnt, Sr * 4); ENS(seen_bm, cr.seen / 8 + 64); ENS(seen_mode, Sr * 4);
    ENS(st, cr.st * sizeof(StRec)); ENS(prod, cr.nd * 16);
    ENS(nd, cr.nd * sizeof(NodeRec)); ENS(nlist, cr.nd * 4); ENS(nd_slot, cr.nd * 4); ENS(cslot, cr.cand * 8);
    ENS(pos, cr.pos * 2); ENS(br, cr.br * 4); ENS(sp, cr.sp * 4); ENS(cand, cr.cand * 32);
    ENS(looptab, cr.looptab * 8);
    ENS(trec, cr.trec * 16); ENS(tsid, cr.tsid * 4);
    ENS(work0, cr.work * 4); ENS(work1, cr.work * 4); ENS(work2, cr.work * 4); ENS(work3, cr.work * 4); ENS(work4, cr.work * 4); ENS(work5, cr.work * 4);
    ENS(mat, cr.mat * sizeof(MatRec));
    ENS(counters, sizeof(Counters));
#undef ENS


    memset(&d, 0, sizeof d);
    d.T = g.T; d.tw = g.tw; d.S = (int)S;
    d.codes = (const uint8_t *)ws.codes.p; d.seq_off = (const int *)ws.seq_off.p; d.seq_len = (const int *)ws.seq_len.p;
    d.K = p.nb_mode; d.B = p.max_stack; d.max_branch = p.max_branch; d.min_hp = p.min_hp; d.traj = p.traj;
    d.min_nrj = p.min_nrj; d.gc = p.gc_wei; d.au = p.au_wei; d.gu = p.gu_wei;
    // identical loops share one expansion only when the energy filter cannot depend on the
    // parent's absolute energy through float32 rounding, i.e. for the default min_nrj == 0
    d.memo = (p.min_nrj == 0.0) ? 1 : 0;
    if (cfg.no_memo) d.memo = 0;
    if (cfg.force_fft) d.force_fft = 1;   // tests: FFT path for short regions too
    d.rl_cap = RL_CAP;
    longseq = maxL > LDS_SEQ;
    d.pos_packed = longseq ? 0 : 1;          // 12 bits of position leave room for the base code (Dev::pos_packed)
    // 64 productive regions per structure (no BASELINE workload has more: the configs[3] shard - 3000 nt, ms=200 - folds without a
    // regrowth); the lists live in materialize_kernel's LDS: with 256 entries a CU holds 19 of its workgroups instead of 20 at
    // 86 VGPRs (measured: 68.4 -> 62.2 ms per 36 benchmark batches), with 1024 entries 8 (1.5 -> 2.3 ms per batch) - so the long
    // lists are for sequences beyond 4096 nt and for a wave that overflowed the short ones and is being folded again
    d.max_prod = (longseq || big_prod) ? MAX_PROD_LONG : MAX_PROD;
    if (cfg.test_max_prod > 0 && !big_prod && !longseq) d.max_prod = std::max(1, std::min(cfg.test_max_prod, MAX_PROD));   // test hook: short lists overflow early
    if (longseq) {       // scratch of the class for regions beyond 4096 positions: lag values (fp64) + lag column, per workgroup
        d.big_stride = (size_t)2 * cf[0].nmax + (size_t)2 * cf[0].nmax / 4;
        if (int rc = ensure(ws.big, (size_t)cf[0].grid * d.big_stride * 8)) return rc;
        d.big_keyv = (double *)ws.big.p;
    } else if (cf[3].direct3) {      // ... and of class 3 when it runs without FFT buffers: FFT size 8192 at most
        d.big_stride = (size_t)MAX_P + (size_t)MAX_P / 4;
        if (int rc = ensure(ws.big, (size_t)cf[3].grid * d.big_stride * 8)) return rc;
        d.big_keyv = (double *)ws.big.p;
    }
    d.cls1_P = cls1_P(cfg); d.cls1_br = cf[1].brmax;
    d.c3_switch = cfg.c3_switch >= 0 ? cfg.c3_switch : g.n_cu;
    d.cand_slab = std::max(16, cfg.slab);
    d.fetch_bulk = std::max(1, cfg.fetch);
    d.taper_pct = std::max(0, std::min(100, cfg.taper));
    // wide classes: regions of up to 1024 positions are correlated by the exact direct form on multi-word bit masks, longer ones
    // by the LDS FFT (measured on the configs[3] shard: n <= 1024 direct 219.7 ms against 222.8 with the FFT everywhere, 236.4
    // with the direct form up to 4096 - scipy itself switches at 2381, rafft/utils.py:121).  RAFFT_DIRECT_N moves the limit.
    d.direct_n = cfg.direct_n;
    // small-region classes (expand_small_kernel): packed positions (no sequence beyond 4096 nt), the bit-mask form of
    // window_slide (non-negative weights, no forced FFT).  RAFFT_SMALL="n4,n5" moves the limits ("0,0": off).
    d.sm_n4 = std::max(0, std::min(cfg.small_n4, 16)); d.sm_n5 = std::max(d.sm_n4, std::min(cfg.small_n5, 32));
    if (!d.pos_packed || d.force_fft || !(p.gc_wei >= 0.0 && p.au_wei >= 0.0 && p.gu_wei >= 0.0)) d.sm_n4 = d.sm_n5 = 0;
    d.mat_tile = 64;
    d.mat_tile = std::max(1, std::min(cfg.mat_tile, 64));                  // tests: several tiles per structure
    if (cfg.rl_cap >= 0) d.rl_cap = std::min(cfg.rl_cap, RL_CAP);         // tests: region lists not resident in LDS
    d.beam = (int *)ws.beam.p; d.beam_n = (int *)ws.beam_n.p; d.done = (int *)ws.done.p; d.nsteps = (int *)ws.nsteps.p;
    d.ch_cap = c.ch_cap;
    d.ch_parent = (uint16_t *)ws.ch_parent.p; d.ch_combo = (uint64_t *)ws.ch_combo.p; d.ch_dcal = (int *)ws.ch_dcal.p; d.ch_h = (uint64_t *)ws.ch_h.p;
    d.seen = (uint64_t *)ws.seen.p; d.seen_cap_total = c.seen;
    d.seen_off = (uint64_t *)ws.seen_off.p; d.seen_cap = (uint32_t *)ws.seen_cap.p; d.seen_cnt = (uint32_t *)ws.seen_cnt.p;
    d.seen_bm = (uint32_t *)ws.seen_bm.p; d.seen_mode = (uint32_t *)ws.seen_mode.p;
    d.st_cap = (uint32_t)c.st;
    d.st = (StRec *)ws.st.p;
    d.prod = (ProdEnt *)ws.prod.p; d.prod_shard_cap = c.nd / NSHARD;
    d.nd_cap = (uint32_t)c.nd;
    d.nd = (NodeRec *)ws.nd.p; d.nlist = (int *)ws.nlist.p; d.nd_slot = (uint32_t *)ws.nd_slot.p; d.cslot = (unsigned long long *)ws.cslot.p;
    d.looptab = (unsigned long long *)ws.looptab.p; d.looptab_cap = c.looptab;
    d.pos = (uint16_t *)ws.pos.p; d.pos_cap = c.pos; d.br = (uint32_t *)ws.br.p; d.br_cap = c.br;
    d.sp = (uint32_t *)ws.sp.p; d.sp_cap = c.sp;
    d.cand = (Cand *)ws.cand.p; d.cand_cap = c.cand;
    d.trec = (int4 *)ws.trec.p; d.trec_cap = (uint32_t)c.trec; d.tsid = (int *)ws.tsid.p; d.tsid_cap = c.tsid;
    d.work[0] = (int *)ws.work0.p; d.work[1] = (int *)ws.work1.p; d.work[2] = (int *)ws.work2.p; d.work[3] = (int *)ws.work3.p;
    d.work[4] = (int *)ws.work4.p; d.work[5] = (int *)ws.work5.p; d.work_cap = (uint32_t)c.work;
    d.mat = (MatRec *)ws.mat.p; d.mat_cap = (uint32_t)c.mat;
    d.c = (Counters *)ws.counters.p;
    d.nd_base = S; d.nd_shard_cap = (c.nd - S) / NSHARD;
    d.pos_base = sumL; d.pos_shard_cap = (c.pos - sumL) / NSHARD;
    d.sp_shard_cap = c.sp / NSHARD;
    d.br_shard_cap = c.br / NSHARD; d.cand_shard_cap = c.cand / NSHARD;
    if (seam) d.dbg = seam->dbg;


    // beam_step_kernel LDS: time-shared region 0 (walk scratch 24 B/thread and the occupancy bitmap of the sequence's `seen` table, then
    // the sort keys), region list, per-member records.  The bitmap's budget: for the 256-thread kernel 4 KiB - tables of up to 32 768
    // slots -, which keeps five workgroups on a CU with the benchmark's plan (measured against 8 KiB: DESIGN.md 3.11); for the
    // 1024-thread kernel, one workgroup per CU, 32 KiB.  While a set grows the old bitmap is parked in the walk's scratch, 16 bytes
    // per thread: a budget is at most twice that.  A table beyond the budget keeps the compare-and-swap protocol.  (A wave only ever
    // goes from the 256-thread kernel to the 1024-thread one, so that one's budget is never the smaller: no launch meets a table in
    // bitmap mode that it cannot hold.)
    for (int v = 1; v >= 0; v--) {
        const size_t nt = v ? 1024 : 256;
        const size_t rest = RL_CAP * 12 + B * sizeof(ParentInfo) + (B + 1) * 8 + ((B + 3) & ~(size_t)3) * 4 + 128 + B * 4;      // (+ B ints: the prepass's first node-list entries)
        size_t bm = v ? 32768 : 4096;
        if (cfg.seen_bm_max >= 0) bm = std::min((size_t)cfg.seen_bm_max & ~(size_t)15, 32 * nt);
        while (bm && 24 * nt + bm + rest > 160 * 1024) bm = (bm / 2) & ~(size_t)15;
        if (v == 0) bm = std::min(bm, bs_bm[1]);
        bs_bm[v] = bm;
        bs_lds[v] = std::max((size_t)c.sort_cap * 8, 24 * nt + bm) + rest;
    }
    d.seen_bm0 = (uint32_t)bs_bm[S < (size_t)std::max(0, cfg.wide_below) ? 1 : 0];      // (issue_step: which kernel takes the first step)

    const double ms_plan = since(tw0);
    hipStream_t st = ws.stream;
    // (RAFFT_TRACE: a call of this section that keeps the scheduler thread for more than a millisecond is named - every wave in flight waits)
    double t_mark = ms_plan;
    auto slow_call = [&](const char *what) {
        if (!cfg.trace) return;
        const double now = since(tw0);
        if (now - t_mark > 1.0) fprintf(stderr, "[rafft] setup of a wave of %zu sequences: %s kept the host for %.3f ms\n", S, what, now - t_mark);
        t_mark = now;
    };
    memset(&hc, 0, sizeof hc);
    hc.n_struct = S; hc.seen_top = seen0_total;
    memcpy((char *)stage.p + st_ctr, &hc, sizeof hc);
    {
        // the sequences' initial `seen` tables, back to back (seen_slots0)
        uint64_t *so = (uint64_t *)((char *)stage.p + st_soff);
        uint32_t *sc = (uint32_t *)((char *)stage.p + st_scap);
        // (the tables beyond the first launch's bitmap budget come first: they start zeroed, by one memset - init_roots_kernel applies
        //  the same test to set Dev::seen_mode)
        size_t o = 0;
        for (int big = 1; big >= 0; big--) {
            for (size_t i = 0; i < S; i++) {
                if ((seen_cap0[i] / 8 > d.seen_bm0) != (big != 0)) continue;
                // (a table's bitmap is addressed as bit so[i] of the bitmap arena, in whole 32-bit words)
                if ((o | seen_cap0[i]) & 31) return fail(RAFFT_ERR_PARAM, "internal: a seen table does not start on a whole word of the bitmap arena");
                so[i] = o; sc[i] = seen_cap0[i]; o += seen_cap0[i];
            }
            if (big) seen0_zeroed = o;
        }
        // base codes | offsets | lengths | seen-table offsets | sizes | counters image: one kernel reads them out of the pinned chunk
        StageIn si;
        memset(&si, 0, sizeof si);
        auto seg = [&](size_t off, void *dst, size_t bytes) {
            si.src[si.n] = (const uint32_t *)((const char *)stage.p + off); si.dst[si.n] = (uint32_t *)dst; si.words[si.n] = (bytes + 3) / 4; si.n++;
        };
        seg(st_codes, ws.codes.p, sumL + 16); seg(st_off, ws.seq_off.p, S * 4); seg(st_len, ws.seq_len.p, S * 4);
        seg(st_soff, ws.seen_off.p, S * 8); seg(st_scap, ws.seen_cap.p, S * 4); seg(st_ctr, ws.counters.p, sizeof hc);
        const size_t words = (sumL + 16 + 3) / 4;
        hipLaunchKernelGGL(stage_in_kernel, dim3((unsigned)std::min<size_t>((words + 255) / 256, 1024)), dim3(256), 0, st, si);
        HIPCHK(hipGetLastError());
    }
    slow_call("the launch of stage_in_kernel");
    if (d.memo) HIPCHK(hipMemsetAsync(ws.looptab.p, 0, c.looptab * 8, st));
    slow_call("the memset of the loop table");
    // the bitmaps of every sequence's first table (1/128 of the tables' own bytes; the tables are not zeroed: a slot is read only where
    // its bit is set), and the first tables beyond the bitmap budget themselves; tables handed out later build their bitmap, or are
    // zeroed, where they are allocated (seen_grow).
    if (d.seen_bm0) HIPCHK(hipMemsetAsync(ws.seen_bm.p, 0, seen0_total / 8, st));
    if (seen0_zeroed) HIPCHK(hipMemsetAsync(ws.seen.p, 0, seen0_zeroed * 16, st));
    slow_call("the memset of the seen bitmaps");
    hipLaunchKernelGGL(init_roots_kernel, dim3((unsigned)S), dim3(64), 0, st, d);
    HIPCHK(hipGetLastError());
    slow_call("the launch of init_roots_kernel");
    if (seam) HIPCHK(hipStreamSynchronize(st));      // (the seam overwrites the root region with synchronous copies right after)
    mat_lds = 20 * (size_t)d.max_prod;
    out_row_lds = ((size_t)maxL + 15) & ~(size_t)15;      // output_kernel builds a dot-bracket row in LDS: the longest sequence of the wave
    n_active = (unsigned)S;
    ms_setup = since(tw0);
    if (cfg.trace) fprintf(stderr, "[rafft] setup: encode %.3f ms, plan+buffers %.3f ms, copies+init %.3f ms\n", ms_enc, ms_plan - ms_enc, ms_setup - ms_plan);
    tw1 = std::chrono::steady_clock::now();
    return 0;
}

// expand (three size classes on their own streams) -> beam step -> asynchronous read-back of the hot counters
int Wave::issue_step()
{
    HostTimer acc_{ms_issue};
    hipStream_t st = ws.stream;
    const unsigned wide_below = (unsigned)std::max(0, cfg.wide_below);
    const bool serial = cfg.serial != 0;
    const unsigned small_wg_per_cu = (unsigned)std::max(1, cfg.small_wg);   // 4 wavefronts each
    const size_t hot_len = offsetof(Counters, node);
    HIPCHK(hipEventRecord(ws.ev_fork, st));
    Span wall{next_event(), next_event(), 4};
    SPAN_REC(wall.a, st, 4);
    static const int order[NCLS] = {3, 0, 2, 1, 5, 4};    // big-LDS classes first
    for (int oi = 0; oi < NCLS; oi++) {
        const int cls = order[oi];
        if (cls == 0 && !longseq) continue;                      // regions beyond 4096 positions: only sequences longer than that have them
        if (cls == 3 && merge_target == 2) continue;             // no sequence long enough for a region of that class
        if (merged_now == 3 && cls != 3 && cls != 0) continue;   // the dedupe of the last step sent everything to one class
        if (merged_now == 2 && cls == 1) continue;               // ... or the one-wavefront class to the 256-thread one
        if (cls >= NGEN && (merged_now != 0 || steps == 0 || (cls == 4 ? d.sm_n4 : d.sm_n5) == 0 || (cls == 5 && d.sm_n5 == d.sm_n4))) continue;   // small-region classes: off, or nothing was sent there
        const bool inline_ = serial || (merged_now == 3 && !longseq);   // a single kernel: no fork/join through another stream
        hipStream_t cs = inline_ ? st : ws.cls_stream[cls];
        if (!inline_) HIPCHK(hipStreamWaitEvent(cs, ws.ev_fork, 0));
        Span sp{next_event(), next_event(), 10 + cls};
        SPAN_REC(sp.a, cs, sp.kind);
        // persistent workgroups loop over the work list, so any grid is correct: when few structures were
        // materialized (the tail of a batch) a small grid avoids dispatching thousands of empty workgroups
        unsigned grid = cls >= NGEN ? (unsigned)g.n_cu * small_wg_per_cu : (unsigned)cf[cls].grid;
        if (steps > 0) {
            const unsigned long long bound = (unsigned long long)last_mat * (cls == 1 ? 8ULL : 4ULL) + 32ULL;
            if (bound < grid) grid = (unsigned)bound;
        }
        if (int rc = launch_expand_cls(cfg, d, cls, cf, grid, cs)) return rc;
        if (cls == 1) bt.stats.n_expand_launches++;       // launches of the dominant kernel (ms_expand is their sum)
        SPAN_REC(sp.b, cs, sp.kind);
        spans.push_back(sp);
        if (!inline_) {
            HIPCHK(hipEventRecord(ws.ev_join[cls], cs));
            HIPCHK(hipStreamWaitEvent(st, ws.ev_join[cls], 0));
        }
    }
    SPAN_REC(wall.b, st, 4);
    spans.push_back(wall);
    {
        Span sp{next_event(), next_event(), 1};
        SPAN_REC(sp.a, st, sp.kind);
        // few sequences left (the long ones): a 1024-thread workgroup per sequence shortens the serial
        // chains (16 wavefronts for the prepass, 1024 combos per chunk); many sequences: 256 threads
        if (n_active < wide_below) hipLaunchKernelGGL((beam_step_kernel<1024>), dim3((unsigned)S), dim3(1024), bs_lds[1], st, d, c.sort_cap, (int)bs_bm[1]);
        else hipLaunchKernelGGL((beam_step_kernel<256>), dim3((unsigned)S), dim3(256), bs_lds[0], st, d, c.sort_cap, (int)bs_bm[0]);
        HIPCHK(hipGetLastError());
        SPAN_REC(sp.b, st, sp.kind);
        spans.push_back(sp);
    }
    steps++;
    HIPCHK(hipMemcpyAsync(ws.hot, ws.counters.p, hot_len, hipMemcpyDeviceToHost, st));   // pinned: truly asynchronous
    HIPCHK(hipEventRecord(ws.ev_hot, st));
    t_issued = std::chrono::steady_clock::now();
    return 0;
}

// materialize the `nm` new beam members of the step whose counters have just been read back, and find the loops among their
// regions that are known already
int Wave::issue_materialize(unsigned nm)
{
    hipStream_t st = ws.stream;
    Span sp{next_event(), next_event(), 2};
    SPAN_REC(sp.a, st, sp.kind);
    // (four structures per wavefront, teams of 16 lanes, when the short productive-region lists are in use -
    //  materialize_team_kernel; otherwise one structure per wavefront)
    if (d.max_prod <= MAT4_PROD)
        hipLaunchKernelGGL(materialize_team_kernel, dim3((nm + MAT4_TEAMS - 1) / MAT4_TEAMS), dim3(64), 0, st, d, (int)nm);
    else hipLaunchKernelGGL(materialize_kernel, dim3(nm), dim3(MAT_NT), mat_lds, st, d, (int)nm);
    HIPCHK(hipGetLastError());
    // tail of the batch: so few new structures that their regions fit one wave of workgroups of the widest class
    // (measured on the benchmark batch: 18.8 -> 17.3 ms; thresholds in new structures per step, per CU)
    // (round 3, after the 256-thread class got its production build and four workgroups per CU: everything goes to the widest
    //  class only below 2 structures per CU - 16 per CU before; a burst of 20 shard batches 18.5 -> 17.8 ms, the rest unchanged)
    const unsigned merge_below = cfg.merge_below >= 0 ? (unsigned)cfg.merge_below : 2u * (unsigned)g.n_cu;
    const unsigned merge2_below = cfg.merge2_below >= 0 ? (unsigned)cfg.merge2_below : 128u * (unsigned)g.n_cu;
    d.merge_cls = seam ? 0 : nm < merge_below ? merge_target : nm < merge2_below ? 2 : 0;
    merged_now = d.merge_cls;
    // (a thread per region created in this step - two or three per new structure: light steps launch a handful of workgroups instead
    //  of two per CU, which used to queue behind the expand kernels of the other waves only to find nothing)
    const unsigned dd_grid = std::min<unsigned>((unsigned)g.n_cu * (1024u / DEDUPE_NT), (unsigned)std::min<unsigned long long>(0x7fffffffULL, (unsigned long long)nm * 4ULL / DEDUPE_NT + 2ULL));
    hipLaunchKernelGGL(dedupe_kernel, dim3(dd_grid), dim3(DEDUPE_NT), 0, st, d);
    HIPCHK(hipGetLastError());
    SPAN_REC(sp.b, st, sp.kind);
    spans.push_back(sp);
    return 0;
}

// the beam step of this wave has finished: stop, or materialize the new beam members and go on
int Wave::after_beam()
{
    HostTimer acc_{ms_after};
    hipStream_t st = ws.stream;
    if (draining) return finish_done();            // the last rows have landed
    const size_t hot_len = offsetof(Counters, node);
    memcpy(&hc, ws.hot, hot_len);
    if (hc.overflow) { ovf = hc.overflow; return finish(); }
    // test hook: pretend an arena overflowed at this step of the first attempt (regrowth late in a wave)
    if (cfg.test_ovf_at >= 0 && depth == 0 && steps == cfg.test_ovf_at) { ovf = OVF_STRUCT; return finish(); }
    if (hc.n_mat == 0) return finish();
    n_active = (unsigned)S - hc.n_done;
    last_mat = hc.n_mat;
    // most sequences of the wave have finished: their rows leave beside the folding steps of the others - once this step's kernels
    // are queued (below): the host's share of it, a millisecond or two for a wave of 16 k sequences, is off the wave's own path
    const bool harvest_now = !p.traj && !seam && !harvested && S >= 256 && (size_t)hc.trec_n * 10 >= S * 7;
    const size_t harvest_n = (size_t)hc.trec_n;
    if (int rc = issue_materialize(hc.n_mat)) return rc;
    if (cfg.trace >= 2) {
        Counters h2;
        HIPCHK(hipMemcpyAsync(&h2, ws.counters.p, hot_len, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        fprintf(stderr, "[rafft] step %d: n_mat %u -> work %u %u %u %u | small %u %u\n", steps, hc.n_mat, h2.n_work[0].v, h2.n_work[1].v, h2.n_work[2].v, h2.n_work[3].v, h2.n_work[4].v, h2.n_work[5].v);
    }
    const int step_of_harvest = steps;
    if (int rc = issue_step()) return rc;
    if (harvest_now && !finished) {
        if (int rc = emit_rows(0, harvest_n, true, nullptr)) return rc;
        harvested = harvest_n;
        if (cfg.trace) fprintf(stderr, "[rafft] early harvest after step %d: %zu of %zu sequences\n", step_of_harvest, harvested, S);
    }
    return 0;
}

// Format the beams of trajectory records [first, first + count) as result rows on the device and copy them to a
// pinned chunk of their own.  `early`: on the copy stream, while the wave goes on folding (only the records of
// sequences that have finished are final, so this is used without --traj, where a sequence has one record).
int Wave::emit_rows(size_t first, size_t count, bool early, double *t_gather)
{
    const auto t0_ = std::chrono::steady_clock::now();
    hipStream_t st = early ? ws.copy_stream : ws.stream;
    Buf &b_rec = early ? ws.row_off2 : ws.row_off, &b_db = early ? ws.out_db2 : ws.out_db, &b_dc = early ? ws.out_dcal2 : ws.out_dcal;
    std::vector<int4> trec(count);
    if (count) HIPCHK(hipMemcpy(trec.data(), (const int4 *)ws.trec.p + first, count * sizeof(int4), hipMemcpyDeviceToHost));
    // records in (sequence, step) order; rows are laid out record after record.  (Without --traj a sequence has ONE record: any order
    // of the records will do, and sorting 16 k of them is a millisecond of the scheduler thread.)
    if (p.traj) std::sort(trec.begin(), trec.end(), [](const int4 &a, const int4 &b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
    std::vector<OutRec> &recs = early ? early_recs : late_recs;     // (members: they outlive the asynchronous upload)
    recs.assign(trec.size(), OutRec{});
    long long tot_bytes = 0;
    size_t nrows = 0;
    for (size_t ri = 0; ri < trec.size(); ri++) {
        const int4 &r = trec[ri];
        recs[ri] = OutRec{tot_bytes, (int)nrows, r.w, r.z, len[r.x]};
        tot_bytes += (long long)r.z * (len[r.x] + 1);
        nrows += (size_t)r.z;
    }
    if (t_gather) *t_gather = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count();
    last_rows_bytes = tot_bytes;
    if (!nrows) return 0;
    const size_t dcal_off = ((size_t)tot_bytes + 63) & ~(size_t)63;
    PinBuf chunk;
    chunk = pin_acquire(dcal_off + nrows * 4 + 64);
    if (!chunk.p) return fail(RAFFT_ERR_HIP, "hipHostMalloc failed for the result buffer");
    {
        auto shared = std::make_shared<PinChunk>(chunk);
        for (auto &m : members) m->ho->chunks.push_back(shared);
    }
    char *all_db = (char *)chunk.p;
    int *all_dcal = (int *)((char *)chunk.p + dcal_off);
    if (int rc = ensure(b_rec, (size_t)((double)(recs.size() * sizeof(OutRec)) * reserve))) return rc;
    if (int rc = ensure(b_db, (size_t)((double)tot_bytes * reserve))) return rc;
    if (int rc = ensure(b_dc, (size_t)((double)(nrows * 4) * reserve))) return rc;
    HIPCHK(hipMemcpyAsync(b_rec.p, recs.data(), recs.size() * sizeof(OutRec), hipMemcpyHostToDevice, st));
    Span sp{next_event(), next_event(), 3};
    SPAN_REC(sp.a, st, sp.kind);
    unsigned grid = (unsigned)std::min<size_t>(nrows, 65536);
    hipLaunchKernelGGL(output_kernel, dim3(grid), dim3(64), out_row_lds, st, d, (int)nrows, (int)recs.size(), (const OutRec *)b_rec.p,
                       (char *)b_db.p, (int *)b_dc.p);
    HIPCHK(hipGetLastError());
    SPAN_REC(sp.b, st, sp.kind);
    spans.push_back(sp);
    HIPCHK(hipMemcpyAsync(all_db, b_db.p, (size_t)tot_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(all_dcal, b_dc.p, nrows * 4, hipMemcpyDeviceToHost, st));
    // `recs` was handed to an asynchronous copy from pageable memory: HIP stages such copies before returning.  Nobody waits
    // here: the early rows are waited for at the end of the wave, the late ones by the scheduler's poll of Workspace::ev_hot (finish)
    // per-sequence views into the chunk (the pointers are only read by the caller after the call has returned)
    for (size_t r0 = 0; r0 < recs.size();) {
        const int i = trec[r0].x;
        size_t r1 = r0;
        while (r1 < recs.size() && trec[r1].x == i) r1++;
        const int gi = seqs[i].idx;
        HostOut &out = out_of(i);
        int o = 0;
        if (r1 - r0 == 1) { out.one_size[gi] = o = recs[r0].cnt; out.one_off[gi] = 0; }      // (no heap allocation per sequence)
        else {
            auto &ss = out.step_size[gi];
            auto &so = out.step_off[gi];
            ss.resize(r1 - r0); so.resize(r1 - r0);
            for (size_t r = r0; r < r1; r++) { ss[r - r0] = recs[r].cnt; so[r - r0] = o; o += recs[r].cnt; }
        }
        out.dcal_ptr[gi] = all_dcal + recs[r0].row0;
        out.db_ptr[gi] = all_db + recs[r0].off;
        rafft_seq_result &sr = out.seq[gi];
        sr.status = RAFFT_OK; sr.length = len[i]; sr.n_steps = (int)(r1 - r0); sr.n_structs = o;
        r0 = r1;
    }
    return 0;
}

// Every step is done.  The statistics are read back, the rows that have not left yet are formatted and sent to the host - and
// the scheduler thread goes back to the other waves: it used to sit in a stream synchronize here for the 1-3 ms the rows of a
// wave of five batches take (32 MB D2H), during which no other wave's step was read back or issued.  ready() / after_beam()
// see the end of that copy through Workspace::ev_hot (finish_done).
int Wave::finish_body()
{
    hipStream_t st = ws.stream;
    finished = true;
    tail.ms_loop = since(tw1);
    tail.t0 = std::chrono::steady_clock::now();
    bt.stats.n_steps = std::max<int64_t>(bt.stats.n_steps, steps);
    if (ovf && cfg.trace) fprintf(stderr, "[rafft] wave S=%zu est %.1f overflowed (bits %u) after %d steps, %.1f ms\n", S, est, ovf, steps, since(tw0));
    if (ovf) {
        HIPCHK(hipStreamSynchronize(st));
        if (harvested) HIPCHK(hipStreamSynchronize(ws.copy_stream));
        if ((ovf & OVF_PROD) && !(ovf & OVF_SORT) && d.max_prod < MAX_PROD_LONG) {
            want_big_prod = true;          // not a limit yet: the wave is folded again with the long lists (MAX_PROD_LONG)
            return result = RAFFT_ERR_CAPACITY;
        }
        if (ovf & (OVF_PROD | OVF_SORT))
            return result = fail(RAFFT_ERR_PARAM, "structure with more than 1024 productive regions, or sort capacity exceeded");
        return result = RAFFT_ERR_CAPACITY;
    }
    // statistics (SURVEY.md 8d algorithmic bytes; only expansions the kernels really executed)
    HIPCHK(hipMemcpy(&hc, ws.counters.p, sizeof hc, hipMemcpyDeviceToHost));
    for (int c = 0; c < NCLS; c++)            // the sharded statistics lines (Counters::xstat)
        for (int i = 0; i < NSHARD; i++) {
            const Counters::StatLine &x = hc.xstat[c][i];
            hc.n_expand += x.items; hc.sum_n += x.n; hc.sum_lags += x.lags; hc.sum_nbr += x.nbr;
            hc.cls_items[c] += x.items; hc.cls_sum_n[c] += x.n; hc.cls_sum_lags[c] += x.lags;
            hc.n_alias += x.alias; hc.n_children += x.children; hc.sum_struct_len += x.struct_len;
            bt.stats.n_dE_evals += (int64_t)x.evals; bt.stats.n_dE_guessed += (int64_t)x.guessed; bt.stats.n_kept_guessed += (int64_t)x.kept_guessed;
        }
    {
        unsigned long long nn = S, ni = S;
        for (int i = 0; i < NSHARD; i++) { nn += hc.node[i].v; ni += hc.nlist[i].v; }
        bt.stats.n_nodes_created += (int64_t)nn;
        bt.stats.n_node_instances += (int64_t)ni;
    }
    bt.stats.n_node_expansions += hc.n_expand;
    bt.stats.n_nodes_aliased += (int64_t)hc.n_alias;
    bt.stats.sum_node_len += hc.sum_n;
    bt.stats.sum_lags += hc.sum_lags;
    bt.stats.n_structs += (int64_t)hc.n_struct;
    bt.stats.n_children += hc.n_children;
    bt.stats.sum_struct_len += (int64_t)(hc.sum_struct_len + sumL);
    {
        int64_t ex = 3 * (int64_t)hc.sum_n + 16 * (int64_t)hc.sum_lags + 3 * (int64_t)(hc.sum_struct_len + sumL);
        // the dominant kernel (size class 1, P <= 512): its own regions, and the per-structure term in
        // proportion to the regions it expanded
        double share = hc.n_expand ? (double)hc.cls_items[1] / (double)hc.n_expand : 0.0;
        bt.stats.alg_bytes_expand += 3 * (int64_t)hc.cls_sum_n[1] + 16 * (int64_t)hc.cls_sum_lags[1] +
                                    (int64_t)(share * 3.0 * (double)(hc.sum_struct_len + sumL));
        for (int c = 0; c < NCLS; c++) {       // the same figure per size class (2, 3 + regions beyond 4096 positions, small-region classes)
            const double sh = hc.n_expand ? (double)hc.cls_items[c] / (double)hc.n_expand : 0.0;
            const int64_t v = 3 * (int64_t)hc.cls_sum_n[c] + 16 * (int64_t)hc.cls_sum_lags[c] + (int64_t)(sh * 3.0 * (double)(hc.sum_struct_len + sumL));
            if (c == 2) bt.stats.alg_bytes_expand_c2 += v;
            else if (c == 3 || c == 0) bt.stats.alg_bytes_expand_c3 += v;
            else if (c >= NGEN) bt.stats.alg_bytes_expand_small += v;
        }
        bt.stats.alg_bytes_beam += 2 * (int64_t)hc.sum_struct_len + 8 * (int64_t)(hc.n_struct - S);
        bt.stats.alg_bytes_expand_all += ex;
        bt.stats.alg_bytes += ex + 2 * (int64_t)hc.sum_struct_len + 8 * (int64_t)(hc.n_struct - S);
    }


    tail.stats = since(tail.t0);
    // ---- the rows that have not left yet: records of sequences that finished after the early harvest (or all)
    if (int rc = emit_rows(harvested, (size_t)hc.trec_n - harvested, false, &tail.gather)) return rc;
    tail.gather += tail.stats;
    if (harvested) {                                  // the early rows went through the copy stream: one event covers both
        HIPCHK(hipEventRecord(ws.ev_copy, ws.copy_stream));
        HIPCHK(hipStreamWaitEvent(st, ws.ev_copy, 0));
    }
    HIPCHK(hipEventRecord(ws.ev_hot, st));
    finished = false; draining = true;
    return 0;
}

int Wave::finish_done_body()
{
    finished = true;
    const double tl_copy = since(tail.t0);
    const long long tot_bytes = last_rows_bytes;
    if (cfg.trace) {
        auto mx = [&](const ShardCtr *sc) { unsigned long long m = 0, t = 0; for (int i = 0; i < NSHARD; i++) { m = std::max(m, sc[i].v); t += sc[i].v; } return std::make_pair(m, t); };
        auto nd = mx(hc.node), po = mx(hc.pos), br = mx(hc.br), spr = mx(hc.sp), ca = mx(hc.cand), pr = mx(hc.prod), nl = mx(hc.nlist);
        fprintf(stderr, "[rafft] max productive regions per structure: %u (limit %d)\n", hc.max_nprod, d.max_prod);
        fprintf(stderr, "[rafft] arenas used/cap (max shard | total): st %llu/%zu  nd %llu/%llu|%llu  pos %llu/%llu|%llu  br %llu/%llu|%llu  sp %llu/%llu|%llu  cand %llu/%llu|%llu  prod %llu/%llu|%llu  nlist %llu/%llu|%llu  seen %llu/%zu  est %.1f\n",
                hc.n_struct, c.st, nd.first, (unsigned long long)d.nd_shard_cap, nd.second, po.first, (unsigned long long)d.pos_shard_cap, po.second,
                br.first, (unsigned long long)d.br_shard_cap, br.second, spr.first, (unsigned long long)d.sp_shard_cap, spr.second,
                ca.first, (unsigned long long)d.cand_shard_cap, ca.second, pr.first, (unsigned long long)d.prod_shard_cap, pr.second, nl.first, (unsigned long long)d.nd_shard_cap, nl.second, hc.seen_top, c.seen, est);
    }
    if (cfg.trace >= 2) {       // how full the `seen` sets got, by sequence length (sizes the initial tables: a growth is a rehash)
        std::vector<uint32_t> cnt(S), cap(S);
        HIPCHK(hipMemcpy(cnt.data(), d.seen_cnt, S * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cap.data(), d.seen_cap, S * 4, hipMemcpyDeviceToHost));
        const int edges[] = {0, 80, 100, 130, 200, 300, 500, 1000, 2000, 1 << 30};
        for (int e = 0; e + 1 < (int)(sizeof(edges) / sizeof(edges[0])); e++) {
            unsigned long long n = 0, sum = 0, mxc = 0, grown = 0, slots = 0;
            for (size_t i = 0; i < S; i++) if (len[i] > edges[e] && len[i] <= edges[e + 1]) { n++; sum += cnt[i]; mxc = std::max<unsigned long long>(mxc, cnt[i]); grown += cap[i] > seen_cap0[i] ? 1 : 0; slots += cap[i]; }
            if (n) fprintf(stderr, "[rafft] seen sets, %d < L <= %d: %llu sequences, mean %llu entries, max %llu, %llu grew, %llu slots at the end\n", edges[e], edges[e + 1], n, sum / n, mxc, grown, slots);
        }
    }
    if (cfg.trace) fprintf(stderr, "[rafft] host time inside issue_step %.3f ms, inside after_beam (incl. nested issue_step and this tail) %.3f ms\n", ms_issue, ms_after);
    if (cfg.trace) fprintf(stderr, "[rafft] wave S=%zu setup %.2f ms, loop %.2f ms (%d steps), tail %.2f ms (counters %.3f, records+gather %.3f, rows out %.3f incl. %.1f MB D2H)\n",
                                       S, ms_setup, tail.ms_loop, steps, since(tail.t0), tail.stats, tail.gather - tail.stats, tl_copy - tail.gather, (double)tot_bytes / 1e6);
    return result = 0;
}

// rafft_expand_node: one region of one given structure through the expand kernel
int run_seam(Batch &bt, const std::vector<SeqIn> &one, const SeamIn &sm)
{
    Wave w(g.ws[0], {std::shared_ptr<Batch>(&bt, [](Batch *) {})}, one, 4.0, &sm);
    if (int rc = w.setup()) return rc;
    Workspace &W = g.ws[0];
    // overwrite the root region of sequence 0 with the given loop of the given structure
    {
        std::vector<uint16_t> packed(sm.pos);
        if (w.d.pos_packed) {
            for (auto &v : packed) v = (uint16_t)(v | (kBaseCode[(unsigned char)one[0].s[v]] << 12));
        }
        HIPCHK(hipMemcpy(W.pos.p, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    }
    if (!sm.br.empty()) {
        std::vector<uint32_t> pb(sm.br);
        if (w.d.pos_packed)      // (the base codes of a helix's outermost pair ride in bits 12-15 and 28-31)
            for (auto &v : pb) v |= ((uint32_t)kBaseCode[(unsigned char)one[0].s[v & 0xFFFFu]] << 12) | ((uint32_t)kBaseCode[(unsigned char)one[0].s[v >> 16]] << 28);
        HIPCHK(hipMemcpy(W.br.p, pb.data(), pb.size() * 4, hipMemcpyHostToDevice));
    }
    int n = (int)sm.pos.size(), nbr = (int)sm.br.size();
    {
        NodeRec root;                                       // region 0 as init_roots_kernel left it, with the given loop
        HIPCHK(hipMemcpy(&root, W.nd.p, sizeof root, hipMemcpyDeviceToHost));
        root.n = n; root.nbr = nbr; root.ci = sm.ci; root.cj = sm.cj; root.pdcal = sm.pdcal;
        HIPCHK(hipMemcpy(W.nd.p, &root, sizeof root, hipMemcpyHostToDevice));
    }
    int cls = node_class(n, (sm.ci < 0 || one[0].len > LDS_SEQ) ? one[0].len : sm.cj + 1 - sm.ci, nbr, 0, w.d.cls1_P, w.d.cls1_br, w.d.K, w.d.sm_n4, w.d.sm_n5);
    int zero = 0;
    memset(&w.hc.n_work, 0, sizeof w.hc.n_work);
    w.hc.n_work[cls].v = 1;
    HIPCHK(hipMemcpy(W.counters.p, &w.hc, sizeof w.hc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(w.d.work[cls], &zero, 4, hipMemcpyHostToDevice));
    if (int rc = launch_expand_cls(w.cfg, w.d, cls, w.cf, 1, W.stream)) return rc;
    HIPCHK(hipStreamSynchronize(W.stream));
    return 0;
}

} // namespace
