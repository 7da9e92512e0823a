// rafft_sched.h - the scheduler: the one thread that drives every wave of every batch in flight, what finishes a batch,
// the idle trimming of the workspaces, and the thread's start, fork handling and drain.
// Part of the single translation unit of rafft_api.hip (included there, after rafft_wave.h).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------------- scheduler
// ONE thread drives every wave of every batch in flight.  A wave is a small state machine (issue_step / after_beam
// above): while the thread waits for one wave's 152-byte read-back the kernels of the others keep the GPU busy.
// Batches queue up (rafft_fold_submit); a batch is cut in a long-tail job and a bulk job (lanes 0 and 1).  What runs
// when - continuous batching:
//   * every queued job is admitted as soon as a workspace is free: the bulk of the next batch starts while the running
//     one is still folding, so the tail of a batch - and its long-tail wave - run beside the next batch's busy steps
//     (measured on the benchmark batch, three batches in flight: 11.9 ms per batch against 13.1 for synchronous
//     calls; holding the next bulk wave back until the running one has turned light was 2-4 % slower);
//   * a job that does not fit the HBM still free is split (or waits for running waves to release theirs).
struct Slot { std::unique_ptr<Wave> wave; Job job; int lane = 0; };

static unsigned admit_below()
{
    return 128u * (unsigned)g.n_cu;     // = the step size below which the one-wavefront expand class is merged away
}

static bool same_params(const rafft_params &a, const rafft_params &b)
{
    return a.nb_mode == b.nb_mode && a.max_stack == b.max_stack && a.max_branch == b.max_branch && a.min_hp == b.min_hp &&
           a.min_nrj == b.min_nrj && a.traj == b.traj && a.temp == b.temp && a.gc_wei == b.gc_wei && a.au_wei == b.au_wei && a.gu_wei == b.gu_wei;
}

static void finalize_batch(const std::shared_ptr<Batch> &bp)
{
    Batch &b = *bp;
    if (b.rc) {
        // early-harvest copies or kernels of a sibling wave may still be in flight: the pinned result chunks return
        // to the pool only once the device is idle
        { hipError_t e_ = hipDeviceSynchronize(); (void)e_; }
        free_out(b.ho);
        b.ho = nullptr;
    } else {
        if (b.cfg.trace) {       // per-step timeline: spans are recorded in step order
            float acc[16] = {0};
            int stepno = 0;
            for (auto &sp : b.spans) {
                float ms = 0;
                if (!span_on(sp.kind) || hipEventElapsedTime(&ms, sp.a, sp.b) != hipSuccess) continue;
                if (sp.kind < 16) acc[sp.kind] += ms;
                if (sp.kind == 1) {        // the beam step closes a folding step (materialize of it follows)
                    fprintf(stderr, "[rafft] t-step %2d: expand wall %.3f (c1 %.3f c2 %.3f c3 %.3f) beam %.3f  prev-materialize %.3f\n",
                            ++stepno, acc[4], acc[11], acc[12], acc[13], acc[1], acc[2]);
                    for (float &x : acc) x = 0;
                }
            }
        }
        for (auto &sp : b.spans) {
            float ms = 0;
            if (span_on(sp.kind) && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
                if (sp.kind == 14 || sp.kind == 15) b.stats.ms_expand_c1 += ms;   /* small-region classes 4 and 5 (expand_small_kernel) */
                else if (sp.kind == 10) b.stats.ms_expand_c3 += ms;   /* class 0 (regions beyond 4096 positions) rides with the widest class */
                else if (sp.kind == 11) b.stats.ms_expand += ms;   /* dominant kernel: regions with P <= 512 */
                else if (sp.kind == 12) b.stats.ms_expand_c2 += ms;
                else if (sp.kind == 13) b.stats.ms_expand_c3 += ms;
                else if (sp.kind == 4) b.stats.ms_expand_wall += ms;
                else if (sp.kind == 1) b.stats.ms_beam += ms;
                else if (sp.kind == 2) b.stats.ms_materialize += ms;
                else b.stats.ms_output += ms;
            }
        }
        HostOut *ho = b.ho;
        for (int i = 0; i < b.n_seq; i++) {
            rafft_seq_result &sr = ho->seq[i];
            const bool one = ho->step_size[i].empty();
            sr.step_size = one ? &ho->one_size[i] : ho->step_size[i].data(); sr.step_off = one ? &ho->one_off[i] : ho->step_off[i].data();
            sr.db = ho->db_ptr[i]; sr.dcal = ho->dcal_ptr[i];
        }
        ho->res.n_seq = b.n_seq; ho->res.seq = ho->seq.data(); ho->res._owner = ho;
        ho->res.n_failed = 0;
        for (int i = 0; i < b.n_seq; i++) ho->res.n_failed += ho->seq[i].status != RAFFT_OK;
        b.stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b.t0).count();
    }
    for (hipEvent_t e : b.events) g.ev_free.push_back(e);
    b.events.clear(); b.spans.clear();
    {
        std::lock_guard<std::mutex> lk(g.qmu);
        b.done = true;
        g.n_inflight--;
    }
    g.qcv_done.notify_all();
}

// Nothing in flight: workspaces that grew beyond two fifths of the HBM for some huge batch are given back (other processes
// may share the card; the next batch allocates what it needs).
static void trim_workspaces()
{
    std::unique_lock<std::mutex> lk(g.ws_mu, std::try_to_lock);
    if (!lk.owns_lock()) return;              // a seam call is using workspace 0 right now
    size_t held = 0;
    for (int i = 0; i < MAX_PIPES; i++) held += g.ws[i].bytes();
    if (held <= g.hbm_total / 5 * 2) return;       // (round 5: 2/5 of the card, a quarter until then - a stream's three bulk workspaces, sized for the merge cap at once, are 96 GB and stay)
    for (int i = 0; i < MAX_PIPES; i++) g.ws[i].release_buffers();
}

struct Scheduler {
    Slot slot[MAX_PIPES];
    std::deque<Job> queue[2];                 // lane 0: long-tail jobs, lane 1: bulk jobs; submission order
    int n_active_batches = 0;
    // waves in flight: two (typically the long-tail wave of one batch beside a bulk wave) - more only split the work
    // into smaller, less efficient waves (measured with 6-12 batches in flight: 2 waves 9.5-9.9 ms per benchmark batch, 3-4
    // waves 10.1-10.3 ms) and multiply the HBM held by workspaces
    // (round 4: THREE bulk waves.  A kernel trace of the pipelined loop with two - tools/concurrency.py - shows an expand kernel in flight
    //  for 70 % of the wall time; for the rest only a beam step or the small latency-bound kernels of the tails are.  A third wave fills
    //  part of that: steady state over 80 benchmark batches 367-377 k -> 384-388 k sequences/s with 15 in flight, a 20-step bench run
    //  366 -> 373 k; four waves of four batches 372-375 k - smaller waves, more launches.  Round 2 measured the opposite with waves of
    //  one or two batches and twice the kernel time per batch.)
    const Config &scfg = g.sched_cfg;          // (read by start_scheduler, before this thread was started)
    const int max_waves = std::max(1, std::min(scfg.max_waves, MAX_PIPES));
    bool big_prod_seen = false;               // a wave with `big_prod_params` met a structure with more productive regions than the short lists hold
    rafft_params big_prod_params{};
    int big_prod_quiet = 0;                   // ... and this many waves in a row since then, folded with the long lists, never needed them:
                                              // after eight the short lists are back (one outlier batch does not slow the process for good)
    std::chrono::steady_clock::time_point last_progress = std::chrono::steady_clock::now();
    // of the pass in progress (run): whether anything moved, and the waves that are running
    bool progressed = false, heavy_running = false;
    int n_running = 0, n_lane[2] = {0, 0};

    // a member batch is finished when its last job is: finalise it
    void release(Job &job, int rc, const std::string &err)
    {
        for (auto &m : job.members) {
            if (rc && !m->rc) { m->rc = rc; m->err = err; }
            if (--m->pending == 0) { finalize_batch(m); n_active_batches--; }
        }
        job.members.clear();
    }
    // A job some of whose member batches have failed elsewhere keeps folding for the healthy ones: the failed members'
    // sequences are taken out (their batches are released from this job), the rest stays one job.  False: nothing left.
    bool strip_failed(Job &job)
    {
        bool any = false;
        for (auto &m : job.members) any = any || m->rc != 0;
        if (!any) return true;
        std::vector<int> remap(job.members.size(), -1);
        std::vector<std::shared_ptr<Batch>> keep_m;
        for (size_t i = 0; i < job.members.size(); i++) {
            auto &m = job.members[i];
            if (m->rc == 0) { remap[i] = (int)keep_m.size(); keep_m.push_back(m); }
            else if (--m->pending == 0) { finalize_batch(m); n_active_batches--; }
        }
        std::vector<SeqIn> keep_s;
        for (SeqIn sq : job.seqs) if (remap[sq.bi] >= 0) { sq.bi = remap[sq.bi]; keep_s.push_back(sq); }
        job.members.swap(keep_m); job.seqs.swap(keep_s);
        return !job.members.empty() && !job.seqs.empty();
    }
    // A hard error of a wave that folds several batches (merged by the scheduler because their parameters were equal)
    // must not fail batches whose own sequences are fine: every member is folded again on its own; only a job of ONE
    // batch takes the error.
    void fail_or_split(Slot &sl, int rc, const std::string &err)
    {
        if (sl.job.members.size() <= 1 || rc == RAFFT_ERR_NO_DEVICE) { release(sl.job, rc, err); return; }
        for (size_t i = 0; i < sl.job.members.size(); i++) {
            Job one;
            one.est = sl.job.est; one.depth = sl.job.depth; one.no_merge = true; one.big_prod = sl.job.big_prod;
            one.members.assign(1, sl.job.members[i]);
            for (SeqIn sq : sl.job.seqs) if (sq.bi == (int)i) { sq.bi = 0; one.seqs.push_back(sq); }
            if (one.seqs.empty()) { if (--sl.job.members[i]->pending == 0) { finalize_batch(sl.job.members[i]); n_active_batches--; } continue; }
            queue[sl.lane].push_front(std::move(one));        // (the member's pending count moves with it)
        }
        sl.job.members.clear();
    }
    // The wave of this slot failed with `rc` (g_err holds the message): the device runs dry, the slot is freed and the job takes
    // the error or is split by member.  `whole_job`: a sticky device error - no member is folded again, the job is released.
    void fail_slot(Slot &sl, int rc, bool whole_job = false)
    {
        const std::string err = g_err;
        { hipError_t e_ = hipDeviceSynchronize(); (void)e_; }
        if (whole_job) release(sl.job, rc, err);
        sl.wave.reset();
        if (!whole_job) fail_or_split(sl, rc, err);
    }
    // under g.qmu, as g.n_inflight is documented
    static int n_inflight()
    {
        std::lock_guard<std::mutex> lk(g.qmu);
        return g.n_inflight;
    }

    // the submitted batches join the lane queues (sleeping while there is nothing to do); false: the process is exiting
    bool intake()
    {
        if (n_active_batches == 0) free_garbage();            // nothing in flight: the device is idle, hipFree is cheap
        std::unique_lock<std::mutex> lk(g.qmu);
        if (g.stop && n_active_batches == 0 && g.submitted.empty()) return false;
        if (n_active_batches == 0 && g.submitted.empty()) {
            // idle for a second: give back workspaces that grew huge (re-allocating 80 GB costs seconds, so not between
            // back-to-back batches)
            if (!g.qcv_sched.wait_for(lk, std::chrono::seconds(1), [] { return !g.submitted.empty() || g.stop; })) {
                lk.unlock();
                trim_workspaces();
                lk.lock();
                g.qcv_sched.wait(lk, [] { return !g.submitted.empty() || g.stop; });
            }
            if (g.stop && g.submitted.empty()) return false;
        }
        while (!g.submitted.empty()) {
            std::shared_ptr<Batch> bp = g.submitted.front();
            g.submitted.pop_front();
            n_active_batches++;
            bp->pending = 1;                                  // (held while its jobs are being queued)
            for (int ln = 0; ln < 2; ln++)
                for (Job &j : bp->lane[ln]) {
                    if (j.seqs.empty()) continue;
                    j.members.assign(1, bp);
                    bp->pending++;
                    queue[ln].push_back(std::move(j));
                }
            bp->lane[0].clear(); bp->lane[1].clear();
            if (--bp->pending == 0) { lk.unlock(); finalize_batch(bp); n_active_batches--; lk.lock(); }   // nothing foldable in it
        }
        return true;
    }

    // a running wave whose step has landed goes on - or ends: released, regrown, or failed
    void advance(Slot &sl)
    {
        if (!sl.wave) return;
        const int rdy = sl.wave->ready();
        if (rdy == 0) return;
        progressed = true;
        if (rdy < 0) { fail_slot(sl, RAFFT_ERR_HIP, true); return; }      // sticky device error: fail the job, free the slot
        int rc = sl.wave->after_beam();
        if (sl.wave->finished) {
            if (sl.wave->result || !rc) rc = sl.wave->result;      // (a failure on the way out that left no result keeps its own code)
            if (rc == RAFFT_ERR_CAPACITY) {
                if (sl.job.depth >= 12)
                    release(sl.job, RAFFT_ERR_CAPACITY, "HBM arena overflow after 12 regrowths (bits " + std::to_string(sl.wave->ovf) + ")");
                else {                                   // re-run with larger arenas, ahead of everything queued
                    sl.job.members[0]->stats.n_regrows++;
                    if (sl.wave->want_big_prod) {                                // (same arenas, longer lists)
                        sl.job.big_prod = true;
                        sl.job.members[0]->stats.n_regrows_prod++;
                        // sticky: later waves with these parameters start with the long lists instead of paying the double fold again
                        big_prod_seen = true; big_prod_params = sl.job.members[0]->p; big_prod_quiet = 0;
                    }
                    else sl.job.est *= (sl.job.depth >= 2 ? 4.0 : 2.0);
                    sl.job.depth++;
                    queue[sl.lane].push_front(std::move(sl.job));
                }
            } else if (rc) fail_slot(sl, rc);
            else {
                if (sl.wave->big_prod && !sl.job.members.empty()) {
                    sl.job.members[0]->stats.n_waves_long_lists++;
                    if (!sl.job.big_prod && big_prod_seen) {       // the long lists came from the sticky flag, not from this job's own overflow
                        if (sl.wave->hc.max_nprod <= MAX_PROD) { if (++big_prod_quiet >= 8) { big_prod_seen = false; big_prod_quiet = 0; } }
                        else big_prod_quiet = 0;
                    }
                }
                release(sl.job, 0, "");
            }
            sl.wave.reset();
        } else if (rc) fail_slot(sl, rc);
    }

    // A caller that streams batches (two or more in flight) queues them microseconds apart: a bulk wave admitted the moment the
    // first one arrives would fold that one alone and the second wave whatever came in the meantime - three waves one after the
    // other (heavy phases do not overlap) where one merged wave would do.  So while submissions keep coming (the last one less
    // than RAFFT_LINGER_US = 600 us ago) and the queues are below the merge cap, both lanes wait for them.  A lone synchronous
    // call never lingers.
    bool should_linger()
    {
        const long linger_us = scfg.linger_us;
        bool linger = false;
        if (linger_us > 0 && (!queue[1].empty() || !queue[0].empty())) {
            size_t queued = 0;
            for (int ln = 0; ln < 2; ln++) for (auto &j : queue[ln]) queued = std::max(queued, j.seqs.size() * queue[ln].size());   // (a bound is enough)
            std::lock_guard<std::mutex> lk(g.qmu);
            // (the FIRST batch of a burst lingers too when it came through rafft_fold_submit - otherwise it is folded alone, in both
            //  lanes, and the long-tail lane, one wave at a time, needs two rounds: 20 shard batches 17.8 -> 13.4 ms.  rafft_fold_batch,
            //  whose caller is blocked and cannot be streaming, never lingers.)
            const long lim = (g.n_inflight >= 2 || g.last_submit_async) ? linger_us : 0;
            linger = queued < merge_cap() &&
                     std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - g.t_last_submit).count() < lim;
        }
        return linger;
    }

    // a free workspace.  The long-tail lane keeps workspace 0 to itself and the bulk lane the others; a lane whose own are all
    // busy takes any free one - the biggest for a bulk wave, the smallest otherwise.  (Round 5: by slot parity - "this
    // lane's first" - a bulk wave now and then landed on the workspace the long-tail waves had used so far and grew all
    // its 43 buffers to bulk size: 23.6 GB of hipMalloc in the middle of a stream of batches, in one bench run out of four,
    // and one hipMalloc in a few hundred takes SECONDS - measured 3.4 s, a run of 13 k sequences/s instead of 500 k.)
    int pick_workspace(int ln, bool job_heavy)
    {
        int w = -1;
        auto better = [&](int k) { return w < 0 || (job_heavy ? g.ws[k].bytes() > g.ws[w].bytes() : g.ws[k].bytes() < g.ws[w].bytes()); };
        for (int k = 0; k < MAX_PIPES; k++) if (!slot[k].wave && (k == 0) == (ln == 0) && better(k)) w = k;
        if (w < 0) for (int k = 0; k < MAX_PIPES; k++) if (!slot[k].wave && better(k)) w = k;
        return w;
    }
    // continuous batching: queued jobs with the same parameters join this one (first regrowths stay alone)
    void merge_queued(Job &job, int ln)
    {
        // (a sequence beyond 16 384 nt makes the class for the biggest regions plan for 32 768 positions, which lowers the
        //  wave's nb_mode limit from ~400 to 106 - class_cfg: jobs are not merged across that line)
        auto very_long = [](const Job &j) { for (auto &sq : j.seqs) if (sq.len > 16384) return true; return false; };
        const bool job_vl = very_long(job);
        while (job.depth == 0 && !job.no_merge && !queue[ln].empty()) {
            Job &nx = queue[ln].front();
            bool nx_failed = false;
            for (auto &m : nx.members) nx_failed = nx_failed || m->rc != 0;
            if (nx.depth != 0 || nx.no_merge || nx_failed || !same_params(nx.members[0]->p, job.members[0]->p) || !same_config(nx.members[0]->cfg, job.members[0]->cfg) ||
                job.seqs.size() + nx.seqs.size() > merge_cap() || very_long(nx) != job_vl)
                break;
            const int off = (int)job.members.size();
            for (SeqIn sq : nx.seqs) { sq.bi += off; job.seqs.push_back(sq); }
            for (auto &m : nx.members) job.members.push_back(m);
            job.est = std::max(job.est, nx.est);
            queue[ln].pop_front();
        }
    }
    enum class Fit { fits, split, wait };
    // the HBM admission test of a job for workspace `w`: a job too big for one wave goes back to the queue in halves, one that
    // only does not fit beside what running waves hold goes back whole
    Fit fits_or_split(Job &job, int w, int ln)
    {
        const Caps cc = plan_job(job.members[0]->cfg, job.members[0]->p, job.seqs, job.est).caps;
        size_t others = 0;
        for (int k = 0; k < MAX_PIPES; k++) if (k != w) others += g.ws[k].bytes();
        const size_t budget = (size_t)((double)g.hbm_total * 0.55 / 2.0);
        bool fits_now = std::max(cc.bytes, g.ws[w].bytes()) + others <= (size_t)((double)g.hbm_total * 0.85);
        // waves whose arenas take more than a tenth of the HBM run one at a time (the halves of a split job would
        // otherwise fill two workspaces of that size)
        const double big_wave_frac = scfg.big_wave_frac;
        const size_t big_wave = (size_t)((double)g.hbm_total * big_wave_frac);
        if (cc.bytes > big_wave)
            for (int k = 0; k < MAX_PIPES; k++) if (slot[k].wave && slot[k].wave->c.bytes > big_wave) fits_now = false;
        if ((cc.bytes > budget || cc.capped || (!fits_now && n_running == 0)) && job.seqs.size() > 1) {
            const size_t h = job.seqs.size() / 2;          // too big for one wave: two jobs, one after the other
            if (job.members[0]->cfg.trace)
                fprintf(stderr, "[rafft] job of %zu sequences folded in halves: plan %.1f GB (budget %.1f), this workspace holds %.1f GB, the others %.1f GB, %s%s\n",
                        job.seqs.size(), (double)cc.bytes / 1e9, (double)budget / 1e9, (double)g.ws[w].bytes() / 1e9, (double)others / 1e9,
                        cc.capped ? "a table at the limit of its ids, " : "", fits_now ? "fits" : "does not fit beside what is held");
            Job a{std::vector<SeqIn>(job.seqs.begin(), job.seqs.begin() + h), job.est, job.depth, job.members, true, job.big_prod};
            Job c{std::vector<SeqIn>(job.seqs.begin() + h, job.seqs.end()), job.est, job.depth, job.members, true, job.big_prod};
            for (auto &m : job.members) m->pending++;      // one job became two (halves of a split are not merged again)
            queue[ln].push_front(std::move(c));
            queue[ln].push_front(std::move(a));
            progressed = true;
            return Fit::split;
        }
        if (!fits_now && n_running > 0) { queue[ln].push_front(std::move(job)); return Fit::wait; }   // wait for running waves to finish
        return Fit::fits;
    }
    // A stream of batches (two or more in flight) will have `max_waves` bulk waves going at once: the bulk lane's other
    // workspaces are brought to this one's sizes NOW, while the stream is young, instead of whenever a third wave first
    // overlaps two others - 23.6 GB of hipMalloc at an arbitrary moment, and one hipMalloc in a few hundred takes
    // seconds (bench.py: a run in six allocated its third workspace inside the timed region, 300 k instead of 500 k).
    // Only workspaces that are not bulk-sized yet (less than a quarter of this one): one that merely lags behind a
    // workspace that grew for some wave is left alone - following it would put 2 x 47 GB of hipMalloc into the stream.
    int prematch_siblings(int w)
    {
        int rc = 0;
        size_t held = 0, add = 0;
        for (int k = 0; k < MAX_PIPES; k++) held += g.ws[k].bytes();
        for (int k = 1; k <= max_waves && k < MAX_PIPES; k++) if (k != w && !slot[k].wave && g.ws[k].bytes() < g.ws[w].bytes() / 4) add += g.ws[w].bytes() - g.ws[k].bytes();
        size_t free_b = 0, total_b = 0;
        if (add && hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
        // (at most half of the card for this process, and at most half of what is free now: other processes share it)
        if (add && held + add <= (size_t)((double)g.hbm_total * 0.5) && add <= free_b / 2)
            for (int k = 1; k <= max_waves && k < MAX_PIPES && !rc; k++)
                if (k != w && !slot[k].wave && g.ws[k].bytes() < g.ws[w].bytes() / 4) { rc = init_ws(g.ws[k]); if (!rc) rc = g.ws[k].match(g.ws[w]); }
        return rc;
    }
    void start_wave(Job &&job, int w, int ln, bool job_heavy)
    {
        Slot &sl = slot[w];
        sl.job = std::move(job);
        sl.lane = ln;
        int rc = init_ws(g.ws[w]);
        if (!rc) {
            sl.wave.reset(new Wave(g.ws[w], sl.job.members, sl.job.seqs, sl.job.est));
            sl.wave->depth = sl.job.depth;
            sl.wave->big_prod = sl.job.big_prod || (big_prod_seen && same_params(big_prod_params, sl.job.members[0]->p));
            if (sl.job.members[0]->cfg.trace) fprintf(stderr, "[rafft] wave of %zu sequences (lane %d) takes workspace %d (%.1f GB held)\n", sl.job.seqs.size(), ln, w, (double)g.ws[w].bytes() / 1e9);
            rc = sl.wave->setup();
            if (!rc && job_heavy && n_inflight() >= 2) rc = prematch_siblings(w);
            if (!rc) rc = sl.wave->issue_step();
        }
        progressed = true;
        if (rc) { fail_slot(sl, rc); return; }
        n_running++; n_lane[ln]++;
        heavy_running = heavy_running || (job_heavy && sl.wave->heavy(admit_below()));
    }
    void admit(int ln)
    {
        while (!queue[ln].empty() && (ln == 0 ? n_lane[0] < 1 : n_lane[1] < max_waves && n_running < MAX_PIPES)) {
            Job &front = queue[ln].front();
            if (!strip_failed(front)) {                       // every member already failed elsewhere: nothing to fold
                Job j = std::move(front); queue[ln].pop_front(); release(j, 0, ""); progressed = true; continue;
            }
            const bool job_heavy = front.seqs.size() >= 256;
            if (job_heavy && heavy_running) break;
            const int w = pick_workspace(ln, job_heavy);
            if (w < 0) break;
            Job job = std::move(front);
            queue[ln].pop_front();
            merge_queued(job, ln);
            const Fit fit = fits_or_split(job, w, ln);
            if (fit == Fit::split) continue;
            if (fit == Fit::wait) break;
            start_wave(std::move(job), w, ln, job_heavy);
        }
    }

    // Nothing moved.  A step's read-back lands within tens to hundreds of microseconds, so the thread polls for a
    // short while; after that it stops holding a core (below).
    void idle(bool linger)
    {
        const auto now = std::chrono::steady_clock::now();
        if (progressed) { last_progress = now; return; }
        if (linger) { std::this_thread::yield(); return; }          // (at most linger_us: keep looking)
        const long spin_us = scfg.spin_us;
        if (std::chrono::duration_cast<std::chrono::microseconds>(now - last_progress).count() < spin_us) { std::this_thread::yield(); return; }
        bool any_wave = false;
        for (int i = 0; i < MAX_PIPES; i++) any_wave = any_wave || (bool)slot[i].wave;
        if (any_wave) {
            // Several waves run and ANY of them may finish its step next: sleeping on one wave's event made the others wait for it
            // (measured: the long-tail wave's steps - 14 sequences, 0.3 ms of kernels - sat 0.5 ms on average, up to 1.6 ms, behind
            // a bulk wave's step, and while the long-tail wave holds one of the two wave slots the bulk waves do not overlap).  So
            // the thread naps in short slices and looks at all of them; a nap costs no core to speak of.
            const long nap_us = scfg.nap_us;
            std::this_thread::sleep_for(std::chrono::microseconds(nap_us));
        } else {
            // nothing running yet something queued (a job waiting for HBM that running waves hold cannot happen here: no wave runs)
            std::unique_lock<std::mutex> lk(g.qmu);
            g.qcv_sched.wait_for(lk, std::chrono::milliseconds(1), [] { return !g.submitted.empty() || g.stop; });
        }
    }

    void run()
    {
        for (;;) {
            if (!intake()) return;
            progressed = false;
            // ---- advance the running waves
            for (Slot &sl : slot) advance(sl);
            // ---- admit queued jobs: the long-tail lane first (light from the start), then the bulk lane
            n_running = 0; heavy_running = false;
            for (int i = 0; i < MAX_PIPES; i++) if (slot[i].wave) { n_running++; heavy_running = heavy_running || slot[i].wave->heavy(admit_below()); }
            // The long-tail lane has a wave slot of its own: a long-tail wave (a handful of sequences, two dozen latency-bound steps)
            // never keeps a second bulk wave from starting (288 -> 294 k sequences/s with eight batches in flight, three interleaved
            // pairs of runs, against the lanes sharing the `max_waves` slots as in round 2)
            n_lane[0] = n_lane[1] = 0;
            for (int i = 0; i < MAX_PIPES; i++) if (slot[i].wave) n_lane[slot[i].lane]++;
            const bool linger = should_linger();
            for (int ln = 0; ln < 2 && !linger; ln++) admit(ln);          // (both lanes: the long-tail jobs of a burst are merged into one wave too - the lane runs one at a time)
            idle(linger);
        }
    }
};

static void scheduler_main()
{
    { hipError_t e_ = hipSetDevice(g.device); (void)e_; }
    Scheduler s;
    s.run();
}

// In the child of a fork() the scheduler thread does not exist (only the forking thread survives), yet the inherited Ctx says it
// was started and the inherited atexit(rafft_shutdown) would join it: the child forgets the thread object (never joined, never
// destructed as joinable) and starts a scheduler of its own if it ever submits.  (A HIP context does not survive a fork either:
// a child that folds must initialise the GPU itself - this only keeps a child that does NOT fold from hanging in exit().)
static void atfork_child()
{
    new (&g.sched_thread) std::thread();      // placement-new over the stale handle: ~thread() of a joinable thread would terminate()
    g.sched_started = false; g.stop = false; g.n_inflight = 0;
    new (&g.qmu) std::mutex(); new (&g.mu) std::mutex();       // (may have been held by another thread of the parent at fork time)
}
static void start_scheduler()
{
    std::lock_guard<std::mutex> lk(g.qmu);    // (sched_started / sched_thread: the same mutex as rafft_shutdown)
    if (g.sched_started) return;
    g.sched_started = true;
    g.sched_cfg = read_config();              // the scheduler's own settings: read when it starts (rafft_config.h)
    g.sched_thread = std::thread(scheduler_main);
    static bool registered = false;
    if (!registered) {
        registered = true;
        // stopped and joined at process exit BEFORE the HIP runtime tears down (atexit handlers run in reverse order of
        // registration and the runtime registered its own when it was initialised, earlier than this)
        atexit(rafft_shutdown);
        pthread_atfork(nullptr, nullptr, atfork_child);
    }
}

// no batch may be in flight when the device tables change or a seam call borrows workspace 0
static void drain()
{
    std::unique_lock<std::mutex> lk(g.qmu);
    g.qcv_done.wait(lk, [] { return g.n_inflight == 0; });
}

} // namespace
