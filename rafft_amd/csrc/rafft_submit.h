// rafft_submit.h - a fold from the caller's side: rafft_fold_submit validates the batch, copies and encodes its sequences, cuts
// it into lanes (rafft_hostpure.h) and queues it for the scheduler; rafft_fold_wait hands the finished result over.
// Part of the single translation unit of rafft_api.hip (included there, after rafft_sched.h).
#pragma once

struct rafft_job { std::shared_ptr<Batch> b; };

namespace {

// (holds g.mu)
int submit_locked(const rafft_params *p, int n_seq, const char *const *seqs, const int *lens, int device, rafft_job **job_, bool async_call = true)
{
    if (!p || !job_ || n_seq < 0 || (n_seq > 0 && !seqs)) return fail(RAFFT_ERR_PARAM, "null argument");
    *job_ = nullptr;
    if (!(p->temp > -273.15 && p->temp < 1000.0)) return fail(RAFFT_ERR_TEMP, "temp out of range");
    if (p->temp != 37.0 && !param_set().has_dH)
        return fail(RAFFT_ERR_TEMP, "temp != 37 needs the enthalpy tables of a ViennaRNA parameter file (rafft_load_params); "
                                    "the built-in tables are 37 C only");
    if (p->max_stack < 1 || p->max_stack > 65535) return fail(RAFFT_ERR_PARAM, "max_stack must be in [1, 65535]");
    if (p->nb_mode < 0 || p->max_branch < 0) return fail(RAFFT_ERR_PARAM, "nb_mode/max_branch must be >= 0");
    if (int rc = init_ctx(device)) return rc;
    if (g.T_dirty || g.T_temp != p->temp) {       // other tables: the batches in flight finish with theirs first
        drain();
        if (int rc = ensure_tables(p->temp)) return rc;
    }
    std::shared_ptr<Batch> bp(new Batch());
    Batch &b = *bp;
    b.cfg = read_config();                    // the environment switches as they are NOW travel with the batch (rafft_config.h)
    g_span_level = b.cfg.trace ? 2 : b.cfg.spans >= 0 ? b.cfg.spans : 1;
    b.p = *p; b.n_seq = n_seq; b.t0 = std::chrono::steady_clock::now();
    HostOut *ho = b.ho = new HostOut();
    ho->resize(n_seq);
    // the sequences are copied: the caller's buffers may go away before rafft_fold_wait
    std::vector<int> L(n_seq);
    size_t tot = 0;
    for (int i = 0; i < n_seq; i++) { L[i] = lens ? lens[i] : (int)strlen(seqs[i]); tot += (size_t)std::max(L[i], 0); }
    b.seqbuf.resize(tot + 1);
    b.codebuf.resize(tot + 1);
    std::vector<SeqIn> good;
    std::vector<int> good_len;
    size_t o = 0;
    for (int i = 0; i < n_seq; i++) {
        rafft_seq_result &sr = ho->seq[i];
        memset(&sr, 0, sizeof sr);
        sr.length = L[i];
        sr.status = RAFFT_ERR_HIP;          // "never folded": only emit_rows sets RAFFT_OK, with the rows in place
        if (L[i] <= 0) { sr.status = RAFFT_ERR_EMPTY; continue; }
        char *dst = b.seqbuf.data() + o;
        memcpy(dst, seqs[i], (size_t)L[i]);
        o += (size_t)L[i];
        unsigned bad = 0;
        uint8_t *cdst = b.codebuf.data() + (dst - b.seqbuf.data());
        for (int x = 0; x < L[i]; x++) { const unsigned k = kBaseCode[(unsigned char)dst[x]]; bad |= k; cdst[x] = (uint8_t)(k & 7); }
        if (bad & 8) { sr.status = RAFFT_ERR_BAD_CHAR; continue; }
        if (L[i] > RAFFT_MAX_LEN) { sr.status = RAFFT_ERR_TOO_LONG; continue; }
        good.push_back({dst, L[i], i, 0, cdst});
        good_len.push_back(L[i]);
    }
    for (LaneJob &lj : cut_lanes(good, split_length(std::move(good_len), b.cfg.split), b.cfg.est))
        b.lane[lj.lane].push_back(Job{std::move(lj.seqs), lj.est, 0});
    start_scheduler();
    {
        std::lock_guard<std::mutex> lk(g.qmu);
        g.submitted.push_back(bp);
        g.n_inflight++;
        g.t_last_submit = std::chrono::steady_clock::now();
        g.last_submit_async = async_call;
    }
    g.qcv_sched.notify_one();
    *job_ = new rafft_job{bp};
    return 0;
}

int wait_job(rafft_job *job, rafft_result **out_)
{
    if (out_) *out_ = nullptr;
    if (!job) return fail(RAFFT_ERR_PARAM, "null job");
    std::shared_ptr<Batch> bp = job->b;
    delete job;
    {
        std::unique_lock<std::mutex> lk(g.qmu);
        g.qcv_done.wait(lk, [&] { return bp->done; });
    }
    {
        std::lock_guard<std::mutex> lk(g.mu);
        g.stats = bp->stats;
    }
    if (bp->rc) return fail(bp->rc, bp->err);
    if (!out_) { free_out(bp->ho); bp->ho = nullptr; return fail(RAFFT_ERR_PARAM, "null result pointer"); }
    *out_ = &bp->ho->res;
    bp->ho = nullptr;          // the caller owns it now (rafft_free_result)
    return 0;
}

} // namespace
