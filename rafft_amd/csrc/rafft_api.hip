// rafft_api.hip - the C-ABI of include/rafft_hip.h, and the one translation unit of libraffthip.so.
//
// One process drives one GPU.  The kernels and the host headers below are included here, so templates and the Dev struct are
// shared without a device-link step; this file itself holds the extern "C" entry points and their direct helpers: submit / wait of
// a fold, structure evaluation, the seam call, energy parameters, kinetics, the folding landscape and accuracy scoring.
// A fold is the reference's bfs_pairs recursion (rafft/rafft.py:156-216) turned into an iteration over folding steps that
// advances every sequence of a wave at once:   expand (new unpaired regions) -> beam step (per sequence) -> materialize
// (new beam members) -> ... until every sequence reached its fixed point.  Every workspace has a stream set of its own
// (rafft_host_ctx.h); one scheduler thread drives the waves of all batches in flight (rafft_sched.h); the other entry points
// drain the folds in flight and run on the streams of workspace 0.
#include "../../include/rafft_hip.h"
#include "rafft_kernels.h"
#include "rafft_params.h"
#include "rafft_config.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <deque>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>

// kernels (rafft_kernels.hip - the shared device helpers, which in turn includes one file per fold kernel: rafft_expand.hip,
// rafft_expand_small.hip, rafft_beam.hip, rafft_materialize.hip, rafft_io_kernels.hip - is compiled into the same translation
// unit so the templates and the Dev struct are shared without a device-link step)
#include "rafft_kernels.hip"
#include "rafft_kin.hip"
#include "rafft_landscape.hip"
#include "rafft_score.hip"

// host side, one responsibility per file (each in its own anonymous namespace)
#include "rafft_host_ctx.h"     // errors, workspaces and their buffers, the global context, memory pools, initialisation
#include "rafft_plan.h"         // size classes and LDS plans of the expand kernel, the HBM arenas of a job
#include "rafft_wave.h"         // jobs, batches, the Wave state machine, the seam call
#include "rafft_sched.h"        // the scheduler thread

extern "C" {

const char *rafft_last_error(void) { return g_err.c_str(); }

/* Drains the batches in flight, stops the scheduler thread and joins it.  Registered with atexit(); may be called by
 * hand before unloading the library.  Entry points called afterwards start a fresh scheduler. */
void rafft_shutdown(void)
{
    std::thread t;
    {
        std::unique_lock<std::mutex> lk(g.qmu);
        if (!g.sched_started) return;
        g.qcv_done.wait(lk, [] { return g.n_inflight == 0; });
        g.stop = true;
        t = std::move(g.sched_thread);
    }
    g.qcv_sched.notify_all();
    if (t.joinable()) t.join();
    std::lock_guard<std::mutex> lk(g.qmu);
    g.stop = false; g.sched_started = false;
}

/* out[0..4] = device buffers allocated so far (calls), their bytes, the slowest such call in microseconds, pinned host chunks
 * allocated (calls), their bytes.  Process-wide, monotonic: a caller that takes the difference around a region of its own
 * sees whether the library had to allocate inside it (a hipMalloc of gigabytes now and then takes seconds). */
void rafft_alloc_counters(unsigned long long out[5])
{
    out[0] = g_dev_allocs; out[1] = g_dev_bytes; out[2] = g_dev_worst_us; out[3] = g_pin_allocs; out[4] = g_pin_bytes;
}

const char *rafft_version(void) { return "raffthip 0.2 (gfx950, HIP; built-in Turner-2004 37C tables or ViennaRNA parameter files)"; }

int rafft_init(int device)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return init_ctx(device);
}

struct rafft_job { std::shared_ptr<Batch> b; };

// (holds g.mu)
static int submit_locked(const rafft_params *p, int n_seq, const char *const *seqs, const int *lens, int device, rafft_job **job_, bool async_call = true)
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
    ho->seq.resize(n_seq); ho->step_size.resize(n_seq); ho->step_off.resize(n_seq); ho->one_size.assign(n_seq, 0); ho->one_off.assign(n_seq, 0);
    ho->dcal_ptr.assign(n_seq, nullptr); ho->db_ptr.assign(n_seq, nullptr);
    // the sequences are copied: the caller's buffers may go away before rafft_fold_wait
    std::vector<int> L(n_seq);
    size_t tot = 0;
    for (int i = 0; i < n_seq; i++) { L[i] = lens ? lens[i] : (int)strlen(seqs[i]); tot += (size_t)std::max(L[i], 0); }
    b.seqbuf.resize(tot + 1);
    b.codebuf.resize(tot + 1);
    std::vector<SeqIn> good;
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
    }
    // ---- lanes.  Folds are independent, so how the batch is cut cannot change any result.  The number of
    // folding steps of a wave is set by its longest sequence, and the steps that only the long ones still need
    // are latency-bound and nearly empty (the benchmark set: 24 steps for two 2.9-knt sequences, 12 for the rest).
    // So a batch whose few longest sequences stand far out is cut in two jobs: the long tail starts first and runs
    // beside the bulk (and beside the bulk of the next batch).  The workspaces of the bulk lane have a stream
    // priority of their own, which gives them HW queues of their own - with all streams at one priority the waves
    // share the process's four queues and the cut is a loss (17.3 ms against 15.2 for the benchmark batch; with it: 13.3 ms).
    // RAFFT_SPLIT: unset / -1 automatic, 0 never, > 0 cut at that length.
    int split_len = 0;
    {
        const int want = b.cfg.split;
        if (good.size() >= 32 && want != 0 && (want > 0 || good.size() < 16384)) {     // (very large batches amortise the tail anyway)
            if (want > 0) split_len = want;
            else {   // the sequences at least twice as long as the 99th percentile of the batch (leaving room for two)
                std::vector<int> ls;
                for (auto &sq : good) ls.push_back(sq.len);
                std::sort(ls.begin(), ls.end());
                const size_t top = std::max<size_t>(2, ls.size() / 100);
                const int ref = ls[ls.size() - top - 1];
                if (ls.back() >= 2 * ref) split_len = 2 * ref;
            }
        }
    }
    {
        auto est_of = [&](const std::vector<SeqIn> &v) {
            // expected survivors per beam slot (~ folding steps in which a slot is renewed): grows with length
            size_t sl = 0;
            for (auto &sq : v) sl += sq.len;
            double e0 = 6.0 + (v.empty() ? 0.0 : (double)sl / (double)v.size()) / 100.0;
            if (b.cfg.est > 0) e0 = b.cfg.est;
            return e0;
        };
        std::vector<SeqIn> shorts, longs;
        for (auto &sq : good) (split_len > 0 && sq.len >= split_len ? longs : shorts).push_back(sq);
        if (!longs.empty() && !shorts.empty()) {
            b.lane[0].push_back(Job{longs, est_of(longs), 0});      // the long tail starts first
            b.lane[1].push_back(Job{shorts, est_of(shorts), 0});
        } else if (!good.empty())
            b.lane[good.size() >= 256 ? 1 : 0].push_back(Job{good, est_of(good), 0});
    }
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

static int wait_job(rafft_job *job, rafft_result **out_)
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

int rafft_fold_submit(const rafft_params *p, int n_seq, const char *const *seqs, const int *lens, int device, rafft_job **job)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return submit_locked(p, n_seq, seqs, lens, device, job);
}

int rafft_fold_wait(rafft_job *job, rafft_result **out) { return wait_job(job, out); }

int rafft_fold_batch(const rafft_params *p, int n_seq, const char *const *seqs, const int *lens, int device, rafft_result **out_)
{
    if (!out_) return fail(RAFFT_ERR_PARAM, "null argument");
    *out_ = nullptr;
    rafft_job *job = nullptr;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        if (int rc = submit_locked(p, n_seq, seqs, lens, device, &job, false)) return rc;      // (this caller cannot be streaming: no linger)
    }
    return wait_job(job, out_);
}

void rafft_free_result(rafft_result *r)
{
    if (r && r->_owner) free_out((HostOut *)r->_owner);
}

int rafft_get_stats(rafft_stats *o)
{
    if (!o) return RAFFT_ERR_PARAM;
    std::lock_guard<std::mutex> lk(g.mu);
    *o = g.stats;
    return 0;
}

static int parse_db(const char *seq, const char *db, int L, std::vector<int16_t> &pt)
{
    pt.assign(L, -1);
    std::vector<int> stk;
    for (int i = 0; i < L; i++) {
        if (db[i] == '(') stk.push_back(i);
        else if (db[i] == ')') {
            if (stk.empty()) return RAFFT_ERR_STRUCT;
            int j = stk.back(); stk.pop_back();
            pt[i] = (int16_t)j; pt[j] = (int16_t)i;
        } else if (db[i] != '.') return RAFFT_ERR_STRUCT;
    }
    return stk.empty() ? 0 : RAFFT_ERR_STRUCT;
}

static thread_local bool g_ws_locked_by_me = false;     // rafft_expand_node holds ws_mu across its nested evaluation

static int eval_structures_impl(int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out, double temp = 37.0, int *guessed_out = nullptr)
{
    if (int rc = init_ctx(-1)) return rc;
    drain();                                   // (g.mu is held: nothing new is submitted meanwhile)
    std::unique_lock<std::mutex> ws_lk(g.ws_mu, std::defer_lock);
    if (!g_ws_locked_by_me) ws_lk.lock();
    if (int rc = ensure_tables(temp)) return rc;
    if (int rc = init_ws(g.ws[0])) return rc;
    std::vector<long long> off(n);
    std::vector<int> len(n), status(n, 0);
    long long tot = 0;
    for (int i = 0; i < n; i++) {
        len[i] = (int)strlen(seqs[i]);
        off[i] = tot;
        if ((int)strlen(dbs[i]) != len[i] || len[i] > RAFFT_MAX_LEN) { status[i] = RAFFT_ERR_STRUCT; len[i] = 0; }      // (16-bit pair tables: positions 0..32767)
        tot += len[i];
    }
    std::vector<uint8_t> codes(tot + 16, 0);
    std::vector<int16_t> pts(tot + 16, -1);
    for (int i = 0; i < n; i++) {
        if (status[i]) continue;
        std::vector<int16_t> pt;
        if (parse_db(seqs[i], dbs[i], len[i], pt)) { status[i] = RAFFT_ERR_STRUCT; len[i] = 0; continue; }
        for (int x = 0; x < len[i]; x++) {
            char ch = seqs[i][x];
            int c = ch == 'A' ? 1 : ch == 'C' ? 2 : ch == 'G' ? 3 : ch == 'U' ? 4 : ch == 'N' ? 0 : -1;
            if (c < 0) { status[i] = RAFFT_ERR_BAD_CHAR; break; }
            codes[off[i] + x] = (uint8_t)c;
            pts[off[i] + x] = pt[x];
        }
        if (status[i]) len[i] = 0;
    }
    struct DevMem {      // the call's device buffers: freed on every way out
        void *p[7] = {};
        ~DevMem() { for (void *q : p) if (q) { hipError_t fe = hipFree(q); (void)fe; } }
    } mem;
    void *&dc = mem.p[0], *&dp = mem.p[1], *&doff = mem.p[2], *&dlen = mem.p[3], *&dout = mem.p[4], *&dst = mem.p[5], *&dg = mem.p[6];
    HIPCHK(hipMalloc(&dc, tot + 16)); HIPCHK(hipMalloc(&dp, (tot + 16) * 2)); HIPCHK(hipMalloc(&doff, n * 8 + 8));
    HIPCHK(hipMalloc(&dlen, n * 4 + 4)); HIPCHK(hipMalloc(&dout, n * 4 + 4)); HIPCHK(hipMalloc(&dst, n * 4 + 4)); HIPCHK(hipMalloc(&dg, n * 4 + 4));
    HIPCHK(hipMemcpy(dc, codes.data(), tot + 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dp, pts.data(), (tot + 16) * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(doff, off.data(), n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dlen, len.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_kernel, dim3(n), dim3(64), 0, g.ws[0].stream, g.T, n, (const uint8_t *)dc, (const int16_t *)dp,
                       (const long long *)doff, (const int *)dlen, (int *)dout, (int *)dst, (int *)dg);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.ws[0].stream));
    std::vector<int> st2(n);
    HIPCHK(hipMemcpy(dcal_out, dout, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(st2.data(), dst, n * 4, hipMemcpyDeviceToHost));
    if (guessed_out) HIPCHK(hipMemcpy(guessed_out, dg, n * 4, hipMemcpyDeviceToHost));
    if (guessed_out) for (int i = 0; i < n; i++) if (status[i] || st2[i]) guessed_out[i] = 0;      // (a row with an error has no energy to qualify)
    int worst = 0;
    for (int i = 0; i < n; i++) {
        int s = status[i] ? status[i] : st2[i];
        if (status_out) status_out[i] = s;
        if (s && !worst) worst = s;
    }
    if (worst && !status_out) return fail(worst, "malformed structure, bad character or non-canonical pair");
    return 0;
}

int rafft_eval_structures(int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return eval_structures_impl(n, seqs, dbs, dcal_out, status_out);
}

int rafft_eval_structure(const char *seq, const char *db, int *dcal_out)
{
    return rafft_eval_structures(1, &seq, &db, dcal_out, nullptr);
}

int rafft_eval_structures_at(double temp, int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return eval_structures_impl(n, seqs, dbs, dcal_out, status_out, temp);
}

int rafft_eval_structures_info(int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out, int *guessed_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return eval_structures_impl(n, seqs, dbs, dcal_out, status_out, 37.0, guessed_out);
}

int rafft_params_unpinned(int counts[3])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!counts) return fail(RAFFT_ERR_PARAM, "null argument");
    counts[0] = counts[1] = counts[2] = 0;
    if (param_set().builtin_set) rafft_par::builtin_unpinned_counts(counts);
    return 0;
}

// ---- energy parameters (no GPU needed to load, inspect or save a parameter set; the upload happens with the next fold)

static int set_params_from_text(const std::string &text, const std::string &source)
{
    std::unique_ptr<rafft_par::ParamSet> P(new rafft_par::ParamSet());
    std::string err;
    if (!rafft_par::parse(text, *P, err)) return fail(RAFFT_ERR_PARAM, "parameter file " + source + ": " + err);
    P->source = source;
    {   // every table must survive the conversion to the device layout at 37 C
        std::unique_ptr<EnergyTables> h(new EnergyTables());
        if (!rafft_par::scaled_tables(*P, 37.0, h.get(), err)) return fail(RAFFT_ERR_PARAM, "parameter file " + source + ": " + err);
    }
    delete g.P;
    g.P = P.release();
    g.T_dirty = true;
    return 0;
}

int rafft_load_params(const char *path)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!path) return fail(RAFFT_ERR_PARAM, "null path");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(RAFFT_ERR_PARAM, std::string("cannot open parameter file ") + path);
    std::string text;
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, k);
    fclose(f);
    return set_params_from_text(text, path);
}

int rafft_load_params_text(const char *text, const char *source_name)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!text) return fail(RAFFT_ERR_PARAM, "null text");
    return set_params_from_text(text, source_name ? source_name : "<memory>");
}

int rafft_reset_params(void)
{
    std::lock_guard<std::mutex> lk(g.mu);
    delete g.P;
    g.P = nullptr;
    g.T_dirty = true;
    return 0;
}

int rafft_save_params(const char *path)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!path) return fail(RAFFT_ERR_PARAM, "null path");
    const std::string txt = rafft_par::format(param_set());
    FILE *f = fopen(path, "wb");
    if (!f) return fail(RAFFT_ERR_PARAM, std::string("cannot write ") + path);
    const bool ok = fwrite(txt.data(), 1, txt.size(), f) == txt.size();
    fclose(f);
    return ok ? 0 : fail(RAFFT_ERR_PARAM, std::string("short write to ") + path);
}

int rafft_params_info(char *source, int source_cap, int *has_enthalpies)
{
    std::lock_guard<std::mutex> lk(g.mu);
    const rafft_par::ParamSet &P = param_set();
    if (source && source_cap > 0) { strncpy(source, P.source.c_str(), (size_t)source_cap - 1); source[source_cap - 1] = 0; }
    if (has_enthalpies) *has_enthalpies = P.has_dH ? 1 : 0;
    return 0;
}

// The 37 C value of one table entry of the current parameter set, by ViennaRNA table name and flat row-major index in
// ViennaRNA's own array shape (pairs 0..7, bases 0..4): lets a caller check what a file gave without a GPU.
int rafft_param_value(const char *table, int enthalpy, long index, int *value_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    const rafft_par::ParamSet &P = param_set();
    if (!table || !value_out) return fail(RAFFT_ERR_PARAM, "null argument");
    const int w = enthalpy ? 1 : 0;
    struct Ent { const char *n; const int *p; long cnt; };
    const Ent ents[] = {
        {"stack", &P.stack[w][0][0], 64}, {"hairpin", P.hairpin[w], 31}, {"bulge", P.bulge[w], 31}, {"interior", P.interior[w], 31},
        {"mismatch_hairpin", &P.mmH[w][0][0][0], 200}, {"mismatch_interior", &P.mmI[w][0][0][0], 200},
        {"mismatch_interior_1n", &P.mm1n[w][0][0][0], 200}, {"mismatch_interior_23", &P.mm23[w][0][0][0], 200},
        {"mismatch_multi", &P.mmM[w][0][0][0], 200}, {"mismatch_exterior", &P.mmE[w][0][0][0], 200},
        {"dangle5", &P.d5[w][0][0], 40}, {"dangle3", &P.d3[w][0][0], 40},
        {"int11", &P.int11[w][0][0][0][0], 8 * 8 * 25}, {"int21", &P.int21[w][0][0][0][0][0], 8 * 8 * 125},
        {"int22", &P.int22[w][0][0][0][0][0][0], 8 * 8 * 625},
        {"ninio", &P.ninio[w], 1}, {"ml_base", &P.ml_base[w], 1}, {"ml_closing", &P.ml_closing[w], 1}, {"ml_intern", &P.ml_intern[w], 1},
        {"terminal_au", &P.term_au[w], 1}, {"max_ninio", &P.max_ninio, 1}};
    for (const Ent &e : ents)
        if (!strcmp(e.n, table)) {
            if (index < 0 || index >= e.cnt) return fail(RAFFT_ERR_PARAM, "index out of range");
            *value_out = e.p[index];
            return 0;
        }
    return fail(RAFFT_ERR_PARAM, std::string("unknown table ") + table);
}

int rafft_expand_node(const rafft_params *p, const char *seq, const char *db, const int *pos, int n,
                      int *n_ranked, int *lag, double *corval, int *nb, int *mi, int *mj,
                      double *score, int *ddcal, int *n_kept, int *kept)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (int rc = init_ctx(-1)) return rc;
    drain();
    std::lock_guard<std::mutex> ws_lk(g.ws_mu);
    struct Flag { Flag() { g_ws_locked_by_me = true; } ~Flag() { g_ws_locked_by_me = false; } } flag_;
    const int L = (int)strlen(seq);
    if (L == 0 || L > RAFFT_MAX_LEN || n < 1 || n > L) return fail(RAFFT_ERR_PARAM, "bad node");
    std::vector<int16_t> pt;
    if (parse_db(seq, db, L, pt)) return fail(RAFFT_ERR_STRUCT, "malformed dot-bracket");
    // enclosing loop of the region: nearest pair (i,j) with i < pos[0] < j
    int ci = -1, cj = L;
    for (int x = pos[0] - 1, depth = 0; x >= 0; x--) {
        if (pt[x] < 0) continue;
        if (pt[x] < x) { depth++; continue; }
        if (depth > 0) { depth--; continue; }
        if (pt[x] > pos[0]) { ci = x; cj = pt[x]; break; }
    }
    SeamIn sm;
    sm.ci = ci; sm.cj = cj;
    for (int x = ci + 1; x < cj;) {            // branch helices hanging in that loop
        if (pt[x] < 0) { x++; continue; }
        sm.br.push_back((uint32_t)x | ((uint32_t)pt[x] << 16));
        x = pt[x] + 1;
    }
    sm.pos.assign(pos, pos + n);
    int par_dcal = 0;
    if (int rc = eval_structures_impl(1, &seq, &db, &par_dcal, nullptr, p->temp)) return rc;   // (also scales the tables for p->temp)
    sm.pdcal = par_dcal;
    const int K = std::max(1, std::min(p->nb_mode, 2 * n - 1));
    if (int rc = ensure(g.ws[0].dbg, (size_t)K * (4 * 7 + 8 * 2) + 64)) return rc;
    char *b = (char *)g.ws[0].dbg.p;
    DebugOut &dbg = sm.dbg;
    dbg.n_ranked = (int *)b; b += 16;
    dbg.lag = (int *)b; b += 4 * K; dbg.nb = (int *)b; b += 4 * K; dbg.mi = (int *)b; b += 4 * K; dbg.mj = (int *)b; b += 4 * K;
    dbg.ddcal = (int *)b; b += 4 * K; dbg.kept = (int *)b; b += 4 * K;
    b = (char *)(((uintptr_t)b + 15) & ~(uintptr_t)15);
    dbg.corval = (double *)b; b += 8 * K; dbg.score = (double *)b;
    std::vector<SeqIn> one{{seq, L, 0, 0}};
    HostOut ho;
    ho.seq.resize(1); ho.step_size.resize(1); ho.step_off.resize(1); ho.one_size.assign(1, 0); ho.one_off.assign(1, 0); ho.dcal_ptr.assign(1, nullptr); ho.db_ptr.assign(1, nullptr);
    Batch bt;                                  // a private batch: the scheduler is idle (drained above) and g.mu is held
    bt.p = *p;
    bt.cfg = read_config();
    bt.p.max_stack = std::max(1, bt.p.max_stack);
    bt.n_seq = 1; bt.ho = &ho;
    const int src = run_seam(bt, one, sm);
    for (hipEvent_t e : bt.events) g.ev_free.push_back(e);
    if (src) return src;
    int hdr[4];
    HIPCHK(hipMemcpy(hdr, dbg.n_ranked, 16, hipMemcpyDeviceToHost));
    *n_ranked = hdr[0]; *n_kept = hdr[1];
    int r = hdr[0];
    HIPCHK(hipMemcpy(lag, dbg.lag, 4 * r, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nb, dbg.nb, 4 * r, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mi, dbg.mi, 4 * r, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mj, dbg.mj, 4 * r, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ddcal, dbg.ddcal, 4 * r, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kept, dbg.kept, 4 * hdr[1], hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(corval, dbg.corval, 8 * r, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(score, dbg.score, 8 * r, hipMemcpyDeviceToHost));
    return 0;
}

// ---- kinetics on the fast-folding graph

int rafft_kin_rate_matrix(int n_steps, const int *step_size, int L, const char *rows, const int *uid, int n_unique,
                          const double *energy, double kt, double *rate_device)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!step_size || !rows || !uid || !energy || !rate_device || n_steps < 1 || L < 1 || L > 32767 || n_unique < 1 || !(kt > 0))
        return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = init_ctx(-1)) return rc;
    // like the other seam calls: no fold in flight (hipMalloc / hipFree below synchronise the device, and the matrix is
    // written on the library's stream - the caller hands over a buffer its own stream is done with), workspace 0 held
    drain();
    std::lock_guard<std::mutex> ws_lk(g.ws_mu);
    if (int rc = init_ws(g.ws[0])) return rc;
    long long n = 0;
    std::vector<int> row0(n_steps);
    for (int i = 0; i < n_steps; i++) { row0[i] = (int)n; n += step_size[i]; if (step_size[i] < 0) return fail(RAFFT_ERR_PARAM, "negative step size"); }
    if (n < 1 || n > 0x7fffffff) return fail(RAFFT_ERR_PARAM, "bad number of structures");
    for (long long r = 0; r < n; r++) if (uid[r] < 0 || uid[r] >= n_unique) return fail(RAFFT_ERR_PARAM, "uid out of range");
    hipStream_t st = g.ws[0].stream;
    void *d_rows = nullptr, *d_pt = nullptr, *d_stack = nullptr, *d_uid = nullptr, *d_en = nullptr, *d_bad = nullptr;
    auto cleanup = [&]() { for (void *q : {d_rows, d_pt, d_stack, d_uid, d_en, d_bad}) if (q) { hipError_t fe = hipFree(q); (void)fe; } };
#define KCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(); return fail(RAFFT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } } while (0)
    KCHK(hipMalloc(&d_rows, (size_t)n * L)); KCHK(hipMalloc(&d_pt, (size_t)n * L * 2)); KCHK(hipMalloc(&d_stack, (size_t)n * L * 2));
    KCHK(hipMalloc(&d_uid, (size_t)n * 4)); KCHK(hipMalloc(&d_en, (size_t)n_unique * 8)); KCHK(hipMalloc(&d_bad, 4));
    KCHK(hipMemcpyAsync(d_rows, rows, (size_t)n * L, hipMemcpyHostToDevice, st));
    KCHK(hipMemcpyAsync(d_uid, uid, (size_t)n * 4, hipMemcpyHostToDevice, st));
    KCHK(hipMemcpyAsync(d_en, energy, (size_t)n_unique * 8, hipMemcpyHostToDevice, st));
    KCHK(hipMemsetAsync(d_bad, 0, 4, st));
    KCHK(hipMemsetAsync(rate_device, 0, (size_t)n_unique * n_unique * 8, st));
    hipLaunchKernelGGL(kin_pair_table_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (int)n, L, (const char *)d_rows,
                       (int16_t *)d_pt, (int16_t *)d_stack, (int *)d_bad);
    KCHK(hipGetLastError());
    for (int i = 0; i < n_steps; i++) {
        const int pi = i == 0 ? n_steps - 1 : i - 1;      // the reference compares step 0 with the LAST step (fast_paths[-1], rafft_kin.py:75)
        if (!step_size[i] || !step_size[pi]) continue;
        hipLaunchKernelGGL(kin_rates_kernel, dim3((unsigned)step_size[i]), dim3(KIN_NT), (size_t)L * 2, st, L, (const int16_t *)d_pt,
                           row0[i], step_size[pi], row0[pi], (const int *)d_uid, (const double *)d_en, kt, n_unique, rate_device);
        KCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(kin_diag_kernel, dim3((unsigned)n_unique), dim3(256), 0, st, n_unique, rate_device);
    KCHK(hipGetLastError());
    int bad = 0;
    KCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    KCHK(hipStreamSynchronize(st));
#undef KCHK
    cleanup();
    if (bad) return fail(RAFFT_ERR_STRUCT, "malformed dot-bracket row");
    return 0;
}

// ---- folding landscape (kernels in rafft_landscape.hip)

static long long g_landscape_counters[4];      // MDS calls, SMACOF passes enqueued, host read-backs of the `done` words, passes of the last call
#define LANDSCAPE_CHUNK 64                     // SMACOF passes enqueued between two read-backs

int rafft_landscape_distances(int n, int L, const char *rows, uint16_t *dist_device)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!rows || !dist_device || n < 1 || L < 1 || L > 32767) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = init_ctx(-1)) return rc;
    drain();
    std::lock_guard<std::mutex> ws_lk(g.ws_mu);
    if (int rc = init_ws(g.ws[0])) return rc;
    hipStream_t st = g.ws[0].stream;
    const int Lp = (L + LS_CHUNK - 1) / LS_CHUNK * LS_CHUNK;
    void *d_rows = nullptr, *d_pt = nullptr, *d_stack = nullptr, *d_open = nullptr, *d_np = nullptr, *d_bad = nullptr;
    auto cleanup = [&]() { for (void *q : {d_rows, d_pt, d_stack, d_open, d_np, d_bad}) if (q) { hipError_t fe = hipFree(q); (void)fe; } };
#define KCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(); return fail(RAFFT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } } while (0)
    KCHK(hipMalloc(&d_rows, (size_t)n * L)); KCHK(hipMalloc(&d_pt, (size_t)n * L * 2)); KCHK(hipMalloc(&d_stack, (size_t)n * L * 2));
    KCHK(hipMalloc(&d_open, (size_t)n * Lp * 2)); KCHK(hipMalloc(&d_np, (size_t)n * 4)); KCHK(hipMalloc(&d_bad, 4));
    KCHK(hipMemcpyAsync(d_rows, rows, (size_t)n * L, hipMemcpyHostToDevice, st));
    KCHK(hipMemsetAsync(d_bad, 0, 4, st));
    hipLaunchKernelGGL(kin_pair_table_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, L, (const char *)d_rows,
                       (int16_t *)d_pt, (int16_t *)d_stack, (int *)d_bad);
    KCHK(hipGetLastError());
    int bad = 0;
    KCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    KCHK(hipStreamSynchronize(st));
    if (bad) { cleanup(); return fail(RAFFT_ERR_STRUCT, "malformed dot-bracket row"); }
    hipLaunchKernelGGL(landscape_open_table_kernel, dim3((unsigned)n), dim3(64), 0, st, n, L, Lp, (const int16_t *)d_pt, (uint16_t *)d_open, (int *)d_np);
    KCHK(hipGetLastError());
    const unsigned T = (unsigned)((n + LS_TILE - 1) / LS_TILE);
    if (T > 65535) { cleanup(); return fail(RAFFT_ERR_PARAM, "too many structures"); }
    hipLaunchKernelGGL(landscape_distance_kernel, dim3(T, T), dim3(256), 0, st, n, Lp, (const uint16_t *)d_open, (const int *)d_np, dist_device);
    KCHK(hipGetLastError());
    KCHK(hipStreamSynchronize(st));
    cleanup();
    return 0;
}

int rafft_landscape_mds(int n, const uint16_t *dist_device, int n_init, const double *x_init, int max_iter, double eps,
                        double *x_device, double *stress_out, int *n_iter_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!dist_device || !x_init || !x_device || !stress_out || !n_iter_out || n < 1 || n_init < 1 || n_init > 65535 || max_iter < 1 || !(eps == eps))
        return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = init_ctx(-1)) return rc;
    drain();
    std::lock_guard<std::mutex> ws_lk(g.ws_mu);
    if (int rc = init_ws(g.ws[0])) return rc;
    hipStream_t st = g.ws[0].stream;
    void *d_x = nullptr, *d_rs = nullptr, *d_state = nullptr;
    auto cleanup = [&]() { for (void *q : {d_x, d_rs, d_state}) if (q) { hipError_t fe = hipFree(q); (void)fe; } };
    const size_t per = (size_t)n * 2 * sizeof(double);            // one configuration
    KCHK(hipMalloc(&d_x, per * 2 * n_init)); KCHK(hipMalloc(&d_rs, per * n_init)); KCHK(hipMalloc(&d_state, sizeof(LandscapeMdsState) * n_init));
    KCHK(hipMemsetAsync(d_state, 0, sizeof(LandscapeMdsState) * n_init, st));
    for (int k = 0; k < n_init; k++)                               // X_0 of start k -> its buffer 0
        KCHK(hipMemcpyAsync((char *)d_x + per * 2 * k, x_init + (size_t)k * n * 2, per, hipMemcpyHostToDevice, st));
    // X in LDS up to 128 KiB (8192 points, one workgroup per CU); beyond that it is read through the caches
    const size_t lds = (size_t)n * 16;
    const bool xlds = lds <= ((size_t)128 << 10);
    static bool lds_attr_set = false;
    if (xlds && !lds_attr_set) {
        KCHK(hipFuncSetAttribute((const void *)landscape_smacof_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 << 10));
        lds_attr_set = true;
    }
    const int rows_per_wg = LS_SM_NT / 64;
    int gx = (n + rows_per_wg - 1) / rows_per_wg;
    const int cap = g.n_cu / n_init > 0 ? g.n_cu / n_init : 1;    // one workgroup per CU over all starts when X fills the LDS
    if (gx > cap) gx = cap;
    std::vector<LandscapeMdsState> hs(n_init);
    g_landscape_counters[0]++;
    g_landscape_counters[3] = 0;
    bool all_done = false;
    for (int pass = 0; pass <= max_iter && !all_done; ) {
        const int stop = pass + LANDSCAPE_CHUNK < max_iter + 1 ? pass + LANDSCAPE_CHUNK : max_iter + 1;
        for (; pass < stop; pass++) {
            const int guttman = pass < max_iter;
            if (xlds)
                hipLaunchKernelGGL(landscape_smacof_kernel<true>, dim3((unsigned)gx, (unsigned)n_init), dim3(LS_SM_NT), lds, st, n, dist_device, (double *)d_x,
                                   (double *)d_rs, (const LandscapeMdsState *)d_state, pass, guttman);
            else
                hipLaunchKernelGGL(landscape_smacof_kernel<false>, dim3((unsigned)gx, (unsigned)n_init), dim3(LS_SM_NT), 0, st, n, dist_device, (double *)d_x,
                                   (double *)d_rs, (const LandscapeMdsState *)d_state, pass, guttman);
            hipLaunchKernelGGL(landscape_smacof_finalize_kernel, dim3((unsigned)n_init), dim3(256), 0, st, n, (const double *)d_x, (const double *)d_rs,
                               (LandscapeMdsState *)d_state, pass, max_iter, eps, x_device);
            g_landscape_counters[1]++; g_landscape_counters[3]++;
        }
        KCHK(hipGetLastError());
        KCHK(hipMemcpyAsync(hs.data(), d_state, sizeof(LandscapeMdsState) * n_init, hipMemcpyDeviceToHost, st));
        KCHK(hipStreamSynchronize(st));
        g_landscape_counters[2]++;
        all_done = true;
        for (int k = 0; k < n_init; k++) all_done = all_done && hs[k].done;
    }
    cleanup();
    if (!all_done) return fail(RAFFT_ERR_HIP, "internal: SMACOF did not finish within max_iter + 1 passes");
    for (int k = 0; k < n_init; k++) { stress_out[k] = hs[k].stress; n_iter_out[k] = hs[k].n_iter; }
    return 0;
}

int rafft_landscape_surface(int n, const double *x_device, const double *w_device, int grid, double lo, double hi, double *z_device,
                            double *phi_device)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!x_device || n < 1 || (!z_device && !phi_device) || (z_device && (!w_device || grid < 1 || grid > 32768 || !(lo <= hi))))
        return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = init_ctx(-1)) return rc;
    drain();
    std::lock_guard<std::mutex> ws_lk(g.ws_mu);
    if (int rc = init_ws(g.ws[0])) return rc;
    hipStream_t st = g.ws[0].stream;
    if (phi_device) {
        if (n > 65535) return fail(RAFFT_ERR_PARAM, "too many structures");
        hipLaunchKernelGGL(landscape_tps_fill_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, st, n, x_device, phi_device);
        HIPCHK(hipGetLastError());
    }
    if (z_device) {
        const long long pts = (long long)grid * grid;
        hipLaunchKernelGGL(landscape_tps_kernel, dim3((unsigned)((pts + 255) / 256)), dim3(256), 0, st, n, x_device, w_device, grid, lo, hi, z_device);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
#undef KCHK

int rafft_landscape_counters(long long out[4])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < 4; k++) out[k] = g_landscape_counters[k];
    return 0;
}

// ---- accuracy scoring (kernels in rafft_score.hip)

// device buffers of the scoring calls: grow-only and kept for the life of the process (a call on a warm library allocates nothing).
// Unlike the workspaces they are not trimmed when the library idles: after the biggest call so far they hold its rows, its row
// records and, for sequences beyond the LDS plans, up to 1024 workgroups' scratch (tens of MB at the benchmark's sizes).
static struct { Buf rows, known, seqs, items, row_out, seq_out, scratch; } g_score;

// the known structure's table as rafft/utils.py:53-67 pairs it: ( and < share a stack, [ has its own; 1-based partners, 0 = unpaired
static bool score_known_table(const char *db, int L, uint16_t *t, int *n_known, std::string &err)
{
    const size_t n = strlen(db);
    if (n != (size_t)L) { err = "known structure of length " + std::to_string(n) + " for a sequence of length " + std::to_string(L); return false; }
    std::vector<int> reg, pk;
    int pairs = 0;
    for (int i = 0; i < L; i++) {
        const char c = db[i];
        t[i] = 0;
        if (c == '(' || c == '<') reg.push_back(i);
        else if (c == '[') pk.push_back(i);
        else if (c == ')' || c == '>' || c == ']') {
            std::vector<int> &stk = c == ']' ? pk : reg;
            if (stk.empty()) { err = std::string("known structure: unmatched '") + c + "' at position " + std::to_string(i); return false; }
            const int j = stk.back(); stk.pop_back();
            t[i] = (uint16_t)(j + 1); t[j] = (uint16_t)(i + 1);
            pairs++;
        } else if (c != '.') { err = std::string("known structure: character '") + c + "' at position " + std::to_string(i); return false; }
    }
    if (!reg.empty() || !pk.empty()) { err = "known structure: unclosed bracket at position " + std::to_string(!reg.empty() ? reg.back() : pk.back()); return false; }
    *n_known = pairs;
    return true;
}

struct ScoreSrc { const char *base; size_t bytes; size_t dev_off; };      // a host range of rows that goes to the device as it lies

// rows_off[s]: where sequence s's first row lies in the device copy of `src`; pre_status[s] != 0: the sequence is not scored
static int score_impl(int n_seq, const int *lens, const int *n_rows, const int *stride, const unsigned long long *rows_off, const int *pre_status,
                      const std::vector<ScoreSrc> &src, size_t rows_bytes, const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out)
{
    std::lock_guard<std::mutex> ws_lk(g.ws_mu);
    if (int rc = init_ws(g.ws[0])) return rc;
    hipStream_t st = g.ws[0].stream;
    std::vector<ScoreSeq> seqs(n_seq);
    std::vector<uint16_t> ktab;
    std::vector<ScoreItem> items[3];
    int Lc[3] = {2, 2, 2};
    long long total_rows = 0;
    std::string first_err;
    for (int s = 0; s < n_seq; s++) {
        ScoreSeq &q = seqs[s];
        q = ScoreSeq{};
        q.rows_off = rows_off[s]; q.L = lens[s]; q.n_rows = n_rows[s]; q.stride = stride[s]; q.row0 = (int)total_rows;
        q.status = pre_status ? pre_status[s] : 0;
        total_rows += n_rows[s];
        if (total_rows > 0x7fffffff) return fail(RAFFT_ERR_PARAM, "too many rows");
        if (q.status) continue;
        const size_t o = ktab.size();
        if (o + (size_t)q.L > 0xffffffffull) return fail(RAFFT_ERR_PARAM, "known structures too long in total");
        ktab.resize(o + (size_t)q.L);
        std::string err;
        if (!score_known_table(known[s], q.L, ktab.data() + o, &q.n_known, err)) {
            ktab.resize(o);
            q.status = RAFFT_ERR_STRUCT; q.n_known = 0;
            if (first_err.empty()) first_err = "sequence " + std::to_string(s) + ": " + err;
            continue;
        }
        q.known_off = (unsigned)o;
        const int cls = q.L <= SC_L_SMALL ? 0 : q.L <= SC_L_LDS ? 1 : 2;
        Lc[cls] = std::max(Lc[cls], (q.L + 1) & ~1);
        for (int r0 = 0; r0 < q.n_rows; r0 += SC_ROWS) items[cls].push_back(ScoreItem{s, r0, std::min(r0 + SC_ROWS, q.n_rows)});
    }
    if (n_seq == 0) return 0;
    std::vector<ScoreItem> all;
    size_t item0[3];
    for (int c = 0; c < 3; c++) { item0[c] = all.size(); all.insert(all.end(), items[c].begin(), items[c].end()); }
    const unsigned grid2 = (unsigned)std::min<size_t>(items[2].size(), 1024);
    const size_t scratch_bytes = (size_t)grid2 * SC_WAVES * (size_t)(Lc[2] + Lc[2] / 2) * 2;
    if (int rc = ensure(g_score.rows, rows_bytes + 64)) return rc;
    if (int rc = ensure(g_score.known, ktab.size() * 2 + 64)) return rc;
    if (int rc = ensure(g_score.seqs, seqs.size() * sizeof(ScoreSeq))) return rc;
    if (int rc = ensure(g_score.items, all.size() * sizeof(ScoreItem) + 64)) return rc;
    if (int rc = ensure(g_score.row_out, (size_t)total_rows * sizeof(rafft_score_row) + 64)) return rc;
    if (int rc = ensure(g_score.seq_out, seqs.size() * sizeof(rafft_score_seq))) return rc;
    if (int rc = ensure(g_score.scratch, scratch_bytes + 64)) return rc;
    for (const ScoreSrc &x : src)
        if (x.bytes) HIPCHK(hipMemcpyAsync((char *)g_score.rows.p + x.dev_off, x.base, x.bytes, hipMemcpyHostToDevice, st));
    if (!ktab.empty()) HIPCHK(hipMemcpyAsync(g_score.known.p, ktab.data(), ktab.size() * 2, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g_score.seqs.p, seqs.data(), seqs.size() * sizeof(ScoreSeq), hipMemcpyHostToDevice, st));
    if (!all.empty()) HIPCHK(hipMemcpyAsync(g_score.items.p, all.data(), all.size() * sizeof(ScoreItem), hipMemcpyHostToDevice, st));
    if (total_rows) HIPCHK(hipMemsetAsync(g_score.row_out.p, 0, (size_t)total_rows * sizeof(rafft_score_row), st));
    for (int c = 0; c < 3; c++) {
        if (items[c].empty()) continue;
        const ScoreItem *it = (const ScoreItem *)g_score.items.p + item0[c];
        if (c < 2)
            hipLaunchKernelGGL(score_rows_kernel<true>, dim3((unsigned)std::min<size_t>(items[c].size(), (size_t)1 << 20)), dim3(SC_NT), (size_t)14 * Lc[c], st,
                               (int)items[c].size(), it, (const ScoreSeq *)g_score.seqs.p, (const char *)g_score.rows.p, (const uint16_t *)g_score.known.p, Lc[c],
                               (uint16_t *)nullptr, (rafft_score_row *)g_score.row_out.p);
        else
            hipLaunchKernelGGL(score_rows_kernel<false>, dim3(grid2), dim3(SC_NT), 0, st,
                               (int)items[c].size(), it, (const ScoreSeq *)g_score.seqs.p, (const char *)g_score.rows.p, (const uint16_t *)g_score.known.p, Lc[c],
                               (uint16_t *)g_score.scratch.p, (rafft_score_row *)g_score.row_out.p);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(score_pick_kernel, dim3((unsigned)((n_seq + SC_WAVES - 1) / SC_WAVES)), dim3(SC_NT), 0, st, n_seq, (const ScoreSeq *)g_score.seqs.p,
                       (const rafft_score_row *)g_score.row_out.p, (rafft_score_seq *)g_score.seq_out.p);
    HIPCHK(hipGetLastError());
    if (row_out && total_rows) HIPCHK(hipMemcpyAsync(row_out, g_score.row_out.p, (size_t)total_rows * sizeof(rafft_score_row), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(seq_out, g_score.seq_out.p, seqs.size() * sizeof(rafft_score_seq), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (row_out)
        for (int s = 0; s < n_seq; s++)
            if (seqs[s].status)
                for (int r = 0; r < seqs[s].n_rows; r++) row_out[(size_t)seqs[s].row0 + r].status = seqs[s].status;
    g_err = first_err;
    return 0;
}

// rows of every sequence packed into one host buffer (strides kept): rows that lie anywhere in pageable memory
static void score_pack(int n_seq, const int *lens, const int *n_rows, const char *const *rows, const int *stride, const int *pre_status,
                       std::vector<char> &pack, std::vector<unsigned long long> &rows_off)
{
    size_t tot = 0;
    for (int s = 0; s < n_seq; s++) {
        rows_off[s] = tot;
        if (n_rows[s] && !(pre_status && pre_status[s])) tot += (size_t)(n_rows[s] - 1) * stride[s] + lens[s];
    }
    pack.resize(tot);
    for (int s = 0; s < n_seq; s++) {
        const size_t end = s + 1 < n_seq ? rows_off[s + 1] : tot;
        if (end > rows_off[s]) memcpy(pack.data() + rows_off[s], rows[s], end - rows_off[s]);
    }
}

int rafft_score_rows(int n_seq, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                     const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || (n_seq > 0 && (!lens || !n_rows || !rows || !row_stride || !known || !seq_out))) return fail(RAFFT_ERR_PARAM, "bad argument");
    for (int s = 0; s < n_seq; s++) {
        if (lens[s] < 0 || lens[s] > 32767) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": length outside 0..32767");
        if (n_rows[s] < 0) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": negative number of rows");
        if (row_stride[s] < lens[s]) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": row stride below the length");
        if (!known[s] || (n_rows[s] && !rows[s])) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": null pointer");
    }
    if (int rc = init_ctx(-1)) return rc;
    drain();
    std::vector<char> pack;
    std::vector<unsigned long long> rows_off(n_seq);
    score_pack(n_seq, lens, n_rows, rows, row_stride, nullptr, pack, rows_off);
    std::vector<ScoreSrc> src{ScoreSrc{pack.data(), pack.size(), 0}};
    return score_impl(n_seq, lens, n_rows, row_stride, rows_off.data(), nullptr, src, pack.size(), known, row_out, seq_out);
}

int rafft_score_result(const rafft_result *r, const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!r || r->n_seq < 0 || (r->n_seq > 0 && (!r->seq || !known || !seq_out))) return fail(RAFFT_ERR_PARAM, "bad argument");
    const int n_seq = r->n_seq;
    std::vector<int> lens(n_seq), n_rows(n_seq), stride(n_seq), pre(n_seq);
    std::vector<const char *> rows(n_seq);
    for (int s = 0; s < n_seq; s++) {
        const rafft_seq_result &sr = r->seq[s];
        pre[s] = sr.status;
        if (sr.status) { lens[s] = n_rows[s] = stride[s] = 0; rows[s] = nullptr; continue; }
        if (sr.length < 0 || sr.length > 32767) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": length outside 0..32767");
        if (!known[s]) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": null pointer");
        const int last = sr.n_steps - 1;
        lens[s] = sr.length; stride[s] = sr.length + 1;
        n_rows[s] = last >= 0 ? sr.step_size[last] : 0;
        rows[s] = n_rows[s] ? sr.db + (size_t)sr.step_off[last] * (size_t)(sr.length + 1) : nullptr;
    }
    if (int rc = init_ctx(-1)) return rc;
    drain();
    // the rows lie in the pinned chunks the fold's copies landed in: per chunk, the range the final beams span goes up as one copy
    const HostOut *ho = (const HostOut *)r->_owner;
    std::vector<unsigned long long> rows_off(n_seq, 0);
    std::vector<ScoreSrc> src;
    std::vector<char> pack;
    size_t rows_bytes = 0;
    bool in_chunks = ho != nullptr;
    if (in_chunks) {
        const size_t nc = ho->chunks.size();
        std::vector<const char *> lo(nc, nullptr), hi(nc, nullptr);
        std::vector<int> chunk_of(n_seq, -1);
        for (int s = 0; s < n_seq && in_chunks; s++) {
            if (!n_rows[s]) continue;
            const char *a = rows[s], *b = a + (size_t)(n_rows[s] - 1) * stride[s] + lens[s];
            for (size_t c = 0; c < nc; c++) {
                const char *cb = (const char *)ho->chunks[c]->b.p;
                if (a >= cb && b <= cb + ho->chunks[c]->b.cap) { chunk_of[s] = (int)c; break; }
            }
            if (chunk_of[s] < 0) { in_chunks = false; break; }
            const int c = chunk_of[s];
            if (!lo[c] || a < lo[c]) lo[c] = a;
            if (!hi[c] || b > hi[c]) hi[c] = b;
        }
        if (in_chunks) {
            std::vector<size_t> dev_off(nc, 0);
            for (size_t c = 0; c < nc; c++) {
                if (!lo[c]) continue;
                dev_off[c] = rows_bytes;
                src.push_back(ScoreSrc{lo[c], (size_t)(hi[c] - lo[c]), rows_bytes});
                rows_bytes += ((size_t)(hi[c] - lo[c]) + 255) & ~(size_t)255;
            }
            for (int s = 0; s < n_seq; s++)
                if (chunk_of[s] >= 0) rows_off[s] = dev_off[chunk_of[s]] + (size_t)(rows[s] - lo[chunk_of[s]]);
        }
    }
    if (!in_chunks) {       // a result that was not made by this library's fold
        score_pack(n_seq, lens.data(), n_rows.data(), rows.data(), stride.data(), pre.data(), pack, rows_off);
        src.assign(1, ScoreSrc{pack.data(), pack.size(), 0});
        rows_bytes = pack.size();
    }
    return score_impl(n_seq, lens.data(), n_rows.data(), stride.data(), rows_off.data(), pre.data(), src, rows_bytes, known, row_out, seq_out);
}

} // extern "C"
