// rafft_api.hip - the C-ABI of include/rafft_hip.h, and the one translation unit of libraffthip.so.
//
// One process drives one GPU.  The kernels and the host headers below are included here, so templates and the Dev struct are
// shared without a device-link step; this file itself holds the extern "C" entry points only: each locks g.mu, checks its
// arguments and hands over to the host header that does the work.
// A fold is the reference's bfs_pairs recursion (rafft/rafft.py:156-216) turned into an iteration over folding steps that
// advances every sequence of a wave at once:   expand (new unpaired regions) -> beam step (per sequence) -> materialize
// (new beam members) -> ... until every sequence reached its fixed point.  Every workspace has a stream set of its own
// (rafft_host_ctx.h); one scheduler thread drives the waves of all batches in flight (rafft_sched.h); the other entry points
// drain the folds in flight and run on the streams of workspace 0.
#include "../../include/rafft_hip.h"
#include "rafft_kernels.h"
#include "rafft_params.h"
#include "rafft_config.h"
#include "rafft_hostpure.h"

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
// rafft_expand_small.hip, rafft_beam.hip, rafft_materialize.hip, rafft_io_kernels.hip, rafft_findpath.hip, rafft_descend.hip, rafft_barriers.hip, rafft_kinfold.hip - is compiled into the same translation
// unit so the templates and the Dev struct are shared without a device-link step)
#include "rafft_kernels.hip"
#include "rafft_kin.hip"
#include "rafft_kin_batch.hip"
#include "rafft_landscape.hip"
#include "rafft_score.hip"
#include "rafft_mfe.hip"
#include "rafft_mfe_span.hip"
#include "rafft_cofold.hip"
#include "rafft_pf.hip"
#include "rafft_pf_span.hip"
#include "rafft_mea.hip"
#include "rafft_sample.hip"
#include "rafft_subopt.hip"

// host side, one responsibility per file (each in its own anonymous namespace)
#include "rafft_host_ctx.h"     // errors, workspaces and their buffers, the global context, memory pools, initialisation
#include "rafft_plan.h"         // size classes and LDS plans of the expand kernel, the HBM arenas of a job
#include "rafft_wave.h"         // jobs, batches, the Wave state machine, the seam call
#include "rafft_sched.h"        // the scheduler thread
#include "rafft_submit.h"       // rafft_fold_submit / rafft_fold_wait from the caller's side: validation, lanes, hand-over
#include "rafft_seam.h"         // the seam calls: their shared entry and device-buffer owner, evaluation, rafft_expand_node, the features
#include "rafft_batch.h"        // the batch drivers on top of them: kin_batch, mfe_batch, mfe_con_batch, cofold_batch, mfe_span_batch, pf_batch, pf_con_batch, pf_span_batch, mea_batch, mea_probs_batch, sample_batch, subopt_batch, findpath_batch, descend_batch, barriers_batch, kinfold_batch

// the arguments rafft_mfe_batch and rafft_pf_batch share
static int check_seq_args(int n_seq, const char *const *seqs, const int *lens, const void *seq_out, char *const *db_out)
{
    if (n_seq > 0 && (!seqs || !lens || !seq_out || !db_out)) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int s = 0; s < n_seq; s++)
        if (!db_out[s] || (lens[s] > 0 && !seqs[s])) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": null pointer");
    return 0;
}

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
 * sees whether the library had to allocate inside it (a device allocation of gigabytes now and then takes seconds). */
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

int rafft_eval_structures(int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return eval_structures(n, seqs, dbs, dcal_out, status_out);
}

int rafft_eval_structure(const char *seq, const char *db, int *dcal_out)
{
    return rafft_eval_structures(1, &seq, &db, dcal_out, nullptr);
}

int rafft_eval_structures_at(double temp, int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return eval_structures(n, seqs, dbs, dcal_out, status_out, temp);
}

int rafft_eval_structures_info(int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out, int *guessed_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return eval_structures(n, seqs, dbs, dcal_out, status_out, 37.0, guessed_out);
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

// (holds g.mu)
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
    long cnt = 0;
    const int *v = rafft_par::table_by_name(P, table, enthalpy ? 1 : 0, &cnt);
    if (!v) return fail(RAFFT_ERR_PARAM, std::string("unknown table ") + table);
    if (index < 0 || index >= cnt) return fail(RAFFT_ERR_PARAM, "index out of range");
    *value_out = v[index];
    return 0;
}

int rafft_expand_node(const rafft_params *p, const char *seq, const char *db, const int *pos, int n,
                      int *n_ranked, int *lag, double *corval, int *nb, int *mi, int *mj,
                      double *score, int *ddcal, int *n_kept, int *kept)
{
    std::lock_guard<std::mutex> lk(g.mu);
    return expand_node(p, seq, db, pos, n, n_ranked, lag, corval, nb, mi, mj, score, ddcal, n_kept, kept);
}

int rafft_kin_rate_matrix(int n_steps, const int *step_size, int L, const char *rows, const int *uid, int n_unique,
                          const double *energy, double kt, double *rate_device)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!step_size || !rows || !uid || !energy || !rate_device || n_steps < 1 || L < 1 || L > 32767 || n_unique < 1 || !(kt > 0))
        return fail(RAFFT_ERR_PARAM, "bad argument");
    return kin_rate_matrix(n_steps, step_size, L, rows, uid, n_unique, energy, kt, rate_device);
}

int rafft_kin_batch(int n_graphs, const int *lens, const int *n_steps, const int *const *step_size, const char *const *rows, const int *row_stride,
                    const double *const *energy, double kt, int n_times, const double *times, const int *m, const double *h, long long workspace_bytes,
                    rafft_kin_graph *graph_out, int *uid_out, int *first_row_out, double *pop_out, double *const *rate_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_graphs < 0 || n_times < 1 || !times || !m || !h || !(kt > 0) || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (n_graphs > 0 && (!lens || !n_steps || !step_size || !rows || !row_stride || !energy || !graph_out || !uid_out || !first_row_out || !pop_out))
        return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < n_times; k++) {
        if (!(times[k] > (k ? times[k - 1] : 0.0)) || !(times[k] < INFINITY)) return fail(RAFFT_ERR_PARAM, "times must be positive and ascend");
        if (m[k] < 1 || !(h[k] > 0) || !(h[k] < INFINITY)) return fail(RAFFT_ERR_PARAM, "interval " + std::to_string(k) + ": non-positive sub-step count or step");
    }
    for (int i = 0; i < n_graphs; i++) {
        const std::string who = "graph " + std::to_string(i);
        if (lens[i] < 0 || lens[i] > 32767) return fail(RAFFT_ERR_PARAM, who + ": length outside 0..32767");
        if (row_stride[i] < lens[i]) return fail(RAFFT_ERR_PARAM, who + ": row stride below the length");
        if (n_steps[i] < 0 || (n_steps[i] && !step_size[i])) return fail(RAFFT_ERR_PARAM, who + ": negative number of steps or no step sizes");
        long long nr = 0;
        for (int s = 0; s < n_steps[i]; s++) {
            if (step_size[i][s] < 0) return fail(RAFFT_ERR_PARAM, who + ": negative step size");
            nr += step_size[i][s];
        }
        if (nr && (!rows[i] || !energy[i])) return fail(RAFFT_ERR_PARAM, who + ": null pointer");
    }
    return kin_batch(n_graphs, lens, n_steps, step_size, rows, row_stride, energy, kt, n_times, m, h, workspace_bytes, graph_out, uid_out, first_row_out,
                     pop_out, rate_out);
}

int rafft_landscape_distances(int n, int L, const char *rows, uint16_t *dist_device)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!rows || !dist_device || n < 1 || L < 1 || L > 32767) return fail(RAFFT_ERR_PARAM, "bad argument");
    return landscape_distances(n, L, rows, dist_device);
}

int rafft_landscape_mds(int n, const uint16_t *dist_device, int n_init, const double *x_init, int max_iter, double eps,
                        double *x_device, double *stress_out, int *n_iter_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!dist_device || !x_init || !x_device || !stress_out || !n_iter_out || n < 1 || n_init < 1 || n_init > 65535 || max_iter < 1 || !(eps == eps))
        return fail(RAFFT_ERR_PARAM, "bad argument");
    return landscape_mds(n, dist_device, n_init, x_init, max_iter, eps, x_device, stress_out, n_iter_out);
}

int rafft_landscape_surface(int n, const double *x_device, const double *w_device, int grid, double lo, double hi, double *z_device,
                            double *phi_device)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!x_device || n < 1 || (!z_device && !phi_device) || (z_device && (!w_device || grid < 1 || grid > 32768 || !(lo <= hi))))
        return fail(RAFFT_ERR_PARAM, "bad argument");
    return landscape_surface(n, x_device, w_device, grid, lo, hi, z_device, phi_device);
}

int rafft_landscape_counters(long long out[4])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < 4; k++) out[k] = g_landscape_counters[k];
    return 0;
}

int rafft_score_rows(int n_seq, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                     const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || (n_seq > 0 && (!lens || !n_rows || !rows || !row_stride || !known || !seq_out))) return fail(RAFFT_ERR_PARAM, "bad argument");
    return score_rows(n_seq, lens, n_rows, rows, row_stride, known, row_out, seq_out);
}

int rafft_score_result(const rafft_result *r, const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!r || r->n_seq < 0 || (r->n_seq > 0 && (!r->seq || !known || !seq_out))) return fail(RAFFT_ERR_PARAM, "bad argument");
    return score_result(r, known, row_out, seq_out);
}

int rafft_mfe_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int max_lds_len, long long workspace_bytes,
                    rafft_mfe_seq *seq_out, char *const *db_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || max_lds_len < 0 || max_lds_len > RAFFT_MFE_LDS_LEN || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return mfe_batch(n_seq, seqs, lens, temp, max_lds_len ? max_lds_len : RAFFT_MFE_LDS_LEN, workspace_bytes, seq_out, db_out);
}

int rafft_mfe_lds_len(void) { return RAFFT_MFE_LDS_LEN; }

int rafft_mfe_constrained_batch(int n_seq, const char *const *seqs, const int *lens, double temp, const char *const *constraints,
                                const int32_t *const *soft_unpaired, const int32_t *const *soft_stack, int max_lds_len, long long workspace_bytes,
                                rafft_mfe_con_seq *seq_out, char *const *db_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || max_lds_len < 0 || max_lds_len > RAFFT_MFE_LDS_LEN || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return mfe_con_batch(n_seq, seqs, lens, temp, constraints, soft_unpaired, soft_stack, max_lds_len ? max_lds_len : RAFFT_MFE_LDS_LEN, workspace_bytes,
                         seq_out, db_out);
}

int rafft_cofold_batch(int n_seq, const char *const *seqs, const int *lens, const int *cuts, double temp, int max_lds_len, long long workspace_bytes,
                       rafft_cofold_seq *seq_out, char *const *db_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || max_lds_len < 0 || max_lds_len > RAFFT_MFE_LDS_LEN || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return cofold_batch(n_seq, seqs, lens, cuts, temp, max_lds_len ? max_lds_len : RAFFT_MFE_LDS_LEN, workspace_bytes, seq_out, db_out);
}

int rafft_cofold_duplex_init(double temp, int *dcal_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!dcal_out) return fail(RAFFT_ERR_PARAM, "null argument");
    if (int rc = check_temp(temp)) return rc;
    *dcal_out = cofold_duplex_init(temp);
    return 0;
}

int rafft_mfe_span_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int max_span, long long workspace_bytes,
                         rafft_mfe_seq *seq_out, char *const *db_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (max_span < 1 || max_span > RAFFT_MFE_MAX_LEN) return fail(RAFFT_ERR_PARAM, "max_span outside 1 .. RAFFT_MFE_MAX_LEN");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return mfe_span_batch(n_seq, seqs, lens, temp, max_span, workspace_bytes, seq_out, db_out);
}

int rafft_pf_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, long long workspace_bytes,
                   rafft_pf_seq *seq_out, char *const *db_out, double *const *prob_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || workspace_bytes < 0 || !std::isfinite(scale_factor) || scale_factor < 0.0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return pf_batch(n_seq, seqs, lens, temp, scale_factor, workspace_bytes, seq_out, db_out, prob_out);
}

int rafft_pf_constrained_batch(int n_seq, const char *const *seqs, const int *lens, double temp, const char *const *constraints,
                               const int32_t *const *soft_unpaired, const int32_t *const *soft_stack, double scale_factor, long long workspace_bytes,
                               rafft_pf_seq *seq_out, char *const *db_out, double *const *prob_out, double *const *unpaired_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || workspace_bytes < 0 || !std::isfinite(scale_factor) || scale_factor < 0.0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return pf_con_batch(n_seq, seqs, lens, temp, constraints, soft_unpaired, soft_stack, scale_factor, workspace_bytes, seq_out, db_out, prob_out, unpaired_out);
}

int rafft_pf_span_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, int max_span, long long workspace_bytes,
                        rafft_pf_seq *seq_out, char *const *db_out, double *const *prob_out, double *const *unpaired_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || workspace_bytes < 0 || !std::isfinite(scale_factor) || scale_factor < 0.0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (max_span < 1 || max_span > RAFFT_MFE_MAX_LEN) return fail(RAFFT_ERR_PARAM, "max_span outside 1 .. RAFFT_MFE_MAX_LEN");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return pf_span_batch(n_seq, seqs, lens, temp, scale_factor, max_span, workspace_bytes, seq_out, db_out, prob_out, unpaired_out);
}

int rafft_mea_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, long long workspace_bytes, double gamma,
                    rafft_mea_seq *seq_out, char *const *db_out, double *const *prob_out, double *const *unpaired_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || workspace_bytes < 0 || !std::isfinite(scale_factor) || scale_factor < 0.0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (!std::isfinite(gamma) || gamma < 0.0) return fail(RAFFT_ERR_PARAM, "gamma is negative or not finite");
    if (int rc = check_seq_args(n_seq, seqs, lens, seq_out, db_out)) return rc;
    return mea_batch(n_seq, seqs, lens, temp, scale_factor, workspace_bytes, gamma > 0.0 ? gamma : 1.0, seq_out, db_out, prob_out, unpaired_out);
}

int rafft_mea_probs_batch(int n, const int *lens, const double *const *prob_in, double gamma, long long workspace_bytes, rafft_mea_probs_seq *seq_out,
                          char *const *db_out, double *const *unpaired_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n < 0 || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (!std::isfinite(gamma) || gamma < 0.0) return fail(RAFFT_ERR_PARAM, "gamma is negative or not finite");
    if (n > 0 && (!lens || !prob_in || !seq_out || !db_out)) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int s = 0; s < n; s++)
        if (!db_out[s] || (lens[s] > 0 && lens[s] <= RAFFT_PF_MAX_LEN && !prob_in[s])) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": null pointer");
    return mea_probs_batch(n, lens, prob_in, gamma > 0.0 ? gamma : 1.0, workspace_bytes, seq_out, db_out, unpaired_out);
}

int rafft_sample_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, long long workspace_bytes,
                       int n_samples, const unsigned long long *seeds, rafft_sample_seq *seq_out, char *const *db_out, int *const *dcal_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || n_samples < 0 || n_samples > RAFFT_SAMPLE_MAX || workspace_bytes < 0 || !std::isfinite(scale_factor) || scale_factor < 0.0)
        return fail(RAFFT_ERR_PARAM, "bad argument");
    if (!seq_out || (n_samples > 0 && !db_out)) return fail(RAFFT_ERR_PARAM, "null argument");
    if (n_seq > 0 && (!seqs || !lens)) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int s = 0; s < n_seq; s++)
        if ((n_samples > 0 && !db_out[s]) || (lens[s] > 0 && !seqs[s])) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": null pointer");
    return sample_batch(n_seq, seqs, lens, temp, scale_factor, workspace_bytes, n_samples, seeds, seq_out, db_out, dcal_out);
}

int rafft_subopt_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int delta_dcal, int max_structs, long long workspace_bytes,
                       rafft_subopt_result **out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    *out = nullptr;
    if (n_seq < 0 || workspace_bytes < 0 || delta_dcal < 0 || delta_dcal > RAFFT_SUBOPT_MAX_DELTA || max_structs < 1 || max_structs > RAFFT_SUBOPT_MAX_STRUCTS)
        return fail(RAFFT_ERR_PARAM, "bad argument");
    if (n_seq > 0 && (!seqs || !lens)) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int s = 0; s < n_seq; s++)
        if (lens[s] > 0 && !seqs[s]) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": null pointer");
    return subopt_batch(n_seq, seqs, lens, temp, delta_dcal, max_structs, workspace_bytes, out);
}

void rafft_subopt_free(rafft_subopt_result *r)
{
    if (r && r->_owner) delete (SuboptOwner *)r->_owner;
}

int rafft_findpath_batch(int n_paths, const char *const *seqs, const int *lens, const char *const *starts, const char *const *ends, const int *widths,
                         double temp, long long workspace_bytes, rafft_findpath_rec *rec_out, int *const *moves_out, int *const *dcal_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_paths < 0 || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (n_paths > 0 && (!seqs || !lens || !starts || !ends || !widths || !rec_out)) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int p = 0; p < n_paths; p++) {
        if (!starts[p] || !ends[p] || (lens[p] > 0 && !seqs[p])) return fail(RAFFT_ERR_PARAM, "problem " + std::to_string(p) + ": null pointer");
        if (widths[p] < 1 || widths[p] > RAFFT_FINDPATH_MAX_WIDTH)
            return fail(RAFFT_ERR_PARAM, "problem " + std::to_string(p) + ": width outside 1.." + std::to_string(RAFFT_FINDPATH_MAX_WIDTH));
    }
    return findpath_batch(n_paths, seqs, lens, starts, ends, widths, temp, workspace_bytes, rec_out, moves_out, dcal_out);
}

int rafft_findpath_counters(long long out[4])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < 4; k++) out[k] = g_findpath_counters[k];
    return 0;
}

// What the three row calls ask of sequence s before anything runs, as text behind "sequence s", nullptr when nothing is wrong:
// check_seq_args - its row count and its bases; check_row_block - one block of n rows `stride` bytes apart (`own`: the call's other
// per-sequence pointers that go with the block are there).
static const char *check_seq_args(const char *const *seqs, const int *lens, const int *n_rows, int s)
{
    if (n_rows[s] < 0) return ": negative row count";
    if (lens[s] > 0 && !seqs[s]) return ": null pointer";
    return nullptr;
}
static const char *check_row_block(int len, int n, const char *block, int stride, bool own)
{
    if (n <= 0) return nullptr;
    if (!block || !own) return ": null pointer";
    if (stride < (len > 0 ? len : 0)) return ": stride below the length";
    return nullptr;
}
static const char *check_row_args(const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride, int s, bool own)
{
    const char *what = check_seq_args(seqs, lens, n_rows, s);
    return what ? what : check_row_block(lens[s], n_rows[s], rows[s], row_stride[s], own);
}

int rafft_descend_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                        double temp, int max_steps, long long workspace_bytes, rafft_descend_seq *seq_out, rafft_descend_row *row_out,
                        char *const *db_out, int *const *moves_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0 || max_steps < 0 || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (n_seq > 0 && (!seqs || !lens || !n_rows || !rows || !row_stride || !seq_out || !db_out)) return fail(RAFFT_ERR_PARAM, "null argument");
    long long total = 0;
    for (int s = 0; s < n_seq; s++) {
        if (const char *what = check_row_args(seqs, lens, n_rows, rows, row_stride, s, db_out[s] != nullptr)) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + what);
        total += n_rows[s];
    }
    if (total > 0x7fffffffll) return fail(RAFFT_ERR_PARAM, "more than 2^31 - 1 rows");
    if (total > 0 && !row_out) return fail(RAFFT_ERR_PARAM, "null argument");
    return descend_batch(n_seq, seqs, lens, n_rows, rows, row_stride, temp, max_steps, workspace_bytes, seq_out, row_out, db_out, moves_out);
}

int rafft_descend_counters(long long out[4])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < 4; k++) out[k] = g_descend_counters[k];
    return 0;
}

int rafft_barriers_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                         const int *const *dcal, int max_edges, long long workspace_bytes, rafft_barriers_result **out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    *out = nullptr;
    if (n_seq < 0 || max_edges < 0 || workspace_bytes < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (n_seq > 0 && (!seqs || !lens || !n_rows || !rows || !row_stride || !dcal)) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int s = 0; s < n_seq; s++)
        if (const char *what = check_row_args(seqs, lens, n_rows, rows, row_stride, s, dcal[s] != nullptr)) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + what);
    return barriers_batch(n_seq, seqs, lens, n_rows, rows, row_stride, dcal, max_edges, workspace_bytes, out);
}

void rafft_barriers_free(rafft_barriers_result *r)
{
    if (r && r->_owner) delete (BarriersOwner *)r->_owner;
}

int rafft_barriers_counters(long long out[6])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < 6; k++) out[k] = g_barriers_counters[k];
    return 0;
}

int rafft_kinfold_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                        int n_rep, const int *n_watch, const int *n_stop, const char *const *watch, const int *watch_stride,
                        const unsigned long long *seeds, double temp, double kt, double t_max, int max_steps, int n_times, const double *sample_times,
                        long long workspace_bytes, rafft_kinfold_seq *seq_out, rafft_kinfold_traj *traj_out, char *const *db_out,
                        int32_t *const *samples_out, int *const *moves_out, double *const *times_out)
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (n_seq < 0) return fail(RAFFT_ERR_PARAM, "bad argument");
    if (const char *what = kinfold_check_call(n_rep, kt, t_max, max_steps, n_times, sample_times, workspace_bytes)) return fail(RAFFT_ERR_PARAM, what);
    if (n_seq > 0 && (!seqs || !lens || !n_rows || !rows || !row_stride || !seq_out || !db_out)) return fail(RAFFT_ERR_PARAM, "null argument");
    if (n_seq > 0 && n_watch && (!n_stop || !watch || !watch_stride)) return fail(RAFFT_ERR_PARAM, "null argument");
    if (n_seq > 0 && n_times > 0 && !samples_out) return fail(RAFFT_ERR_PARAM, "null argument");
    if (n_seq > 0 && (moves_out == nullptr) != (times_out == nullptr)) return fail(RAFFT_ERR_PARAM, "moves_out and times_out go together");
    long long total = 0;
    for (int s = 0; s < n_seq; s++) {
        // (the watched rows are asked about between the sequence and its start rows: the order of the texts is kept)
        const std::string who = "sequence " + std::to_string(s);
        if (const char *what = check_seq_args(seqs, lens, n_rows, s)) return fail(RAFFT_ERR_PARAM, who + what);
        if (n_watch) {
            if (const char *what = kinfold_check_watch(n_watch[s], n_stop[s])) return fail(RAFFT_ERR_PARAM, who + ": " + what);
            if (const char *what = check_row_block(lens[s], n_watch[s], watch[s], watch_stride[s], true)) return fail(RAFFT_ERR_PARAM, who + what);
        }
        if (const char *what = check_row_block(lens[s], n_rows[s], rows[s], row_stride[s], db_out[s] && !(n_times > 0 && !samples_out[s]))) return fail(RAFFT_ERR_PARAM, who + what);
        if (n_rows[s] > 0 && moves_out && (moves_out[s] == nullptr) != (times_out[s] == nullptr)) return fail(RAFFT_ERR_PARAM, who + ": moves_out and times_out go together");
        total += (long long)n_rows[s] * n_rep;
        if (total > 0x7fffffffll) return fail(RAFFT_ERR_PARAM, "more than 2^31 - 1 trajectories");
    }
    if (total > 0 && !traj_out) return fail(RAFFT_ERR_PARAM, "null argument");
    return kinfold_batch(n_seq, seqs, lens, n_rows, rows, row_stride, n_rep, n_watch, n_stop, watch, watch_stride, seeds, temp, kt, t_max, max_steps,
                         n_times, sample_times, workspace_bytes, seq_out, traj_out, db_out, samples_out, moves_out, times_out);
}

int rafft_kinfold_weights(double temp, double kt, uint64_t *out)
{
    if (!out || !(temp > -273.15 && temp < 1000.0) || !kinfold_weights(temp, kt, out)) return RAFFT_ERR_PARAM;
    return 0;
}

int rafft_kinfold_counters(long long out[4])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < 4; k++) out[k] = g_kinfold_counters[k];
    return 0;
}

int rafft_subopt_counters(long long out[7])
{
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return fail(RAFFT_ERR_PARAM, "null argument");
    for (int k = 0; k < 7; k++) out[k] = g_subopt_counters[k];
    return 0;
}

} // extern "C"
