// rafft_seam.h - the seam calls: entry points that drain the folds in flight and borrow workspace 0 on the caller's thread.
// What they share is written once here - how such a call enters (SeamGuard) and who owns its device buffers (DevScratch) -
// followed by the calls themselves: structure evaluation, rafft_expand_node, and the drivers of the single-item feature kernels
// (the kinetics rate matrix, the folding landscape, accuracy scoring).  The batch drivers are in rafft_batch.h.
// Part of the single translation unit of rafft_api.hip (included there, after rafft_submit.h).
#pragma once

namespace {

// Entry of a seam call.  The entry point holds g.mu and has validated its arguments (a bad argument fails without touching the
// device); then: no fold in flight (nothing new is submitted under g.mu; hipMalloc / hipFree synchronise the device, and results
// are written on the library's stream - the caller hands over buffers its own stream is done with), workspace 0 held against
// the idle trimming until the guard goes out of scope, its streams made.  Copies and kernels of the call go to `stream`.
struct SeamGuard {
    std::unique_lock<std::mutex> ws_lk;
    hipStream_t stream = nullptr;
    int enter()
    {
        if (int rc = init_ctx(-1)) return rc;
        drain();
        ws_lk = std::unique_lock<std::mutex>(g.ws_mu);
        if (int rc = init_ws(g.ws[0])) return rc;
        stream = g.ws[0].stream;
        return 0;
    }
};

// The device buffers of one call: allocated per call (if (int rc = mem.alloc(p, bytes)) return rc;), freed when the scope ends -
// on every way out, each a plain return, and after the call's last synchronise.  Nothing is pooled or cached.
struct DevScratch {
    std::vector<void *> held;
    template <class T> int alloc(T *&p, size_t bytes)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return fail(RAFFT_ERR_HIP, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
        held.push_back(q);
        p = (T *)q;
        return 0;
    }
    ~DevScratch() { for (void *q : held) { hipError_t fe = hipFree(q); (void)fe; } }
};

// energies of n structures at `temp`, under the caller's guard (scales the device tables for `temp`)
int eval_structures_held(hipStream_t st, int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out, double temp, int *guessed_out)
{
    if (int rc = ensure_tables(temp)) return rc;
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
        if (!parse_db(dbs[i], len[i], pt)) { status[i] = RAFFT_ERR_STRUCT; len[i] = 0; continue; }
        for (int x = 0; x < len[i]; x++) {
            const unsigned k = kBaseCode[(unsigned char)seqs[i][x]];
            if (k & 8) { status[i] = RAFFT_ERR_BAD_CHAR; break; }
            codes[off[i] + x] = (uint8_t)k;
            pts[off[i] + x] = pt[x];
        }
        if (status[i]) len[i] = 0;
    }
    DevScratch mem;
    uint8_t *dc; int16_t *dp; long long *doff; int *dlen, *dout, *dst, *dg;
    if (int rc = mem.alloc(dc, tot + 16)) return rc;
    if (int rc = mem.alloc(dp, (tot + 16) * 2)) return rc;
    if (int rc = mem.alloc(doff, n * 8 + 8)) return rc;
    if (int rc = mem.alloc(dlen, n * 4 + 4)) return rc;
    if (int rc = mem.alloc(dout, n * 4 + 4)) return rc;
    if (int rc = mem.alloc(dst, n * 4 + 4)) return rc;
    if (int rc = mem.alloc(dg, n * 4 + 4)) return rc;
    HIPCHK(hipMemcpyAsync(dc, codes.data(), tot + 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dp, pts.data(), (tot + 16) * 2, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(doff, off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dlen, len.data(), n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(eval_kernel, dim3(n), dim3(64), 0, st, g.T, n, dc, dp, doff, dlen, dout, dst, dg);
    HIPCHK(hipGetLastError());
    std::vector<int> st2(n);
    HIPCHK(hipMemcpyAsync(dcal_out, dout, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(st2.data(), dst, n * 4, hipMemcpyDeviceToHost, st));
    if (guessed_out) HIPCHK(hipMemcpyAsync(guessed_out, dg, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
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

// (holds g.mu)
int eval_structures(int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out, double temp = 37.0, int *guessed_out = nullptr)
{
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    return eval_structures_held(sg.stream, n, seqs, dbs, dcal_out, status_out, temp, guessed_out);
}

// rafft_expand_node (holds g.mu): region `pos` of structure `db` through the expand kernel, its ranked lags and kept stems read back
int expand_node(const rafft_params *p, const char *seq, const char *db, const int *pos, int n, int *n_ranked, int *lag, double *corval,
                int *nb, int *mi, int *mj, double *score, int *ddcal, int *n_kept, int *kept)
{
    const int L = (int)strlen(seq);
    if (L == 0 || L > RAFFT_MAX_LEN || n < 1 || n > L) return fail(RAFFT_ERR_PARAM, "bad node");
    std::vector<int16_t> pt;
    if (!parse_db(db, L, pt)) return fail(RAFFT_ERR_STRUCT, "malformed dot-bracket");
    LoopOf lp = enclosing_loop(pt, pos[0]);
    // (a candidate's four cut points are 12-bit branch counts and the class for the biggest regions stages BIG_BR + 1 branch words in
    //  LDS: a loop with more helices is refused here, before the device is touched - Cand::set_cuts, class_cfg's BR[0])
    if ((int)lp.br.size() > BIG_BR)
        return fail(RAFFT_ERR_PARAM, "loop with " + std::to_string(lp.br.size()) + " branch helices: at most " + std::to_string(BIG_BR) + " in one loop (12-bit branch cut points)");
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    SeamIn sm;
    sm.ci = lp.ci; sm.cj = lp.cj; sm.br = std::move(lp.br);
    sm.pos.assign(pos, pos + n);
    if (int rc = eval_structures_held(sg.stream, 1, &seq, &db, &sm.pdcal, nullptr, p->temp, nullptr)) return rc;   // (also scales the tables for p->temp)
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
    ho.resize(1);
    Batch bt;                                  // a private batch: the scheduler is idle (drained by the guard) and g.mu is held
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

int kin_rate_matrix(int n_steps, const int *step_size, int L, const char *rows, const int *uid, int n_unique, const double *energy, double kt,
                    double *rate_device)
{
    long long n = 0;
    std::vector<int> row0(n_steps);
    for (int i = 0; i < n_steps; i++) { row0[i] = (int)n; n += step_size[i]; if (step_size[i] < 0) return fail(RAFFT_ERR_PARAM, "negative step size"); }
    if (n < 1 || n > 0x7fffffff) return fail(RAFFT_ERR_PARAM, "bad number of structures");
    for (long long r = 0; r < n; r++) if (uid[r] < 0 || uid[r] >= n_unique) return fail(RAFFT_ERR_PARAM, "uid out of range");
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    hipStream_t st = sg.stream;
    DevScratch mem;
    char *d_rows; int16_t *d_pt, *d_stack; int *d_uid, *d_bad; double *d_en;
    if (int rc = mem.alloc(d_rows, (size_t)n * L)) return rc;
    if (int rc = mem.alloc(d_pt, (size_t)n * L * 2)) return rc;
    if (int rc = mem.alloc(d_stack, (size_t)n * L * 2)) return rc;
    if (int rc = mem.alloc(d_uid, (size_t)n * 4)) return rc;
    if (int rc = mem.alloc(d_en, (size_t)n_unique * 8)) return rc;
    if (int rc = mem.alloc(d_bad, 4)) return rc;
    HIPCHK(hipMemcpyAsync(d_rows, rows, (size_t)n * L, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_uid, uid, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_en, energy, (size_t)n_unique * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_bad, 0, 4, st));
    HIPCHK(hipMemsetAsync(rate_device, 0, (size_t)n_unique * n_unique * 8, st));
    hipLaunchKernelGGL(kin_pair_table_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (int)n, L, d_rows, d_pt, d_stack, d_bad);
    HIPCHK(hipGetLastError());
    for (int i = 0; i < n_steps; i++) {
        const int pi = kin_prev_step(i, n_steps);
        if (!step_size[i] || !step_size[pi]) continue;
        hipLaunchKernelGGL(kin_rates_kernel, dim3((unsigned)step_size[i]), dim3(KIN_NT), (size_t)L * 2, st, L, d_pt, row0[i], step_size[pi], row0[pi],
                           d_uid, d_en, kt, n_unique, rate_device);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(kin_diag_kernel, dim3((unsigned)n_unique), dim3(256), 0, st, n_unique, rate_device);
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return fail(RAFFT_ERR_STRUCT, "malformed dot-bracket row");
    return 0;
}

// ---- folding landscape

long long g_landscape_counters[4];      // MDS calls, SMACOF passes enqueued, host read-backs of the `done` words, passes of the last call
constexpr int LANDSCAPE_CHUNK = 64;     // SMACOF passes enqueued between two read-backs

int landscape_distances(int n, int L, const char *rows, uint16_t *dist_device)
{
    const unsigned T = (unsigned)((n + LS_TILE - 1) / LS_TILE);
    if (T > 65535) return fail(RAFFT_ERR_PARAM, "too many structures");
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    hipStream_t st = sg.stream;
    const int Lp = (L + LS_CHUNK - 1) / LS_CHUNK * LS_CHUNK;
    DevScratch mem;
    char *d_rows; int16_t *d_pt, *d_stack; uint16_t *d_open; int *d_np, *d_bad;
    if (int rc = mem.alloc(d_rows, (size_t)n * L)) return rc;
    if (int rc = mem.alloc(d_pt, (size_t)n * L * 2)) return rc;
    if (int rc = mem.alloc(d_stack, (size_t)n * L * 2)) return rc;
    if (int rc = mem.alloc(d_open, (size_t)n * Lp * 2)) return rc;
    if (int rc = mem.alloc(d_np, (size_t)n * 4)) return rc;
    if (int rc = mem.alloc(d_bad, 4)) return rc;
    HIPCHK(hipMemcpyAsync(d_rows, rows, (size_t)n * L, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_bad, 0, 4, st));
    hipLaunchKernelGGL(kin_pair_table_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, L, d_rows, d_pt, d_stack, d_bad);
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return fail(RAFFT_ERR_STRUCT, "malformed dot-bracket row");
    hipLaunchKernelGGL(landscape_open_table_kernel, dim3((unsigned)n), dim3(64), 0, st, n, L, Lp, d_pt, d_open, d_np);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(landscape_distance_kernel, dim3(T, T), dim3(256), 0, st, n, Lp, d_open, d_np, dist_device);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int landscape_mds(int n, const uint16_t *dist_device, int n_init, const double *x_init, int max_iter, double eps, double *x_device,
                  double *stress_out, int *n_iter_out)
{
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    hipStream_t st = sg.stream;
    DevScratch mem;
    double *d_x, *d_rs; LandscapeMdsState *d_state;
    const size_t per = (size_t)n * 2 * sizeof(double);            // one configuration
    if (int rc = mem.alloc(d_x, per * 2 * n_init)) return rc;
    if (int rc = mem.alloc(d_rs, per * n_init)) return rc;
    if (int rc = mem.alloc(d_state, sizeof(LandscapeMdsState) * n_init)) return rc;
    HIPCHK(hipMemsetAsync(d_state, 0, sizeof(LandscapeMdsState) * n_init, st));
    for (int k = 0; k < n_init; k++)                               // X_0 of start k -> its buffer 0
        HIPCHK(hipMemcpyAsync((char *)d_x + per * 2 * k, x_init + (size_t)k * n * 2, per, hipMemcpyHostToDevice, st));
    // X in LDS up to 128 KiB (8192 points, one workgroup per CU); beyond that it is read through the caches
    const size_t lds = (size_t)n * 16;
    const bool xlds = lds <= ((size_t)128 << 10);
    static bool lds_attr_set = false;
    if (xlds && !lds_attr_set) {
        HIPCHK(hipFuncSetAttribute((const void *)landscape_smacof_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 << 10));
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
                hipLaunchKernelGGL(landscape_smacof_kernel<true>, dim3((unsigned)gx, (unsigned)n_init), dim3(LS_SM_NT), lds, st, n, dist_device, d_x, d_rs, d_state, pass, guttman);
            else
                hipLaunchKernelGGL(landscape_smacof_kernel<false>, dim3((unsigned)gx, (unsigned)n_init), dim3(LS_SM_NT), 0, st, n, dist_device, d_x, d_rs, d_state, pass, guttman);
            hipLaunchKernelGGL(landscape_smacof_finalize_kernel, dim3((unsigned)n_init), dim3(256), 0, st, n, d_x, d_rs, d_state, pass, max_iter, eps, x_device);
            g_landscape_counters[1]++; g_landscape_counters[3]++;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs.data(), d_state, sizeof(LandscapeMdsState) * n_init, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        g_landscape_counters[2]++;
        all_done = true;
        for (int k = 0; k < n_init; k++) all_done = all_done && hs[k].done;
    }
    if (!all_done) return fail(RAFFT_ERR_HIP, "internal: SMACOF did not finish within max_iter + 1 passes");
    for (int k = 0; k < n_init; k++) { stress_out[k] = hs[k].stress; n_iter_out[k] = hs[k].n_iter; }
    return 0;
}

int landscape_surface(int n, const double *x_device, const double *w_device, int grid, double lo, double hi, double *z_device, double *phi_device)
{
    if (phi_device && n > 65535) return fail(RAFFT_ERR_PARAM, "too many structures");
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    hipStream_t st = sg.stream;
    if (phi_device) {
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

// ---- accuracy scoring

// device buffers of the scoring calls: grow-only and kept for the life of the process (a call on a warm library allocates nothing).
// Unlike the workspaces they are not trimmed when the library idles: after the biggest call so far they hold its rows, its row
// records and, for sequences beyond the LDS plans, up to 1024 workgroups' scratch (tens of MB at the benchmark's sizes).
struct { Buf rows, known, seqs, items, row_out, seq_out, scratch; } g_score;

// under the caller's guard.  rows_off[s]: where sequence s's first row lies in the device copy of `src`; pre_status[s] != 0: the
// sequence is not scored
int score_held(hipStream_t st, int n_seq, const int *lens, const int *n_rows, const int *stride, const unsigned long long *rows_off, const int *pre_status,
               const std::vector<ScoreSrc> &src, size_t rows_bytes, const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out)
{
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

// rafft_score_rows: rows anywhere in host memory, packed first
int score_rows(int n_seq, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride, const char *const *known,
               rafft_score_row *row_out, rafft_score_seq *seq_out)
{
    for (int s = 0; s < n_seq; s++) {
        if (lens[s] < 0 || lens[s] > 32767) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": length outside 0..32767");
        if (n_rows[s] < 0) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": negative number of rows");
        if (row_stride[s] < lens[s]) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": row stride below the length");
        if (!known[s] || (n_rows[s] && !rows[s])) return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": null pointer");
    }
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    std::vector<char> pack;
    std::vector<unsigned long long> rows_off(n_seq);
    score_pack(n_seq, lens, n_rows, rows, row_stride, nullptr, pack, rows_off);
    std::vector<ScoreSrc> src{ScoreSrc{pack.data(), pack.size(), 0}};
    return score_held(sg.stream, n_seq, lens, n_rows, row_stride, rows_off.data(), nullptr, src, pack.size(), known, row_out, seq_out);
}

// rafft_score_result: the final beams of a fold's result
int score_result(const rafft_result *r, const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out)
{
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
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    // the rows lie in the pinned chunks the fold's copies landed in: per chunk, the range the final beams span goes up as one copy
    const HostOut *ho = (const HostOut *)r->_owner;
    std::vector<unsigned long long> rows_off(n_seq, 0);
    std::vector<ScoreSrc> src;
    std::vector<char> pack;
    size_t rows_bytes = 0;
    std::vector<const char *> cbase;
    std::vector<size_t> ccap;
    if (ho) for (auto &c : ho->chunks) { cbase.push_back((const char *)c->b.p); ccap.push_back(c->b.cap); }
    if (!ho || !score_chunk_layout(n_seq, lens.data(), n_rows.data(), stride.data(), rows.data(), cbase.size(), cbase.data(), ccap.data(), src, rows_off, rows_bytes)) {
        // a result that was not made by this library's fold
        score_pack(n_seq, lens.data(), n_rows.data(), rows.data(), stride.data(), pre.data(), pack, rows_off);
        src.assign(1, ScoreSrc{pack.data(), pack.size(), 0});
        rows_bytes = pack.size();
    }
    return score_held(sg.stream, n_seq, lens.data(), n_rows.data(), stride.data(), rows_off.data(), pre.data(), src, rows_bytes, known, row_out, seq_out);
}

} // namespace
