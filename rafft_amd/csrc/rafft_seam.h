// rafft_seam.h - the seam calls: entry points that drain the folds in flight and borrow workspace 0 on the caller's thread.
// What they share is written once here - how such a call enters (SeamGuard) and who owns its device buffers (DevScratch) -
// followed by the calls themselves: structure evaluation, rafft_expand_node, and the drivers of the feature kernels (the kinetics
// rate matrix, the folding landscape, accuracy scoring, minimum-free-energy folds).
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
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    LoopOf lp = enclosing_loop(pt, pos[0]);
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
        const int pi = i == 0 ? n_steps - 1 : i - 1;      // the reference compares step 0 with the LAST step (fast_paths[-1], rafft_kin.py:75)
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

// rafft_kin_batch (arguments validated by the entry point).  Two passes over the device: structure identity for every graph, then -
// the numbers of unique structures being known - rates and integration for chunks of graphs whose matrices fit the workspace budget.
constexpr size_t KIN_BATCH_WORKSPACE = (size_t)512 << 20;

int kin_batch(int n_graphs, const int *lens, const int *n_steps, const int *const *step_size, const char *const *rows, const int *row_stride,
              const double *const *energy, double kt, int n_times, const int *m, const double *h, long long workspace_bytes,
              rafft_kin_graph *rec, int *uid_out, int *first_row_out, double *pop_out, double *const *rate_out)
{
    std::vector<KinGraph> gs(n_graphs);
    long long n = 0;
    unsigned long long bytes = 0;
    int Lmax = 0;
    for (int g = 0; g < n_graphs; g++) {
        long long nr = 0;
        for (int i = 0; i < n_steps[g]; i++) nr += step_size[g][i];
        if (n + nr > 0x7fffffff) return fail(RAFFT_ERR_PARAM, "too many rows");
        gs[g] = KinGraph{bytes, 0, lens[g], (int)nr, (int)n, 0};
        rec[g] = rafft_kin_graph{0, (int)nr, (int)n, 0, 0, 0};
        n += nr;
        bytes += (unsigned long long)nr * (unsigned long long)lens[g];
        if (nr) Lmax = std::max(Lmax, lens[g]);
    }
    if (n == 0) return 0;
    // rows packed back to back; per row: its graph, the step it is compared with, its energy
    std::vector<char> pack(bytes + 1);
    std::vector<int> row_graph(n), row_prev0(n), row_nprev(n);
    std::vector<double> en(n);
    for (int g = 0; g < n_graphs; g++) {
        const KinGraph &G = gs[g];
        if (!G.n_rows) continue;
        if (row_stride[g] == G.L) memcpy(pack.data() + G.off, rows[g], (size_t)G.n_rows * G.L);
        else for (int r = 0; r < G.n_rows; r++) memcpy(pack.data() + G.off + (size_t)r * G.L, rows[g] + (size_t)r * row_stride[g], (size_t)G.L);
        memcpy(en.data() + G.row0, energy[g], (size_t)G.n_rows * sizeof(double));
        std::vector<int> s0(n_steps[g]);
        int at = G.row0;
        for (int i = 0; i < n_steps[g]; i++) { s0[i] = at; at += step_size[g][i]; }
        for (int i = 0; i < n_steps[g]; i++) {
            const int pi = i == 0 ? n_steps[g] - 1 : i - 1;   // the reference compares step 0 with the LAST step (fast_paths[-1], rafft_kin.py:75)
            for (int r = s0[i]; r < s0[i] + step_size[g][i]; r++) { row_graph[r] = g; row_prev0[r] = s0[pi]; row_nprev[r] = step_size[g][pi]; }
        }
    }
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    hipStream_t st = sg.stream;
    DevScratch mem;
    KinGraph *d_gs; char *d_rows; int16_t *d_pt, *d_stack; unsigned long long *d_hash; double *d_en, *d_enu, *d_h;
    int *d_rg, *d_p0, *d_np, *d_bad, *d_first, *d_rank, *d_frow, *d_nu, *d_uid, *d_ne, *d_m;
    const size_t n4 = (size_t)n * 4, g4 = (size_t)n_graphs * 4;
    if (int rc = mem.alloc(d_gs, gs.size() * sizeof(KinGraph))) return rc;
    if (int rc = mem.alloc(d_rows, bytes + 1)) return rc;
    if (int rc = mem.alloc(d_pt, (bytes + 1) * 2)) return rc;
    if (int rc = mem.alloc(d_stack, (bytes + 1) * 2)) return rc;
    if (int rc = mem.alloc(d_hash, n4 * 2)) return rc;
    if (int rc = mem.alloc(d_en, n4 * 2)) return rc;
    if (int rc = mem.alloc(d_enu, n4 * 2)) return rc;
    if (int rc = mem.alloc(d_rg, n4)) return rc;
    if (int rc = mem.alloc(d_p0, n4)) return rc;
    if (int rc = mem.alloc(d_np, n4)) return rc;
    if (int rc = mem.alloc(d_first, n4)) return rc;
    if (int rc = mem.alloc(d_rank, n4)) return rc;
    if (int rc = mem.alloc(d_frow, n4)) return rc;
    if (int rc = mem.alloc(d_uid, n4)) return rc;
    if (int rc = mem.alloc(d_bad, g4)) return rc;
    if (int rc = mem.alloc(d_nu, g4)) return rc;
    if (int rc = mem.alloc(d_ne, g4)) return rc;
    if (int rc = mem.alloc(d_m, (size_t)n_times * 4)) return rc;
    if (int rc = mem.alloc(d_h, (size_t)n_times * 8)) return rc;
    HIPCHK(hipMemcpyAsync(d_gs, gs.data(), gs.size() * sizeof(KinGraph), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_rows, pack.data(), bytes + 1, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_en, en.data(), n4 * 2, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_rg, row_graph.data(), n4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_p0, row_prev0.data(), n4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_np, row_nprev.data(), n4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_m, m, (size_t)n_times * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_h, h, (size_t)n_times * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_bad, 0, g4, st));
    HIPCHK(hipMemsetAsync(d_ne, 0, g4, st));
    HIPCHK(hipMemsetAsync(d_frow, 0xff, n4, st));            // -1: no such unique structure
    HIPCHK(hipMemsetAsync(d_rank, 0, n4, st));
    const unsigned nb64 = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(kin_batch_pair_table_kernel, dim3(nb64), dim3(64), 0, st, (int)n, d_gs, d_rg, d_rows, d_pt, d_stack, d_hash, d_bad);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(kin_batch_identity_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (int)n, d_gs, d_rg, d_rows, d_hash, d_first);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(kin_batch_rank_kernel, dim3((unsigned)n_graphs), dim3(256), 0, st, d_gs, d_first, d_en, d_rank, d_frow, d_enu, d_nu);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(kin_batch_uid_kernel, dim3(nb64), dim3(64), 0, st, (int)n, d_gs, d_rg, d_first, d_rank, d_uid);
    HIPCHK(hipGetLastError());
    std::vector<int> bad(n_graphs), nu(n_graphs);
    HIPCHK(hipMemcpyAsync(bad.data(), d_bad, g4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(nu.data(), d_nu, g4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(uid_out, d_uid, n4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(first_row_out, d_frow, n4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::string first_err;
    for (int g = 0; g < n_graphs; g++) {
        KinGraph &G = gs[g];
        if (bad[g]) {
            rec[g].status = RAFFT_ERR_STRUCT;
            if (first_err.empty()) first_err = "graph " + std::to_string(g) + ": malformed dot-bracket row";
        } else if (nu[g] > RAFFT_KIN_BATCH_MAX_STATES) {
            rec[g].status = RAFFT_ERR_CAPACITY;
            rec[g].n_unique = nu[g];
            if (first_err.empty())
                first_err = "graph " + std::to_string(g) + ": " + std::to_string(nu[g]) + " unique structures, the batch path takes up to " +
                            std::to_string(RAFFT_KIN_BATCH_MAX_STATES) + " - use the single-graph path (rafft_kin_rate_matrix and a dense or sparse solver)";
        } else {
            rec[g].n_unique = G.S = nu[g];
            continue;
        }
        for (int r = 0; r < G.n_rows; r++) uid_out[G.row0 + r] = first_row_out[G.row0 + r] = -1;
    }
    // chunks of consecutive graphs: three S x S blocks per graph and the populations of the chunk within the budget (one graph at least)
    const size_t budget = workspace_bytes > 0 ? (size_t)workspace_bytes : KIN_BATCH_WORKSPACE;
    struct Chunk { int ga, gb; };
    std::vector<Chunk> chunks;
    size_t ws_max = 0, pop_max = 0;
    for (int ga = 0; ga < n_graphs; ) {
        size_t w = 0, pp = 0;
        int gb = ga;
        while (gb < n_graphs) {
            const size_t dw = 3 * (size_t)gs[gb].S * gs[gb].S * 8, dp = (size_t)n_times * gs[gb].n_rows * 8;
            if (gb > ga && (w + dw > budget || pp + dp > budget)) break;
            gs[gb].mat = w / 8;
            w += dw; pp += dp; gb++;
        }
        chunks.push_back(Chunk{ga, gb});
        ws_max = std::max(ws_max, w); pop_max = std::max(pop_max, pp);
        ga = gb;
    }
    double *d_ws, *d_pop;
    if (int rc = mem.alloc(d_ws, ws_max + 8)) return rc;
    if (int rc = mem.alloc(d_pop, pop_max + 8)) return rc;
    HIPCHK(hipMemcpyAsync(d_gs, gs.data(), gs.size() * sizeof(KinGraph), hipMemcpyHostToDevice, st));
    constexpr size_t lds_small = (size_t)(4 * KIN_BATCH_LDS_STATES + 1 + KIN_BATCH_LDS_STATES * KIN_BATCH_LDS_STATES) * 8;
    constexpr size_t lds_big = (size_t)(4 * RAFFT_KIN_BATCH_MAX_STATES + 1) * 8;
    HIPCHK(hipFuncSetAttribute((const void *)kin_batch_integrate_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_small));
    // per chunk the graphs that are solved: those whose inverse fits LDS first, then the others
    std::vector<int> order(n_graphs), n_small(chunks.size()), n_big(chunks.size());
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        int at = chunks[ci].ga;
        for (int g = chunks[ci].ga; g < chunks[ci].gb; g++) if (gs[g].S && gs[g].S <= KIN_BATCH_LDS_STATES) order[at++] = g;
        n_small[ci] = at - chunks[ci].ga;
        for (int g = chunks[ci].ga; g < chunks[ci].gb; g++) if (gs[g].S > KIN_BATCH_LDS_STATES) order[at++] = g;
        n_big[ci] = at - chunks[ci].ga - n_small[ci];
    }
    int *d_order;
    if (int rc = mem.alloc(d_order, g4)) return rc;
    HIPCHK(hipMemcpyAsync(d_order, order.data(), g4, hipMemcpyHostToDevice, st));
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        const Chunk &c = chunks[ci];
        const int ra = gs[c.ga].row0, rb = c.gb < n_graphs ? gs[c.gb].row0 : (int)n;
        const int small = n_small[ci], big = n_big[ci];
        size_t w = 0;
        for (int g = c.ga; g < c.gb; g++) w += 3 * (size_t)gs[g].S * gs[g].S * 8;
        if (rb == ra) continue;
        if (!small && !big) { memset(pop_out + (size_t)n_times * ra, 0, (size_t)n_times * (rb - ra) * 8); continue; }
        HIPCHK(hipMemsetAsync(d_ws, 0, w, st));
        HIPCHK(hipMemsetAsync(d_pop, 0, (size_t)n_times * (rb - ra) * 8, st));
        hipLaunchKernelGGL(kin_batch_rates_kernel, dim3((unsigned)(rb - ra)), dim3(KIN_NT), (size_t)Lmax * 2, st, ra, d_gs, d_rg, d_p0, d_np, d_pt, d_uid, d_enu, kt, d_ws);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(kin_batch_diag_kernel, dim3((unsigned)(rb - ra)), dim3(256), 0, st, ra, d_gs, d_rg, d_ws, d_ne);
        HIPCHK(hipGetLastError());
        if (small) {
            hipLaunchKernelGGL(kin_batch_integrate_kernel<true>, dim3((unsigned)small), dim3(KINB_NT), lds_small, st, d_order + c.ga, ra, d_gs, d_ws, n_times, d_m, d_h, d_pop);
            HIPCHK(hipGetLastError());
        }
        if (big) {
            hipLaunchKernelGGL(kin_batch_integrate_kernel<false>, dim3((unsigned)big), dim3(KINB_NT), lds_big, st, d_order + c.ga + small, ra, d_gs, d_ws, n_times, d_m, d_h, d_pop);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(pop_out + (size_t)n_times * ra, d_pop, (size_t)n_times * (rb - ra) * 8, hipMemcpyDeviceToHost, st));
        if (rate_out)
            for (int g = c.ga; g < c.gb; g++)
                if (rate_out[g] && gs[g].S) HIPCHK(hipMemcpyAsync(rate_out[g], d_ws + gs[g].mat, (size_t)gs[g].S * gs[g].S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    std::vector<int> ne(n_graphs);
    HIPCHK(hipMemcpy(ne.data(), d_ne, g4, hipMemcpyDeviceToHost));
    for (int g = 0; g < n_graphs; g++) rec[g].n_edges = ne[g];
    g_err = first_err;
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

// ---- minimum-free-energy folds

constexpr size_t MFE_WORKSPACE = (size_t)512 << 20;

// rafft_mfe_batch (arguments validated by the entry point).  Sequences up to `lds_len` go through mfe_lds_kernel in one launch, the
// others through the HBM class in chunks whose tables fit the workspace budget (one sequence at least): per chunk one launch per
// anti-diagonal, then the traceback.  One synchronise at the end.
int mfe_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int lds_len, long long workspace_bytes, rafft_mfe_seq *seq_out,
              char *const *db_out)
{
    // as the fold's entry (validate_params): before any sequence is looked at, so a batch of nothing but erroneous sequences fails too
    if (!(temp > -273.15 && temp < 1000.0)) return fail(RAFFT_ERR_TEMP, "temp out of range");
    if (temp != 37.0 && !param_set().has_dH)
        return fail(RAFFT_ERR_TEMP, "temp != 37 needs the enthalpy tables of a ViennaRNA parameter file (rafft_load_params); the built-in tables are 37 C only");
    if (n_seq == 0) return 0;
    std::vector<MfeSeq> qs(n_seq);
    std::vector<int> lds_order, hbm_order;
    unsigned long long n_codes = 0, n_stack = 0, n_db = 0;
    std::string first_err;
    for (int s = 0; s < n_seq; s++) {
        int st = 0;
        if (lens[s] <= 0) st = RAFFT_ERR_EMPTY;
        else if (lens[s] > RAFFT_MFE_MAX_LEN) st = RAFFT_ERR_TOO_LONG;
        else for (int x = 0; x < lens[s] && !st; x++) if (kBaseCode[(unsigned char)seqs[s][x]] & 8) st = RAFFT_ERR_BAD_CHAR;
        const int len = lens[s] > 0 ? lens[s] : 0;
        seq_out[s] = rafft_mfe_seq{st, len, 0, 0};
        memset(db_out[s], '.', (size_t)len);
        db_out[s][len] = 0;
        qs[s] = MfeSeq{n_codes, 0, n_stack, n_db, st ? 0 : len, 0};
        if (st) {
            if (first_err.empty())
                first_err = "sequence " + std::to_string(s) + (st == RAFFT_ERR_EMPTY ? ": empty" : st == RAFFT_ERR_TOO_LONG ? ": longer than RAFFT_MFE_MAX_LEN" : ": character outside ACGUN");
            continue;
        }
        n_codes += (unsigned long long)len; n_stack += (unsigned long long)len + 8; n_db += (unsigned long long)len + 1;
        (len <= lds_len ? lds_order : hbm_order).push_back(s);
    }
    g_err = first_err;
    if (lds_order.empty() && hbm_order.empty()) return 0;
    std::vector<uint8_t> codes(n_codes + 16, 0);
    for (int s = 0; s < n_seq; s++)
        for (int x = 0; x < qs[s].L; x++) codes[qs[s].code_off + x] = (uint8_t)(kBaseCode[(unsigned char)seqs[s][x]] & 7);
    // the longest first: the workgroups of a launch that run last are the short ones
    std::stable_sort(lds_order.begin(), lds_order.end(), [&](int a, int b) { return qs[a].L > qs[b].L; });
    // chunks of the HBM class, in input order
    const size_t budget = workspace_bytes > 0 ? (size_t)workspace_bytes : MFE_WORKSPACE;
    struct Chunk { size_t a, b; int Lmax; };
    std::vector<Chunk> chunks;
    size_t ws_max = 0;
    for (size_t a = 0; a < hbm_order.size();) {
        size_t w = 0, b = a;
        int Lmax = 0;
        while (b < hbm_order.size() && b - a < 65535) {
            MfeSeq &q = qs[hbm_order[b]];
            const size_t dw = 3 * (size_t)q.L * q.L * 4;
            if (b > a && w + dw > budget) break;
            q.tab_off = w / 4;
            w += dw; Lmax = std::max(Lmax, q.L); b++;
        }
        chunks.push_back(Chunk{a, b, Lmax});
        ws_max = std::max(ws_max, w);
        a = b;
    }
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    if (int rc = ensure_tables(temp)) return rc;
    hipStream_t st = sg.stream;
    DevScratch mem;
    MfeSeq *d_qs; uint8_t *d_codes; uint32_t *d_stack; char *d_db; int4 *d_rec; int *d_order, *d_ws = nullptr;
    std::vector<int> order(lds_order);
    order.insert(order.end(), hbm_order.begin(), hbm_order.end());
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(MfeSeq))) return rc;
    if (int rc = mem.alloc(d_codes, codes.size())) return rc;
    if (int rc = mem.alloc(d_stack, n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_db, n_db + 16)) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(int4))) return rc;
    if (int rc = mem.alloc(d_order, order.size() * 4)) return rc;
    if (ws_max) if (int rc = mem.alloc(d_ws, ws_max + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(MfeSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_codes, codes.data(), codes.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(int4), st));
    if (!lds_order.empty()) {
        HIPCHK(hipFuncSetAttribute((const void *)mfe_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MFE_LDS_BYTES));
        hipLaunchKernelGGL(mfe_lds_kernel, dim3((unsigned)lds_order.size()), dim3(MFE_LDS_NT), (size_t)mfe_lds_bytes(qs[lds_order[0]].L), st, g.T, d_qs, d_order,
                           d_codes, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    for (const Chunk &c : chunks) {
        const int *ord = d_order + lds_order.size() + c.a;
        const unsigned ny = (unsigned)(c.b - c.a);
        for (int d = 0; d < c.Lmax; d++) {
            const unsigned nx = (unsigned)std::min((c.Lmax - d + MFE_HBM_NT / 64 - 1) / (MFE_HBM_NT / 64), 1024);
            hipLaunchKernelGGL(mfe_diag_kernel, dim3(nx, ny), dim3(MFE_HBM_NT), 0, st, g.T, d_qs, ord, d_codes, d_ws, d);
        }
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mfe_traceback_kernel, dim3(ny), dim3(64), 0, st, g.T, d_qs, ord, d_codes, d_ws, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    std::vector<int4> rec(n_seq);
    std::vector<char> db(n_db + 16);
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, qs.size() * sizeof(int4), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(db.data(), d_db, n_db, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < n_seq; s++) {
        if (seq_out[s].status) continue;
        if (rec[s].z) return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + ": the traceback found no candidate for a cell");
        seq_out[s].dcal = rec[s].x; seq_out[s].n_pairs = rec[s].y;
        memcpy(db_out[s], db.data() + qs[s].db_off, (size_t)qs[s].L + 1);
    }
    g_err = first_err;
    return 0;
}

// ---- partition function and pair probabilities

constexpr size_t PF_WORKSPACE = (size_t)512 << 20;

// rafft_pf_batch (arguments validated by the entry point).  The MFE of every sequence first (mfe_batch: its errors are this call's,
// its energy gives the scale), then chunks of whole sequences in input order whose six L x L fp64 tables fit the workspace budget
// (one sequence at least): per chunk one launch per anti-diagonal upwards, the exterior sums, one launch per anti-diagonal downwards,
// the probabilities.  One synchronise at the end.
int pf_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, long long workspace_bytes, rafft_pf_seq *seq_out,
             char *const *db_out, double *const *prob_out)
{
    std::vector<rafft_mfe_seq> mfe(std::max(n_seq, 1));
    if (int rc = mfe_batch(n_seq, seqs, lens, temp, RAFFT_MFE_LDS_LEN, workspace_bytes, mfe.data(), db_out)) return rc;
    if (n_seq == 0) return 0;
    const std::string first_err = g_err;
    const double kt = (temp + 273.15) * PF_GAS, beta = 1.0 / (100.0 * kt), sf = scale_factor > 0.0 ? scale_factor : 1.07;
    std::vector<PfSeq> qs(n_seq);
    std::vector<int> order;
    unsigned long long n_codes = 0, n_aux = 0, n_db = 0;
    for (int s = 0; s < n_seq; s++) {
        const int len = mfe[s].length;
        seq_out[s] = rafft_pf_seq{mfe[s].status, len, mfe[s].dcal, 0, 0.0, 0.0};
        memset(db_out[s], '.', (size_t)len);
        db_out[s][len] = 0;
        if (prob_out && prob_out[s]) memset(prob_out[s], 0, (size_t)len * len * sizeof(double));
        const int L = mfe[s].status ? 0 : len;
        const double ln_scale = L ? -sf * ((double)mfe[s].dcal / 100.0) / (kt * (double)L) : 0.0;
        const double scale = std::exp(ln_scale);
        qs[s] = PfSeq{n_codes, 0, n_aux, n_db, L, mfe[s].dcal, scale, std::log(scale)};
        if (!L) continue;
        n_codes += (unsigned long long)L; n_aux += 4 * ((unsigned long long)L + 1); n_db += (unsigned long long)L + 1;
        order.push_back(s);
    }
    if (order.empty()) return 0;
    std::vector<uint8_t> codes(n_codes + 16, 0);
    for (int s = 0; s < n_seq; s++)
        for (int x = 0; x < qs[s].L; x++) codes[qs[s].code_off + x] = (uint8_t)(kBaseCode[(unsigned char)seqs[s][x]] & 7);
    const size_t budget = workspace_bytes > 0 ? (size_t)workspace_bytes : PF_WORKSPACE;
    struct Chunk { size_t a, b; int Lmax; };
    std::vector<Chunk> chunks;
    size_t ws_max = 0;
    for (size_t a = 0; a < order.size();) {
        size_t w = 0, b = a;
        int Lmax = 0;
        while (b < order.size() && b - a < 65535) {
            PfSeq &q = qs[order[b]];
            const size_t dw = 6 * (size_t)q.L * q.L * sizeof(double);
            if (b > a && w + dw > budget) break;
            q.tab_off = w / sizeof(double);
            w += dw; Lmax = std::max(Lmax, q.L); b++;
        }
        chunks.push_back(Chunk{a, b, Lmax});
        ws_max = std::max(ws_max, w);
        a = b;
    }
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    if (int rc = ensure_tables(temp)) return rc;
    hipStream_t st = sg.stream;
    DevScratch mem;
    PfSeq *d_qs; uint8_t *d_codes; double *d_aux, *d_ws; char *d_db; PfRec *d_rec; int *d_order;
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(PfSeq))) return rc;
    if (int rc = mem.alloc(d_codes, codes.size())) return rc;
    if (int rc = mem.alloc(d_aux, n_aux * sizeof(double) + 16)) return rc;
    if (int rc = mem.alloc(d_db, n_db + 16)) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(PfRec))) return rc;
    if (int rc = mem.alloc(d_order, order.size() * 4)) return rc;
    if (int rc = mem.alloc(d_ws, ws_max + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(PfSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_codes, codes.data(), codes.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(PfRec), st));
    hipLaunchKernelGGL(pf_powers_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, st, g.T, d_qs, n_seq, d_aux, beta);
    HIPCHK(hipGetLastError());
    for (const Chunk &c : chunks) {
        const int *ord = d_order + c.a;
        const unsigned ny = (unsigned)(c.b - c.a);
        const auto nx = [&](int d) { return (unsigned)std::min((c.Lmax - d + PF_NT / 64 - 1) / (PF_NT / 64), 1024); };
        for (int d = 0; d < c.Lmax; d++)
            hipLaunchKernelGGL(pf_diag_kernel, dim3(nx(d), ny), dim3(PF_NT), 0, st, g.T, d_qs, ord, d_codes, d_ws, d_aux, beta, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pf_exterior_kernel, dim3(ny), dim3(64), 0, st, g.T, d_qs, ord, d_codes, d_ws, d_aux, beta, kt, d_db, d_rec);
        HIPCHK(hipGetLastError());
        for (int d = c.Lmax - 1; d >= 4; d--)
            hipLaunchKernelGGL(pf_out_diag_kernel, dim3(nx(d), ny), dim3(PF_NT), 0, st, g.T, d_qs, ord, d_codes, d_ws, d_aux, beta, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pf_prob_kernel, dim3(nx(0), ny), dim3(PF_NT), 0, st, d_qs, ord, d_ws, d_aux, d_db, d_rec);
        HIPCHK(hipGetLastError());
        if (prob_out)
            for (size_t k = c.a; k < c.b; k++) {
                const PfSeq &q = qs[order[k]];
                if (prob_out[order[k]])
                    HIPCHK(hipMemcpyAsync(prob_out[order[k]], d_ws + q.tab_off + 3 * (size_t)q.L * q.L, (size_t)q.L * q.L * sizeof(double), hipMemcpyDeviceToHost, st));
            }
    }
    std::vector<PfRec> rec(n_seq);
    std::vector<char> db(n_db + 16);
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, qs.size() * sizeof(PfRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(db.data(), d_db, n_db, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::string err = first_err;
    for (int s = 0; s < n_seq; s++) {
        if (seq_out[s].status) continue;
        if (rec[s].status || rec[s].bad) {
            // the scaled tables left the fp64 range: no number of this sequence is reported
            seq_out[s].status = RAFFT_ERR_CAPACITY;
            if (prob_out && prob_out[s]) memset(prob_out[s], 0, (size_t)qs[s].L * qs[s].L * sizeof(double));
            if (err.empty()) err = "sequence " + std::to_string(s) + ": the scaled partition function left the fp64 range (another scale_factor may hold it)";
            continue;
        }
        seq_out[s].n_pairs = rec[s].n_pairs;
        seq_out[s].energy = rec[s].energy;
        seq_out[s].mfe_frequency = rec[s].mfe_frequency;
        memcpy(db_out[s], db.data() + qs[s].db_off, (size_t)qs[s].L + 1);
    }
    g_err = err;
    return 0;
}

} // namespace
