// rafft_batch.h - the batch drivers: seam calls that take many items in one call and cut them into chunks whose tables fit a
// workspace budget (workspace_budget).  Fifteen of them:
//   kin_batch                    folding kinetics of many graphs
//   mfe_batch, mfe_span_batch    minimum-free-energy folds; the same under a base-pair span, to 32768 nt
//   mfe_con_batch                the folds of mfe_batch under hard constraints and soft terms
//   cofold_batch                 the folds of mfe_batch for two-strand dimers
//   pf_batch, pf_span_batch      partition function and pair probabilities; the same under a span, to 32768 nt
//   pf_con_batch                 the same under hard constraints and soft terms
//   mea_batch, mea_probs_batch   maximum-expected-accuracy structures, of sequences and of given probabilities
//   sample_batch                 structures drawn from the ensemble
//   subopt_batch                 every structure within an energy band
//   findpath_batch               folding barriers between structure pairs
//   descend_batch, barriers_batch, kinfold_batch    the row drivers: gradient walks to local minima, exact barrier trees of
//                                energy bands, stochastic folding trajectories
// What they plan without the device - the chunks, the sequence pack, the graph pack, the solve order of a chunk, the scale of a
// partition function, and every offset their kernels dereference (the *_layout functions) - is in rafft_hostpure.h, where the CPU
// suite checks it: here are the allocations, the copies and the launches.  The drivers that take sequences share their opening
// (SeqCall) and their view of a chunk (ChunkView); the fold drivers also share the MFE of a pack under the caller's guard
// (mfe_held, mfe_span_held) and their tails (mfe_results, pf_results).
// Part of the single translation unit of rafft_api.hip (included there, after rafft_seam.h, whose SeamGuard and DevScratch they use).
#pragma once

namespace {

// the workspace budget of a call: its workspace_bytes, or the default of every batch call when that is 0
constexpr size_t DEFAULT_WORKSPACE = (size_t)512 << 20;
size_t workspace_budget(long long workspace_bytes) { return workspace_bytes > 0 ? (size_t)workspace_bytes : DEFAULT_WORKSPACE; }

// ---- kinetics of a batch of graphs

// rafft_kin_batch (arguments validated by the entry point).  Two passes over the device: structure identity for every graph, then -
// the numbers of unique structures being known - rates and integration for chunks of graphs whose matrices fit the workspace budget.
int kin_batch(int n_graphs, const int *lens, const int *n_steps, const int *const *step_size, const char *const *rows, const int *row_stride,
              const double *const *energy, double kt, int n_times, const int *m, const double *h, long long workspace_bytes,
              rafft_kin_graph *rec, int *uid_out, int *first_row_out, double *pop_out, double *const *rate_out)
{
    KinPack pk;
    if (!kin_pack(n_graphs, lens, n_steps, step_size, rows, row_stride, energy, pk)) return fail(RAFFT_ERR_PARAM, "too many rows");
    const long long n = pk.n;
    const unsigned long long bytes = pk.bytes;
    std::vector<KinGraph> gs(n_graphs);
    int Lmax = 0;
    for (int g = 0; g < n_graphs; g++) {
        gs[g] = KinGraph{pk.off[g], 0, lens[g], pk.n_rows[g], pk.row0[g], 0};
        rec[g] = rafft_kin_graph{0, pk.n_rows[g], pk.row0[g], 0, 0, 0};
        if (pk.n_rows[g]) Lmax = std::max(Lmax, lens[g]);
    }
    if (n == 0) return 0;
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
    HIPCHK(hipMemcpyAsync(d_rows, pk.rows.data(), bytes + 1, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_en, pk.energy.data(), n4 * 2, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_rg, pk.row_graph.data(), n4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_p0, pk.row_prev0.data(), n4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_np, pk.row_nprev.data(), n4, hipMemcpyHostToDevice, st));
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
    const size_t budget = workspace_budget(workspace_bytes);
    std::vector<int> S(n_graphs);
    std::vector<size_t> mat_bytes(n_graphs), pop_bytes(n_graphs);
    for (int g = 0; g < n_graphs; g++) {
        S[g] = gs[g].S;
        mat_bytes[g] = 3 * (size_t)S[g] * S[g] * 8;
        pop_bytes[g] = (size_t)n_times * gs[g].n_rows * 8;
    }
    const ChunkPlan plan = plan_chunks((size_t)n_graphs, mat_bytes.data(), pop_bytes.data(), budget, 0);
    for (int g = 0; g < n_graphs; g++) gs[g].mat = plan.off[g] / 8;
    double *d_ws, *d_pop;
    if (int rc = mem.alloc(d_ws, plan.max_cost + 8)) return rc;
    if (int rc = mem.alloc(d_pop, plan.max_cost2 + 8)) return rc;
    HIPCHK(hipMemcpyAsync(d_gs, gs.data(), gs.size() * sizeof(KinGraph), hipMemcpyHostToDevice, st));
    constexpr size_t lds_small = (size_t)(4 * KIN_BATCH_LDS_STATES + 1 + KIN_BATCH_LDS_STATES * KIN_BATCH_LDS_STATES) * 8;
    constexpr size_t lds_big = (size_t)(4 * RAFFT_KIN_BATCH_MAX_STATES + 1) * 8;
    HIPCHK(hipFuncSetAttribute((const void *)kin_batch_integrate_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_small));
    // per chunk the graphs that are solved: those whose inverse fits LDS first, then the others
    std::vector<int> order(n_graphs);
    std::vector<SolveCounts> solved(plan.chunks.size());
    for (size_t ci = 0; ci < plan.chunks.size(); ci++)
        solved[ci] = kin_solve_order(S.data(), plan.chunks[ci].a, plan.chunks[ci].b, KIN_BATCH_LDS_STATES, order.data());
    int *d_order;
    if (int rc = mem.alloc(d_order, g4)) return rc;
    HIPCHK(hipMemcpyAsync(d_order, order.data(), g4, hipMemcpyHostToDevice, st));
    for (size_t ci = 0; ci < plan.chunks.size(); ci++) {
        const ChunkPlan::Range &c = plan.chunks[ci];
        const int ra = gs[c.a].row0, rb = c.b < (size_t)n_graphs ? gs[c.b].row0 : (int)n;
        const int small = solved[ci].n_small, big = solved[ci].n_big;
        size_t w = 0;
        for (size_t g = c.a; g < c.b; g++) w += mat_bytes[g];
        if (rb == ra) continue;
        if (!small && !big) { memset(pop_out + (size_t)n_times * ra, 0, (size_t)n_times * (rb - ra) * 8); continue; }
        HIPCHK(hipMemsetAsync(d_ws, 0, w, st));
        HIPCHK(hipMemsetAsync(d_pop, 0, (size_t)n_times * (rb - ra) * 8, st));
        hipLaunchKernelGGL(kin_batch_rates_kernel, dim3((unsigned)(rb - ra)), dim3(KIN_NT), (size_t)Lmax * 2, st, ra, d_gs, d_rg, d_p0, d_np, d_pt, d_uid, d_enu, kt, d_ws);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(kin_batch_diag_kernel, dim3((unsigned)(rb - ra)), dim3(256), 0, st, ra, d_gs, d_rg, d_ws, d_ne);
        HIPCHK(hipGetLastError());
        if (small) {
            hipLaunchKernelGGL(kin_batch_integrate_kernel<true>, dim3((unsigned)small), dim3(KINB_NT), lds_small, st, d_order + c.a, ra, d_gs, d_ws, n_times, d_m, d_h, d_pop);
            HIPCHK(hipGetLastError());
        }
        if (big) {
            hipLaunchKernelGGL(kin_batch_integrate_kernel<false>, dim3((unsigned)big), dim3(KINB_NT), lds_big, st, d_order + c.a + small, ra, d_gs, d_ws, n_times, d_m, d_h, d_pop);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(pop_out + (size_t)n_times * ra, d_pop, (size_t)n_times * (rb - ra) * 8, hipMemcpyDeviceToHost, st));
        if (rate_out)
            for (size_t g = c.a; g < c.b; g++)
                if (rate_out[g] && gs[g].S) HIPCHK(hipMemcpyAsync(rate_out[g], d_ws + gs[g].mat, (size_t)gs[g].S * gs[g].S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    std::vector<int> ne(n_graphs);
    HIPCHK(hipMemcpy(ne.data(), d_ne, g4, hipMemcpyDeviceToHost));
    for (int g = 0; g < n_graphs; g++) rec[g].n_edges = ne[g];
    g_err = first_err;
    return 0;
}

// ---- what the drivers that take sequences share

// as the fold's entry (validate_params): before any sequence is looked at, so a batch of nothing but erroneous sequences fails too
int check_temp(double temp)
{
    if (!(temp > -273.15 && temp < 1000.0)) return fail(RAFFT_ERR_TEMP, "temp out of range");
    if (temp != 37.0 && !param_set().has_dH)
        return fail(RAFFT_ERR_TEMP, "temp != 37 needs the enthalpy tables of a ViennaRNA parameter file (rafft_load_params); the built-in tables are 37 C only");
    return 0;
}

// a row of dots for a sequence of `len` (what a sequence with an error keeps)
void dot_row(char *db, int len)
{
    memset(db, '.', (size_t)len);
    db[len] = 0;
}

// The opening of a call that has something to fold, in this order: the seam's entry, the device tables scaled for the call's temp,
// the device copy of pk.codes in the caller's DevScratch (declared after the SeqCall, so that it is freed under the guard).
struct SeqCall {
    SeamGuard sg;
    hipStream_t st = nullptr;
    uint8_t *d_codes = nullptr;
    int open(DevScratch &mem, const SeqPack &pk, double temp)
    {
        if (int rc = sg.enter()) return rc;
        if (int rc = ensure_tables(temp)) return rc;
        st = sg.stream;
        if (int rc = mem.alloc(d_codes, pk.codes.size())) return rc;
        HIPCHK(hipMemcpyAsync(d_codes, pk.codes.data(), pk.codes.size(), hipMemcpyHostToDevice, st));
        return 0;
    }
};

// chunk c of a plan over `order` (d_order: where the device copy of order[0] lies): its part of the order, its sequences, its longest
struct ChunkView { const int *ord; unsigned ny; int Lmax; };
ChunkView chunk_view(const ChunkPlan::Range &c, const int *d_order, const std::vector<int> &order, const SeqPack &pk)
{
    return ChunkView{d_order + c.a, (unsigned)(c.b - c.a), chunk_lmax(c, order, pk.L)};
}

// Sequence s's scaled tables left the fp64 range, so no number of it is reported: its status, the call's first error if it has
// none yet, and `bytes` zeros over what it was given for its numbers (zero may be null)
void pf_left_range(int s, int &status, std::string &err, void *zero, size_t bytes)
{
    status = RAFFT_ERR_CAPACITY;
    if (zero) memset(zero, 0, bytes);
    if (err.empty()) err = "sequence " + std::to_string(s) + ": the scaled partition function left the fp64 range (another scale_factor may hold it)";
}

// ---- minimum-free-energy folds

// The HBM-class tables of a chunk (its sequences' numbers in d_qs): one launch per anti-diagonal, stream order being the
// synchronisation.  mfe_held and subopt_batch fill their tables through this.
int mfe_fill_chunk(hipStream_t st, const MfeSeq *d_qs, const ChunkView &v, const uint8_t *d_codes, int *d_ws)
{
    for (int d = 0; d < v.Lmax; d++) {
        const unsigned nx = (unsigned)std::min((v.Lmax - d + MFE_HBM_NT / 64 - 1) / (MFE_HBM_NT / 64), 1024);
        hipLaunchKernelGGL(mfe_diag_kernel, dim3(nx, v.ny), dim3(MFE_HBM_NT), 0, st, g.T, d_qs, v.ord, d_codes, d_ws, d);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// What mfe_held and mfe_span_held end with: the tracebacks' records and the n_db bytes of rows come down, one synchronise, and
// every sequence without an error gets its dcal, its n_pairs, - db_out may be null (no rows wanted) - its row and - soft_out may
// be null - the soft part of its dcal (mfe_con_held).
template <class Seq>
int mfe_results(hipStream_t st, const std::vector<Seq> &qs, const int4 *d_rec, const char *d_db, unsigned long long n_db, rafft_mfe_seq *seq_out,
                char *const *db_out, int *soft_out = nullptr)
{
    const int n_seq = (int)qs.size();
    std::vector<int4> rec(n_seq);
    std::vector<char> db(n_db + 16);
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, qs.size() * sizeof(int4), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(db.data(), d_db, n_db, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < n_seq; s++) {
        if (seq_out[s].status) continue;
        if (rec[s].z) return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + ": the traceback found no candidate for a cell");
        seq_out[s].dcal = rec[s].x; seq_out[s].n_pairs = rec[s].y;
        if (soft_out) soft_out[s] = rec[s].w;
        if (db_out) memcpy(db_out[s], db.data() + qs[s].db_off, (size_t)qs[s].L + 1);
    }
    return 0;
}

// The MFE folds of a pack, under the caller's guard: the device tables are scaled for the call's temp, d_codes is the device copy
// of pk.codes, seq_out[s].status is set.  Sequences up to `lds_len` go through mfe_lds_kernel in one launch, the others through
// the HBM class in chunks whose tables fit the workspace budget (one sequence at least; mfe_layout): per chunk one launch per
// anti-diagonal, then the traceback.  One synchronise at the end; its device buffers are freed on return.  db_out may be null (no
// rows wanted).
int mfe_held(hipStream_t st, const SeqPack &pk, const uint8_t *d_codes, int lds_len, long long workspace_bytes, rafft_mfe_seq *seq_out, char *const *db_out)
{
    const MfeLayout y = mfe_layout(pk, lds_len, workspace_budget(workspace_bytes));
    const std::vector<MfeSeq> &qs = y.qs;
    DevScratch mem;
    MfeSeq *d_qs; uint32_t *d_stack; char *d_db; int4 *d_rec; int *d_order, *d_ws = nullptr;
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(MfeSeq))) return rc;
    if (int rc = mem.alloc(d_stack, y.n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_db, y.n_db + 16)) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(int4))) return rc;
    if (int rc = mem.alloc(d_order, y.order.size() * 4)) return rc;
    if (y.plan.max_cost) if (int rc = mem.alloc(d_ws, y.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(MfeSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, y.order.data(), y.order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(int4), st));
    if (!y.lds_order.empty()) {
        HIPCHK(hipFuncSetAttribute((const void *)mfe_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MFE_LDS_BYTES));
        hipLaunchKernelGGL(mfe_lds_kernel, dim3((unsigned)y.lds_order.size()), dim3(MFE_LDS_NT), (size_t)mfe_lds_bytes(qs[y.lds_order[0]].L), st, g.T, d_qs, d_order,
                           d_codes, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        const ChunkView v = chunk_view(c, d_order + y.lds_order.size(), y.hbm_order, pk);
        if (int rc = mfe_fill_chunk(st, d_qs, v, d_codes, d_ws)) return rc;
        hipLaunchKernelGGL(mfe_traceback_kernel, dim3(v.ny), dim3(64), 0, st, g.T, d_qs, v.ord, d_codes, d_ws, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    return mfe_results(st, qs, d_rec, d_db, y.n_db, seq_out, db_out);
}

// rafft_mfe_batch (arguments validated by the entry point)
int mfe_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int lds_len, long long workspace_bytes, rafft_mfe_seq *seq_out,
              char *const *db_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);
    for (int s = 0; s < n_seq; s++) {
        seq_out[s] = rafft_mfe_seq{pk.status[s], pk.len[s], 0, 0};
        dot_row(db_out[s], pk.len[s]);
    }
    g_err = pk.first_err;
    if (pk.fold.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    if (int rc = mfe_held(sc.st, pk, sc.d_codes, lds_len, workspace_bytes, seq_out, db_out)) return rc;
    g_err = pk.first_err;
    return 0;
}

// ---- minimum-free-energy folds under constraints and soft terms

// The constrained MFE folds of a pack, under the caller's guard, as mfe_held: the same layout, classes and chunks, the mfe_con_*
// kernels in place of the mfe_* ones, the packs of `cp` (constraint_pack; no sequence of it has an error that pk does not know)
// in device memory.  mfe[s] gets dcal and n_pairs - a dcal of MFE_INF: the sequence has no structure and its row is all dots -
// and soft[s] the soft part of dcal.
int mfe_con_held(hipStream_t st, const SeqPack &pk, const uint8_t *d_codes, const ConstraintPack &cp, int lds_len, long long workspace_bytes,
                 rafft_mfe_seq *mfe, int *soft, char *const *db_out)
{
    const MfeLayout y = mfe_layout(pk, lds_len, workspace_budget(workspace_bytes));
    const std::vector<MfeSeq> &qs = y.qs;
    DevScratch mem;
    MfeSeq *d_qs; uint32_t *d_stack; char *d_db; int4 *d_rec; int *d_order, *d_ws = nullptr, *d_packs; unsigned long long *d_off;
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(MfeSeq))) return rc;
    if (int rc = mem.alloc(d_stack, y.n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_db, y.n_db + 16)) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(int4))) return rc;
    if (int rc = mem.alloc(d_order, y.order.size() * 4)) return rc;
    if (int rc = mem.alloc(d_packs, cp.data.size() * 4)) return rc;
    if (int rc = mem.alloc(d_off, cp.off.size() * 8)) return rc;
    if (y.plan.max_cost) if (int rc = mem.alloc(d_ws, y.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(MfeSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, y.order.data(), y.order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_packs, cp.data.data(), cp.data.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off, cp.off.data(), cp.off.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(int4), st));
    if (!y.lds_order.empty()) {
        HIPCHK(hipFuncSetAttribute((const void *)mfe_con_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MFE_CON_LDS_BYTES));
        hipLaunchKernelGGL(mfe_con_lds_kernel, dim3((unsigned)y.lds_order.size()), dim3(MFE_LDS_NT), (size_t)mfe_con_lds_bytes(qs[y.lds_order[0]].L), st, g.T, d_qs,
                           d_order, d_codes, d_off, d_packs, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        const ChunkView v = chunk_view(c, d_order + y.lds_order.size(), y.hbm_order, pk);
        for (int d = 0; d < v.Lmax; d++) {
            const unsigned nx = (unsigned)std::min((v.Lmax - d + MFE_HBM_NT / 64 - 1) / (MFE_HBM_NT / 64), 1024);
            hipLaunchKernelGGL(mfe_con_diag_kernel, dim3(nx, v.ny), dim3(MFE_HBM_NT), 0, st, g.T, d_qs, v.ord, d_codes, d_off, d_packs, d_ws, d);
        }
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mfe_con_traceback_kernel, dim3(v.ny), dim3(64), 0, st, g.T, d_qs, v.ord, d_codes, d_off, d_packs, d_ws, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    return mfe_results(st, qs, d_rec, d_db, y.n_db, mfe, db_out, soft);
}

// rafft_mfe_constrained_batch (arguments validated by the entry point)
int mfe_con_batch(int n_seq, const char *const *seqs, const int *lens, double temp, const char *const *constraints, const int32_t *const *soft_unpaired,
                  const int32_t *const *soft_stack, int lds_len, long long workspace_bytes, rafft_mfe_con_seq *seq_out, char *const *db_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);
    const ConstraintPack cp = constraint_pack(n_seq, pk.L.data(), pk.codes.data(), pk.code_off.data(), constraints, soft_unpaired, soft_stack);
    if (cp.param_seq >= 0) return fail(RAFFT_ERR_PARAM, cp.first_err);
    // an error of a sequence's constraints is an error of the sequence: it is not folded, and the first error in input order is named
    if (cp.first_seq >= 0) {
        int first = 0;
        while (first < n_seq && !pk.status[first]) first++;
        if (cp.first_seq < first) pk.first_err = cp.first_err;
        for (int s = 0; s < n_seq; s++)
            if (cp.status[s]) { pk.status[s] = cp.status[s]; pk.L[s] = 0; }
        pk.fold.erase(std::remove_if(pk.fold.begin(), pk.fold.end(), [&](int s) { return cp.status[s] != 0; }), pk.fold.end());
    }
    for (int s = 0; s < n_seq; s++) {
        seq_out[s] = rafft_mfe_con_seq{pk.status[s], pk.len[s], 0, 0, 0, 0};
        dot_row(db_out[s], pk.len[s]);
    }
    g_err = pk.first_err;
    if (pk.fold.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    std::vector<rafft_mfe_seq> mfe(n_seq);
    std::vector<int> soft(n_seq, 0);
    for (int s = 0; s < n_seq; s++) mfe[s] = rafft_mfe_seq{pk.status[s], pk.len[s], 0, 0};
    if (int rc = mfe_con_held(sc.st, pk, sc.d_codes, cp, lds_len, workspace_bytes, mfe.data(), soft.data(), db_out)) return rc;
    std::string err = pk.first_err;
    int first = 0;
    while (first < n_seq && !pk.status[first]) first++;
    for (int s = 0; s < n_seq; s++) {
        if (pk.status[s]) continue;
        if (mfe[s].dcal >= MFE_INFH) {
            seq_out[s].status = RAFFT_ERR_INFEASIBLE;
            if (s < first) { first = s; err = "sequence " + std::to_string(s) + ": no structure satisfies its constraints"; }
            continue;
        }
        seq_out[s].dcal = mfe[s].dcal; seq_out[s].n_pairs = mfe[s].n_pairs; seq_out[s].pseudo_dcal = soft[s];
    }
    g_err = err;
    return 0;
}

// ---- minimum-free-energy folds of two-strand dimers

// duplex_init of the parameter set in force at `temp` (check_temp passed): the file's DuplexInit scaled with its enthalpy like
// every other scalar; the built-in tables store none and take Turner 2004's 4.1 kcal/mol at 37 C.  A constant of the cofold
// code, handed to its kernels as an argument: no table set holds it.
#define COFOLD_DUPLEX_INIT_T04 410
int cofold_duplex_init(double temp)
{
    const rafft_par::ParamSet &P = param_set();
    if (P.builtin_set) return COFOLD_DUPLEX_INIT_T04;
    if (temp == 37.0 || !P.has_dH) return P.duplex_init[0];
    return rafft_par::rescale(P.duplex_init[0], P.duplex_init[1], (temp + rafft_par::K0) / rafft_par::TMEASURE);
}

// The dimer folds of a pack, under the caller's guard, as mfe_held: the same layout, classes and chunks, the cofold_* kernels in
// place of the mfe_* ones, cut[s] (cut_pack; 0: a single strand) in device memory.  The HBM class per chunk: one launch per
// anti-diagonal over the intra cells, cofold_ends_kernel, one launch per anti-diagonal over the cross cells - the last two only
// if a sequence of the chunk has a cut - then the traceback.  inter[s]: the pairs of the row that span the nick.
int cofold_held(hipStream_t st, const SeqPack &pk, const uint8_t *d_codes, const std::vector<int> &cut, int dinit, int lds_len, long long workspace_bytes,
                rafft_mfe_seq *mfe, int *inter, char *const *db_out)
{
    const MfeLayout y = mfe_layout(pk, lds_len, workspace_budget(workspace_bytes));
    const std::vector<MfeSeq> &qs = y.qs;
    DevScratch mem;
    MfeSeq *d_qs; uint32_t *d_stack; char *d_db; int4 *d_rec; int *d_order, *d_ws = nullptr, *d_cut, *d_ends;
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(MfeSeq))) return rc;
    if (int rc = mem.alloc(d_stack, y.n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_ends, y.n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_db, y.n_db + 16)) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(int4))) return rc;
    if (int rc = mem.alloc(d_order, y.order.size() * 4)) return rc;
    if (int rc = mem.alloc(d_cut, cut.size() * 4)) return rc;
    if (y.plan.max_cost) if (int rc = mem.alloc(d_ws, y.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(MfeSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, y.order.data(), y.order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_cut, cut.data(), cut.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(int4), st));
    if (!y.lds_order.empty()) {
        HIPCHK(hipFuncSetAttribute((const void *)cofold_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, COFOLD_LDS_BYTES));
        hipLaunchKernelGGL(cofold_lds_kernel, dim3((unsigned)y.lds_order.size()), dim3(MFE_LDS_NT), (size_t)cofold_lds_bytes(qs[y.lds_order[0]].L), st, g.T, d_qs,
                           d_order, d_codes, d_cut, dinit, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        const ChunkView v = chunk_view(c, d_order + y.lds_order.size(), y.hbm_order, pk);
        bool dimers = false;
        for (size_t k = c.a; k < c.b; k++) dimers |= cut[y.hbm_order[k]] != 0;
        for (int cross = 0; cross <= (dimers ? 1 : 0); cross++) {
            for (int d = cross; d < v.Lmax; d++) {
                const unsigned nx = (unsigned)std::min((v.Lmax - d + MFE_HBM_NT / 64 - 1) / (MFE_HBM_NT / 64), 1024);
                hipLaunchKernelGGL(cofold_diag_kernel, dim3(nx, v.ny), dim3(MFE_HBM_NT), 0, st, g.T, d_qs, v.ord, d_codes, d_cut, dinit, d_ends, d_ws, d, cross);
            }
            HIPCHK(hipGetLastError());
            if (!cross && dimers) {
                hipLaunchKernelGGL(cofold_ends_kernel, dim3(v.ny), dim3(64), 0, st, g.T, d_qs, v.ord, d_codes, d_cut, d_ends, d_ws);
                HIPCHK(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(cofold_traceback_kernel, dim3(v.ny), dim3(64), 0, st, g.T, d_qs, v.ord, d_codes, d_cut, dinit, d_ends, d_ws, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    return mfe_results(st, qs, d_rec, d_db, y.n_db, mfe, db_out, inter);
}

// rafft_cofold_batch (arguments validated by the entry point)
int cofold_batch(int n_seq, const char *const *seqs, const int *lens, const int *cuts, double temp, int lds_len, long long workspace_bytes, rafft_cofold_seq *seq_out,
                 char *const *db_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);
    const CutPack cp = cut_pack(n_seq, pk.L.data(), cuts);
    // a bad cut is an error of the sequence: it is not folded, and the first error in input order is named
    if (cp.first_seq >= 0) {
        int first = 0;
        while (first < n_seq && !pk.status[first]) first++;
        if (cp.first_seq < first) pk.first_err = cp.first_err;
        for (int s = 0; s < n_seq; s++)
            if (cp.status[s]) { pk.status[s] = cp.status[s]; pk.L[s] = 0; }
        pk.fold.erase(std::remove_if(pk.fold.begin(), pk.fold.end(), [&](int s) { return cp.status[s] != 0; }), pk.fold.end());
    }
    for (int s = 0; s < n_seq; s++) {
        seq_out[s] = rafft_cofold_seq{pk.status[s], pk.len[s], 0, 0, pk.status[s] ? 0 : cp.cut[s], 0};
        dot_row(db_out[s], pk.len[s]);
    }
    g_err = pk.first_err;
    if (pk.fold.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    std::vector<rafft_mfe_seq> mfe(n_seq);
    std::vector<int> inter(n_seq, 0);
    for (int s = 0; s < n_seq; s++) mfe[s] = rafft_mfe_seq{pk.status[s], pk.len[s], 0, 0};
    if (int rc = cofold_held(sc.st, pk, sc.d_codes, cp.cut, cofold_duplex_init(temp), lds_len, workspace_bytes, mfe.data(), inter.data(), db_out)) return rc;
    for (int s = 0; s < n_seq; s++) {
        if (pk.status[s]) continue;
        seq_out[s].dcal = mfe[s].dcal; seq_out[s].n_pairs = mfe[s].n_pairs; seq_out[s].n_inter = cp.cut[s] ? inter[s] : 0;
    }
    g_err = pk.first_err;
    return 0;
}

// ---- minimum-free-energy folds under a base-pair span

// The MFE folds of a pack under a base-pair span, under the caller's guard as mfe_held: seq_out[s].status is set, db_out may be
// null.  Chunks of whole sequences in input order whose banded tables fit the workspace budget (one sequence at least;
// mfe_span_layout): per chunk one launch per anti-diagonal of its widest band, then the exterior loop and the traceback, a
// wavefront a sequence each.  One synchronise at the end; its device buffers are freed on return.
int mfe_span_held(hipStream_t st, const SeqPack &pk, const uint8_t *d_codes, int max_span, long long workspace_bytes, rafft_mfe_seq *seq_out,
                  char *const *db_out)
{
    const MfeSpanLayout y = mfe_span_layout(pk, max_span, workspace_budget(workspace_bytes));
    const std::vector<MfeSpanSeq> &qs = y.qs;
    DevScratch mem;
    MfeSpanSeq *d_qs; uint32_t *d_stack; char *d_db; int4 *d_rec; int *d_order, *d_f, *d_ws;
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(MfeSpanSeq))) return rc;
    if (int rc = mem.alloc(d_f, y.n_f * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_stack, y.n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_db, y.n_db + 16)) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(int4))) return rc;
    if (int rc = mem.alloc(d_order, pk.fold.size() * 4)) return rc;
    if (int rc = mem.alloc(d_ws, y.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(MfeSpanSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, pk.fold.data(), pk.fold.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(int4), st));
    HIPCHK(hipFuncSetAttribute((const void *)mfe_span_exterior_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, mfe_span_lds_bytes(RAFFT_MFE_SPAN_MAX_LEN)));
    HIPCHK(hipFuncSetAttribute((const void *)mfe_span_traceback_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, mfe_span_lds_bytes(RAFFT_MFE_SPAN_MAX_LEN)));
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        const ChunkView v = chunk_view(c, d_order, pk.fold, pk);
        const int Wmax = chunk_wmax(c, pk.fold, qs);
        for (int d = 0; d < Wmax; d++) {
            const unsigned nx = (unsigned)std::min((v.Lmax - d + MFE_SPAN_NT / 64 - 1) / (MFE_SPAN_NT / 64), 2048);
            hipLaunchKernelGGL(mfe_span_diag_kernel, dim3(nx, v.ny), dim3(MFE_SPAN_NT), 0, st, g.T, d_qs, v.ord, d_codes, d_ws, d);
        }
        HIPCHK(hipGetLastError());
        const size_t lds = (size_t)mfe_span_lds_bytes(v.Lmax);
        hipLaunchKernelGGL(mfe_span_exterior_kernel, dim3(v.ny), dim3(64), lds, st, d_qs, v.ord, d_ws, d_f);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mfe_span_traceback_kernel, dim3(v.ny), dim3(64), lds, st, g.T, d_qs, v.ord, d_codes, d_ws, d_f, d_stack, d_db, d_rec);
        HIPCHK(hipGetLastError());
    }
    return mfe_results(st, qs, d_rec, d_db, y.n_db, seq_out, db_out);
}

// rafft_mfe_span_batch (arguments validated by the entry point)
int mfe_span_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int max_span, long long workspace_bytes, rafft_mfe_seq *seq_out,
                   char *const *db_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_SPAN_MAX_LEN, "RAFFT_MFE_SPAN_MAX_LEN");
    for (int s = 0; s < n_seq; s++) {
        seq_out[s] = rafft_mfe_seq{pk.status[s], pk.len[s], 0, 0};
        dot_row(db_out[s], pk.len[s]);
    }
    g_err = pk.first_err;
    if (pk.fold.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    if (int rc = mfe_span_held(sc.st, pk, sc.d_codes, max_span, workspace_bytes, seq_out, db_out)) return rc;
    g_err = pk.first_err;
    return 0;
}

// ---- partition function and pair probabilities

// The front rafft_pf_batch and rafft_sample_batch share, under the caller's SeqCall: the MFE of every sequence (mfe_held: its energy
// gives the scale; its device buffers are freed before the tables here are allocated), the scales and their powers, and the plan of
// chunks of whole sequences in input order whose `n_tabs` L x L fp64 tables - and, with cost2, a second cost per sequence - fit the
// workspace budget (one sequence at least; pf_layout).  Then, per chunk, pf_front_inside: one launch per anti-diagonal upwards and
// the exterior sums.  The buffers live in the caller's DevScratch.
struct PfFront {
    PfTemp t;
    std::vector<rafft_mfe_seq> mfe;
    std::vector<PfSeq> qs;
    ChunkPlan plan;
    unsigned long long n_db = 0;
    const uint8_t *d_codes; PfSeq *d_qs; double *d_aux, *d_ws; char *d_db; PfRec *d_rec; int *d_order;
    const unsigned long long *d_con_off = nullptr; const int *d_packs = nullptr;    // under constraints: the packs, for the pf_con_* kernels
};

// what pf_front does once f.mfe is there
int pf_front_tables(const SeqCall &sc, DevScratch &mem, const SeqPack &pk, double temp, double scale_factor, long long workspace_bytes, int n_tabs,
                    const size_t *cost2, PfFront &f)
{
    const int n_seq = (int)pk.L.size();
    const std::vector<int> &order = pk.fold;
    hipStream_t st = sc.st;
    f.t = pf_temp(temp);
    PfLayout y = pf_layout(pk, n_tabs, cost2, workspace_budget(workspace_bytes));
    for (int s = 0; s < n_seq; s++) pf_set_scale(y.qs[s], f.mfe[s].dcal, f.t.kt, scale_factor);
    f.qs = std::move(y.qs); f.plan = std::move(y.plan); f.n_db = y.n_db;
    const std::vector<PfSeq> &qs = f.qs;
    if (int rc = mem.alloc(f.d_qs, qs.size() * sizeof(PfSeq))) return rc;
    if (int rc = mem.alloc(f.d_aux, y.n_aux * sizeof(double) + 16)) return rc;
    if (int rc = mem.alloc(f.d_db, y.n_db + 16)) return rc;
    if (int rc = mem.alloc(f.d_rec, qs.size() * sizeof(PfRec))) return rc;
    if (int rc = mem.alloc(f.d_order, order.size() * 4)) return rc;
    if (int rc = mem.alloc(f.d_ws, f.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(f.d_qs, qs.data(), qs.size() * sizeof(PfSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(f.d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(f.d_rec, 0, qs.size() * sizeof(PfRec), st));
    hipLaunchKernelGGL(pf_powers_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, st, g.T, f.d_qs, n_seq, f.d_aux, f.t.beta);
    HIPCHK(hipGetLastError());
    return 0;
}

int pf_front(const SeqCall &sc, DevScratch &mem, const SeqPack &pk, double temp, double scale_factor, long long workspace_bytes, int n_tabs,
             const size_t *cost2, PfFront &f)
{
    const int n_seq = (int)pk.L.size();
    f.d_codes = sc.d_codes;
    f.mfe.resize(n_seq);
    for (int s = 0; s < n_seq; s++) f.mfe[s] = rafft_mfe_seq{pk.status[s], pk.len[s], 0, 0};
    if (int rc = mfe_held(sc.st, pk, f.d_codes, RAFFT_MFE_LDS_LEN, workspace_bytes, f.mfe.data(), nullptr)) return rc;
    return pf_front_tables(sc, mem, pk, temp, scale_factor, workspace_bytes, n_tabs, cost2, f);
}

// The front under constraints: mfe_con_held in place of mfe_held - the constrained objective gives the
// scale -, the packs of `cp` on the device for the chunks, and a sequence without a structure taken out of the pack before the
// layout: status RAFFT_ERR_INFEASIBLE, no tables, not in pk.fold.  pf_front_inside and pf_outside_probs then launch the pf_con_*
// kernels.
int pf_front(const SeqCall &sc, DevScratch &mem, SeqPack &pk, const ConstraintPack &cp, double temp, double scale_factor, long long workspace_bytes,
             int n_tabs, const size_t *cost2, PfFront &f)
{
    const int n_seq = (int)pk.L.size();
    hipStream_t st = sc.st;
    f.d_codes = sc.d_codes;
    f.mfe.resize(n_seq);
    for (int s = 0; s < n_seq; s++) f.mfe[s] = rafft_mfe_seq{pk.status[s], pk.len[s], 0, 0};
    std::vector<int> soft(n_seq, 0);
    if (int rc = mfe_con_held(st, pk, f.d_codes, cp, RAFFT_MFE_LDS_LEN, workspace_bytes, f.mfe.data(), soft.data(), nullptr)) return rc;
    int first = 0;
    while (first < n_seq && !pk.status[first]) first++;
    for (int s = 0; s < n_seq; s++) {
        if (pk.status[s] || f.mfe[s].dcal < MFE_INFH) continue;
        pk.status[s] = RAFFT_ERR_INFEASIBLE; pk.L[s] = 0;
        f.mfe[s].dcal = 0;
        if (s < first) { first = s; pk.first_err = "sequence " + std::to_string(s) + ": no structure satisfies its constraints"; }
    }
    pk.fold.erase(std::remove_if(pk.fold.begin(), pk.fold.end(), [&](int s) { return pk.status[s] != 0; }), pk.fold.end());
    int *d_packs; unsigned long long *d_off;
    if (int rc = mem.alloc(d_packs, cp.data.size() * 4)) return rc;
    if (int rc = mem.alloc(d_off, cp.off.size() * 8)) return rc;
    HIPCHK(hipMemcpyAsync(d_packs, cp.data.data(), cp.data.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off, cp.off.data(), cp.off.size() * 8, hipMemcpyHostToDevice, st));
    f.d_packs = d_packs; f.d_con_off = d_off;
    return pf_front_tables(sc, mem, pk, temp, scale_factor, workspace_bytes, n_tabs, cost2, f);
}

// launches per anti-diagonal of a chunk whose longest sequence has Lmax positions: four cells per workgroup
unsigned pf_diag_blocks(int Lmax, int d) { return (unsigned)std::min((Lmax - d + PF_NT / 64 - 1) / (PF_NT / 64), 1024); }

// the inside tables and the exterior sums of chunk v
int pf_front_inside(hipStream_t st, const PfFront &f, const ChunkView &v)
{
    for (int d = 0; d < v.Lmax; d++)
        if (f.d_packs)
            hipLaunchKernelGGL(pf_con_diag_kernel, dim3(pf_diag_blocks(v.Lmax, d), v.ny), dim3(PF_NT), 0, st, g.T, f.d_qs, v.ord, f.d_codes, f.d_con_off, f.d_packs, f.d_ws,
                               f.d_aux, f.t.beta, d);
        else
            hipLaunchKernelGGL(pf_diag_kernel, dim3(pf_diag_blocks(v.Lmax, d), v.ny), dim3(PF_NT), 0, st, g.T, f.d_qs, v.ord, f.d_codes, f.d_ws, f.d_aux, f.t.beta, d);
    HIPCHK(hipGetLastError());
    if (f.d_packs)
        hipLaunchKernelGGL(pf_con_exterior_kernel, dim3(v.ny), dim3(64), 0, st, g.T, f.d_qs, v.ord, f.d_codes, f.d_con_off, f.d_packs, f.d_ws, f.d_aux, f.t.beta, f.t.kt,
                           f.d_db, f.d_rec);
    else
        hipLaunchKernelGGL(pf_exterior_kernel, dim3(v.ny), dim3(64), 0, st, g.T, f.d_qs, v.ord, f.d_codes, f.d_ws, f.d_aux, f.t.beta, f.t.kt, f.d_db, f.d_rec);
    HIPCHK(hipGetLastError());
    return 0;
}

// What rafft_pf_batch and rafft_mea_batch do to chunk c (v: its view) of six tables a sequence after the inside pass: one launch
// per anti-diagonal downwards, the probabilities (table 3 then holds P, the d_db rows the centroids), and the copies of P the
// caller asked for.
int pf_outside_probs(hipStream_t st, const PfFront &f, const ChunkView &v, const ChunkPlan::Range &c, const std::vector<int> &order, double *const *prob_out)
{
    for (int d = v.Lmax - 1; d >= 4; d--)
        if (f.d_packs)
            hipLaunchKernelGGL(pf_con_out_diag_kernel, dim3(pf_diag_blocks(v.Lmax, d), v.ny), dim3(PF_NT), 0, st, g.T, f.d_qs, v.ord, f.d_codes, f.d_con_off, f.d_packs,
                               f.d_ws, f.d_aux, f.t.beta, d);
        else
            hipLaunchKernelGGL(pf_out_diag_kernel, dim3(pf_diag_blocks(v.Lmax, d), v.ny), dim3(PF_NT), 0, st, g.T, f.d_qs, v.ord, f.d_codes, f.d_ws, f.d_aux, f.t.beta, d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pf_prob_kernel, dim3(pf_diag_blocks(v.Lmax, 0), v.ny), dim3(PF_NT), 0, st, f.d_qs, v.ord, f.d_ws, f.d_aux, f.d_db, f.d_rec);
    HIPCHK(hipGetLastError());
    if (f.d_packs) {
        hipLaunchKernelGGL(pf_con_clamp_kernel, dim3(pf_diag_blocks(v.Lmax, 0), v.ny), dim3(PF_NT), 0, st, f.d_qs, v.ord, f.d_con_off, f.d_ws);
        HIPCHK(hipGetLastError());
    }
    if (prob_out)
        for (size_t k = c.a; k < c.b; k++) {
            const PfSeq &q = f.qs[order[k]];
            if (prob_out[order[k]])
                HIPCHK(hipMemcpyAsync(prob_out[order[k]], f.d_ws + q.tab_off + 3 * (size_t)q.L * q.L, (size_t)q.L * q.L * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    return 0;
}

// What pf_batch and pf_span_batch end with: the records and the n_db bytes of centroid rows come down, one synchronise.  A
// sequence whose tables left the fp64 range takes pf_left_range, and zero_numbers(s) zeroes what the caller was given for its
// numbers; every other one without an error gets n_pairs, energy, mfe_frequency and its row.  Sets the call's error text.
template <class Seq, class Zero>
int pf_results(hipStream_t st, const SeqPack &pk, const std::vector<Seq> &qs, const PfRec *d_rec, const char *d_db, unsigned long long n_db,
               rafft_pf_seq *seq_out, char *const *db_out, Zero zero_numbers)
{
    const int n_seq = (int)qs.size();
    std::vector<PfRec> rec(n_seq);
    std::vector<char> db(n_db + 16);
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, qs.size() * sizeof(PfRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(db.data(), d_db, n_db, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::string err = pk.first_err;
    for (int s = 0; s < n_seq; s++) {
        if (seq_out[s].status) continue;
        if (rec[s].status || rec[s].bad) {
            pf_left_range(s, seq_out[s].status, err, nullptr, 0);
            zero_numbers(s);
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

// rafft_pf_batch (arguments validated by the entry point).  One pack, one guard, one upload of the bases.  The shared front, then
// per chunk of six tables a sequence: the inside pass, one launch per anti-diagonal downwards, the probabilities.  One synchronise at
// the end.
int pf_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, long long workspace_bytes, rafft_pf_seq *seq_out,
             char *const *db_out, double *const *prob_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);     // (RAFFT_PF_MAX_LEN is RAFFT_MFE_MAX_LEN)
    for (int s = 0; s < n_seq; s++) {
        const int len = pk.len[s];
        seq_out[s] = rafft_pf_seq{pk.status[s], len, 0, 0, 0.0, 0.0};
        dot_row(db_out[s], len);
        if (prob_out && prob_out[s]) memset(prob_out[s], 0, (size_t)len * len * sizeof(double));
    }
    g_err = pk.first_err;
    const std::vector<int> &order = pk.fold;
    if (order.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    PfFront f;
    if (int rc = pf_front(sc, mem, pk, temp, scale_factor, workspace_bytes, 6, nullptr, f)) return rc;
    const std::vector<PfSeq> &qs = f.qs;
    for (int s = 0; s < n_seq; s++) seq_out[s].mfe_dcal = f.mfe[s].dcal;
    for (const ChunkPlan::Range &c : f.plan.chunks) {
        const ChunkView v = chunk_view(c, f.d_order, order, pk);
        if (int rc = pf_front_inside(st, f, v)) return rc;
        if (int rc = pf_outside_probs(st, f, v, c, order, prob_out)) return rc;
    }
    return pf_results(st, pk, qs, f.d_rec, f.d_db, f.n_db, seq_out, db_out, [&](int s) {
        if (prob_out && prob_out[s]) memset(prob_out[s], 0, (size_t)qs[s].L * qs[s].L * sizeof(double));
    });
}

// ---- partition function and pair probabilities under constraints and soft terms

// rafft_pf_constrained_batch (arguments validated by the entry point).  pf_batch's steps with the constrained front; an error of a
// sequence's constraints is an error of the sequence, as in mfe_con_batch.  Per chunk, after the probabilities, the unpaired
// probabilities of the sequences whose caller asked for them.
int pf_con_batch(int n_seq, const char *const *seqs, const int *lens, double temp, const char *const *constraints, const int32_t *const *soft_unpaired,
                 const int32_t *const *soft_stack, double scale_factor, long long workspace_bytes, rafft_pf_seq *seq_out, char *const *db_out,
                 double *const *prob_out, double *const *unpaired_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);
    const ConstraintPack cp = constraint_pack(n_seq, pk.L.data(), pk.codes.data(), pk.code_off.data(), constraints, soft_unpaired, soft_stack);
    if (cp.param_seq >= 0) return fail(RAFFT_ERR_PARAM, cp.first_err);
    if (cp.first_seq >= 0) {
        int first = 0;
        while (first < n_seq && !pk.status[first]) first++;
        if (cp.first_seq < first) pk.first_err = cp.first_err;
        for (int s = 0; s < n_seq; s++)
            if (cp.status[s]) { pk.status[s] = cp.status[s]; pk.L[s] = 0; }
        pk.fold.erase(std::remove_if(pk.fold.begin(), pk.fold.end(), [&](int s) { return cp.status[s] != 0; }), pk.fold.end());
    }
    auto zero_numbers = [&](int s) {
        const size_t len = (size_t)pk.len[s];
        if (prob_out && prob_out[s]) memset(prob_out[s], 0, len * len * sizeof(double));
        if (unpaired_out && unpaired_out[s]) memset(unpaired_out[s], 0, len * sizeof(double));
    };
    for (int s = 0; s < n_seq; s++) {
        seq_out[s] = rafft_pf_seq{pk.status[s], pk.len[s], 0, 0, 0.0, 0.0};
        dot_row(db_out[s], pk.len[s]);
        zero_numbers(s);
    }
    g_err = pk.first_err;
    if (pk.fold.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    PfFront f;
    if (int rc = pf_front(sc, mem, pk, cp, temp, scale_factor, workspace_bytes, 6, nullptr, f)) return rc;
    const std::vector<int> &order = pk.fold;        // without the infeasible sequences now
    const std::vector<PfSeq> &qs = f.qs;
    for (int s = 0; s < n_seq; s++) { seq_out[s].status = pk.status[s]; seq_out[s].mfe_dcal = f.mfe[s].dcal; }
    g_err = pk.first_err;
    if (order.empty()) return 0;
    for (const ChunkPlan::Range &c : f.plan.chunks) {
        const ChunkView v = chunk_view(c, f.d_order, order, pk);
        if (int rc = pf_front_inside(st, f, v)) return rc;
        if (int rc = pf_outside_probs(st, f, v, c, order, prob_out)) return rc;
        if (!unpaired_out) continue;
        hipLaunchKernelGGL(pf_unpaired_kernel, dim3(pf_diag_blocks(v.Lmax, 0), v.ny), dim3(PF_NT), 0, st, f.d_qs, v.ord, f.d_ws, f.d_aux);
        HIPCHK(hipGetLastError());
        for (size_t k = c.a; k < c.b; k++) {
            const PfSeq &q = qs[order[k]];
            if (unpaired_out[order[k]]) HIPCHK(hipMemcpyAsync(unpaired_out[order[k]], f.d_aux + q.aux_off, (size_t)q.L * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    return pf_results(st, pk, qs, f.d_rec, f.d_db, f.n_db, seq_out, db_out, zero_numbers);
}

// ---- partition function and pair probabilities under a base-pair span

// rafft_pf_span_batch (arguments validated by the entry point).  One pack, one guard, one upload of the bases.  The span MFE of
// every sequence first (mfe_span_held: its energies give the scales and the mfe_dcal of the records; its device buffers are freed
// before the tables here are allocated).  Then chunks of whole sequences in input order whose banded tables fit the workspace
// budget (one sequence at least; pf_span_layout); per chunk one launch per anti-diagonal of its widest band upwards, the exterior
// sums, one launch per anti-diagonal downwards, the probabilities, and the copies of P and of unpaired the caller asked for.  One
// synchronise at the end.
int pf_span_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, int max_span, long long workspace_bytes,
                  rafft_pf_seq *seq_out, char *const *db_out, double *const *prob_out, double *const *unpaired_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_SPAN_MAX_LEN, "RAFFT_MFE_SPAN_MAX_LEN");
    for (int s = 0; s < n_seq; s++) {
        const int len = pk.len[s];
        seq_out[s] = rafft_pf_seq{pk.status[s], len, 0, 0, 0.0, 0.0};
        dot_row(db_out[s], len);
        if (pk.status[s] == RAFFT_ERR_TOO_LONG) continue;               // (no buffer is asked for beyond the limit)
        if (prob_out && prob_out[s]) memset(prob_out[s], 0, (size_t)len * mfe_span_width(len, max_span) * sizeof(double));
        if (unpaired_out && unpaired_out[s]) memset(unpaired_out[s], 0, (size_t)len * sizeof(double));
    }
    g_err = pk.first_err;
    const std::vector<int> &order = pk.fold;
    if (order.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    std::vector<rafft_mfe_seq> mfe(n_seq);
    for (int s = 0; s < n_seq; s++) mfe[s] = rafft_mfe_seq{pk.status[s], pk.len[s], 0, 0};
    if (int rc = mfe_span_held(st, pk, sc.d_codes, max_span, workspace_bytes, mfe.data(), nullptr)) return rc;
    const auto [kt, beta] = pf_temp(temp);
    PfSpanLayout y = pf_span_layout(pk, max_span, workspace_budget(workspace_bytes));
    for (int s = 0; s < n_seq; s++) {
        pf_set_scale(y.qs[s], mfe[s].dcal, kt, scale_factor);
        seq_out[s].mfe_dcal = mfe[s].dcal;
    }
    const std::vector<PfSpanSeq> &qs = y.qs;
    PfSpanSeq *d_qs; double *d_aux, *d_ws; int *d_exp, *d_order; char *d_db; PfRec *d_rec;
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(PfSpanSeq))) return rc;
    if (int rc = mem.alloc(d_aux, y.n_aux * sizeof(double) + 16)) return rc;
    if (int rc = mem.alloc(d_exp, y.n_exp * sizeof(int) + 16)) return rc;
    if (int rc = mem.alloc(d_db, y.n_db + 16)) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(PfRec))) return rc;
    if (int rc = mem.alloc(d_order, order.size() * 4)) return rc;
    if (int rc = mem.alloc(d_ws, y.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(PfSpanSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(PfRec), st));
    hipLaunchKernelGGL(pf_span_powers_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, st, g.T, d_qs, n_seq, d_aux, beta);
    HIPCHK(hipGetLastError());
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        const ChunkView v = chunk_view(c, d_order, order, pk);
        const int Wmax = chunk_wmax(c, order, qs);
        for (int d = 0; d < Wmax; d++)
            hipLaunchKernelGGL(pf_span_diag_kernel, dim3(pf_diag_blocks(v.Lmax, d), v.ny), dim3(PF_NT), 0, st, g.T, d_qs, v.ord, sc.d_codes, d_ws, d_aux, beta, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pf_span_exterior_kernel, dim3(v.ny), dim3(64), 0, st, d_qs, v.ord, d_ws, d_aux, d_exp, kt, d_db, d_rec);
        HIPCHK(hipGetLastError());
        for (int d = Wmax - 1; d >= 4; d--)
            hipLaunchKernelGGL(pf_span_out_diag_kernel, dim3(pf_diag_blocks(v.Lmax, d), v.ny), dim3(PF_NT), 0, st, g.T, d_qs, v.ord, sc.d_codes, d_ws, d_aux, d_exp, beta, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pf_span_prob_kernel, dim3(pf_diag_blocks(v.Lmax, 0), v.ny), dim3(PF_NT), 0, st, d_qs, v.ord, d_ws, d_aux, d_exp, d_db, d_rec);
        HIPCHK(hipGetLastError());
        for (size_t k = c.a; k < c.b; k++) {
            const int s = order[k];
            const PfSpanSeq &q = qs[s];
            const size_t n = (size_t)pf_span_table_doubles(q.L, q.W);
            if (prob_out && prob_out[s]) HIPCHK(hipMemcpyAsync(prob_out[s], d_ws + q.tab_off + 4 * n, n * sizeof(double), hipMemcpyDeviceToHost, st));
            if (unpaired_out && unpaired_out[s])
                HIPCHK(hipMemcpyAsync(unpaired_out[s], d_aux + q.aux_off + 2 * ((size_t)q.W + 2) + 2 * ((size_t)q.L + 1), (size_t)q.L * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    return pf_results(st, pk, qs, d_rec, d_db, y.n_db, seq_out, db_out, [&](int s) {
        if (prob_out && prob_out[s]) memset(prob_out[s], 0, (size_t)pf_span_table_doubles(qs[s].L, qs[s].W) * sizeof(double));
        if (unpaired_out && unpaired_out[s]) memset(unpaired_out[s], 0, (size_t)qs[s].L * sizeof(double));
    });
}

// ---- maximum-expected-accuracy structures

static_assert(MEA_NT == PF_NT, "pf_diag_blocks counts the workgroups of mea_diag_kernel too");

// The recursion on the P tables of chunk v: q, WT and the diversity's shares, one launch per anti-diagonal upwards, the traceback.
int mea_chunk(hipStream_t st, const MeaSeq *d_mq, const ChunkView &v, double *d_ws, double *d_aux, double gamma, uint32_t *d_stack, int16_t *d_pt, char *d_db,
              MeaRec *d_rec)
{
    const int nt = (v.Lmax + MEA_TILE - 1) / MEA_TILE;
    hipLaunchKernelGGL(mea_prepare_kernel, dim3((unsigned)std::min(nt * nt, 1024), v.ny), dim3(MEA_NT), 0, st, d_mq, v.ord, d_ws, d_aux, gamma);
    HIPCHK(hipGetLastError());
    for (int d = 0; d < v.Lmax; d++)
        hipLaunchKernelGGL(mea_diag_kernel, dim3(pf_diag_blocks(v.Lmax, d), v.ny), dim3(MEA_NT), 0, st, d_mq, v.ord, d_ws, d_aux, d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mea_traceback_kernel, dim3(v.ny), dim3(64), 0, st, d_mq, v.ord, d_ws, d_aux, d_stack, d_pt, d_db, d_rec);
    HIPCHK(hipGetLastError());
    return 0;
}

int mea_bad(int s, int bad)
{
    return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + (bad == MEA_BAD_STACK ? ": the stack of pending intervals is full" : ": the traceback found no candidate for a cell"));
}

// rafft_mea_batch (arguments validated by the entry point; gamma > 0).  rafft_pf_batch's call - the shared front, per chunk the
// inside pass, the outside pass and the probabilities - and then, per chunk, mea_chunk on table 3 with WT, E and ET in the dead
// tables 0, 1, 2 (mea_layout), and one eval_kernel launch on the pair tables the traceback left.  One synchronise at the end.
// Its tail is its own: it fills rafft_mea_seq from three record arrays, where pf_results fills rafft_pf_seq from one.
int mea_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, long long workspace_bytes, double gamma,
              rafft_mea_seq *seq_out, char *const *db_out, double *const *prob_out, double *const *unpaired_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);
    for (int s = 0; s < n_seq; s++) {
        const int len = pk.len[s];
        seq_out[s] = rafft_mea_seq{pk.status[s], len, 0, 0, 0, 0, 0.0, 0.0, 0.0};
        dot_row(db_out[s], len);
        if (prob_out && prob_out[s]) memset(prob_out[s], 0, (size_t)len * len * sizeof(double));
        if (unpaired_out && unpaired_out[s]) memset(unpaired_out[s], 0, (size_t)len * sizeof(double));
    }
    g_err = pk.first_err;
    const std::vector<int> &order = pk.fold;
    if (order.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    PfFront f;
    if (int rc = pf_front(sc, mem, pk, temp, scale_factor, workspace_bytes, 6, nullptr, f)) return rc;
    const std::vector<PfSeq> &qs = f.qs;
    for (int s = 0; s < n_seq; s++) seq_out[s].mfe_dcal = f.mfe[s].dcal;
    const MeaLayout y = mea_layout(qs);
    const size_t n_run = order.size();
    std::vector<long long> e_off(n_run);
    std::vector<int> e_len(n_run);
    for (size_t k = 0; k < n_run; k++) { e_off[k] = (long long)qs[order[k]].code_off; e_len[k] = qs[order[k]].L; }
    MeaSeq *d_mq; MeaRec *d_mrec; uint32_t *d_stack; int16_t *d_pt; long long *d_eoff; int *d_elen, *d_eout, *d_est;
    if (int rc = mem.alloc(d_mq, y.qs.size() * sizeof(MeaSeq))) return rc;
    if (int rc = mem.alloc(d_mrec, y.qs.size() * sizeof(MeaRec))) return rc;
    if (int rc = mem.alloc(d_stack, y.n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_pt, pk.codes.size() * 2)) return rc;
    if (int rc = mem.alloc(d_eoff, n_run * 8)) return rc;
    if (int rc = mem.alloc(d_elen, n_run * 4)) return rc;
    if (int rc = mem.alloc(d_eout, n_run * 4)) return rc;
    if (int rc = mem.alloc(d_est, n_run * 4)) return rc;
    HIPCHK(hipMemcpyAsync(d_mq, y.qs.data(), y.qs.size() * sizeof(MeaSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_eoff, e_off.data(), n_run * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_elen, e_len.data(), n_run * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_mrec, 0, y.qs.size() * sizeof(MeaRec), st));
    for (const ChunkPlan::Range &c : f.plan.chunks) {
        const ChunkView v = chunk_view(c, f.d_order, order, pk);
        if (int rc = pf_front_inside(st, f, v)) return rc;
        if (int rc = pf_outside_probs(st, f, v, c, order, prob_out)) return rc;
        if (int rc = mea_chunk(st, d_mq, v, f.d_ws, f.d_aux, gamma, d_stack, d_pt, f.d_db, d_mrec)) return rc;
        hipLaunchKernelGGL(eval_kernel, dim3(v.ny), dim3(64), 0, st, g.T, (int)v.ny, f.d_codes, d_pt, d_eoff + c.a, d_elen + c.a, d_eout + c.a, d_est + c.a, (int *)nullptr);
        HIPCHK(hipGetLastError());
        if (unpaired_out)
            for (size_t k = c.a; k < c.b; k++) {
                const PfSeq &q = qs[order[k]];
                if (unpaired_out[order[k]]) HIPCHK(hipMemcpyAsync(unpaired_out[order[k]], f.d_aux + q.aux_off, (size_t)q.L * sizeof(double), hipMemcpyDeviceToHost, st));
            }
    }
    std::vector<PfRec> rec(n_seq);
    std::vector<MeaRec> mrec(n_seq);
    std::vector<int> e_out(n_run), e_st(n_run), run_of(n_seq, -1);
    std::vector<char> db(f.n_db + 16);
    HIPCHK(hipMemcpyAsync(rec.data(), f.d_rec, qs.size() * sizeof(PfRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(mrec.data(), d_mrec, qs.size() * sizeof(MeaRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(e_out.data(), d_eout, n_run * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(e_st.data(), d_est, n_run * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(db.data(), f.d_db, f.n_db, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < n_run; k++) run_of[order[k]] = (int)k;
    std::string err = pk.first_err;
    for (int s = 0; s < n_seq; s++) {
        if (seq_out[s].status) continue;
        const size_t L = (size_t)qs[s].L;
        if (rec[s].status || rec[s].bad) {
            pf_left_range(s, seq_out[s].status, err, prob_out ? prob_out[s] : nullptr, L * L * sizeof(double));
            if (unpaired_out && unpaired_out[s]) memset(unpaired_out[s], 0, L * sizeof(double));
            continue;
        }
        if (mrec[s].bad) return mea_bad(s, mrec[s].bad);
        if (e_st[run_of[s]]) return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + ": the row holds a pair the energy model refuses");
        seq_out[s].n_pairs = mrec[s].n_pairs;
        seq_out[s].dcal = e_out[run_of[s]];
        seq_out[s].energy = rec[s].energy;
        seq_out[s].mea = mrec[s].mea;
        seq_out[s].diversity = mrec[s].diversity;
        memcpy(db_out[s], db.data() + qs[s].db_off, L + 1);
    }
    g_err = err;
    return 0;
}

// rafft_mea_probs_batch (arguments validated by the entry point; gamma > 0).  Every matrix is checked before the device is touched;
// then chunks of four tables a matrix (mea_probs_layout): the upload of P, mea_chunk, the download of q.  One synchronise at the end.
int mea_probs_batch(int n, const int *lens, const double *const *prob_in, double gamma, long long workspace_bytes, rafft_mea_probs_seq *seq_out,
                    char *const *db_out, double *const *unpaired_out)
{
    if (n == 0) return 0;
    const MeaProbsLayout y = mea_probs_layout(n, lens, workspace_budget(workspace_bytes));
    for (int s : y.order) {
        int bi = 0, bj = 0;
        const char *why = nullptr;
        if (mea_probs_bad_entry(prob_in[s], y.L[s], bi, bj, why))
            return fail(RAFFT_ERR_PARAM, "sequence " + std::to_string(s) + ": P(" + std::to_string(bi) + "," + std::to_string(bj) + ") " + why);
    }
    for (int s = 0; s < n; s++) {
        seq_out[s] = rafft_mea_probs_seq{y.status[s], y.len[s], 0, 0, 0.0, 0.0};
        dot_row(db_out[s], y.len[s]);
        if (unpaired_out && unpaired_out[s]) memset(unpaired_out[s], 0, (size_t)y.len[s] * sizeof(double));
    }
    g_err = y.first_err;
    const std::vector<int> &order = y.order;
    if (order.empty()) return 0;
    SeamGuard sg;
    if (int rc = sg.enter()) return rc;
    hipStream_t st = sg.stream;
    DevScratch mem;
    MeaSeq *d_mq; MeaRec *d_mrec; uint32_t *d_stack; int16_t *d_pt; int *d_order; double *d_ws, *d_aux; char *d_db;
    if (int rc = mem.alloc(d_mq, y.qs.size() * sizeof(MeaSeq))) return rc;
    if (int rc = mem.alloc(d_mrec, y.qs.size() * sizeof(MeaRec))) return rc;
    if (int rc = mem.alloc(d_stack, y.n_stack * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_pt, y.n_pt * 2 + 16)) return rc;
    if (int rc = mem.alloc(d_order, order.size() * 4)) return rc;
    if (int rc = mem.alloc(d_aux, y.n_aux * sizeof(double) + 16)) return rc;
    if (int rc = mem.alloc(d_db, y.n_db + 16)) return rc;
    if (int rc = mem.alloc(d_ws, y.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_mq, y.qs.data(), y.qs.size() * sizeof(MeaSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_mrec, 0, y.qs.size() * sizeof(MeaRec), st));
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        const ChunkView v{d_order + c.a, (unsigned)(c.b - c.a), chunk_lmax(c, order, y.L)};
        for (size_t k = c.a; k < c.b; k++) {
            const MeaSeq &q = y.qs[order[k]];
            HIPCHK(hipMemcpyAsync(d_ws + q.p_off, prob_in[order[k]], (size_t)q.L * q.L * sizeof(double), hipMemcpyHostToDevice, st));
        }
        if (int rc = mea_chunk(st, d_mq, v, d_ws, d_aux, gamma, d_stack, d_pt, d_db, d_mrec)) return rc;
    }
    std::vector<MeaRec> mrec(n);
    std::vector<char> db(y.n_db + 16);
    if (unpaired_out)
        for (int s : order)
            if (unpaired_out[s]) HIPCHK(hipMemcpyAsync(unpaired_out[s], d_aux + y.qs[s].aux_off, (size_t)y.L[s] * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(mrec.data(), d_mrec, y.qs.size() * sizeof(MeaRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(db.data(), d_db, y.n_db, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s : order) {
        if (mrec[s].bad) return mea_bad(s, mrec[s].bad);
        seq_out[s].n_pairs = mrec[s].n_pairs;
        seq_out[s].mea = mrec[s].mea;
        seq_out[s].diversity = mrec[s].diversity;
        memcpy(db_out[s], db.data() + y.qs[s].db_off, (size_t)y.L[s] + 1);
    }
    g_err = y.first_err;
    return 0;
}

// ---- structures drawn from the ensemble

// rafft_sample_batch (arguments validated by the entry point).  The shared front with three tables a sequence - the inside tables
// are all a stochastic traceback reads - and the rows of a chunk (n_samples (L + 1) bytes a sequence) as the planner's second cost
// (sample_layout).  Per chunk: the inside pass, sample_kernel over (groups of four samples, sequences), one synchronise, the rows and
// energies of the sequences that passed the range check straight into the caller's buffers.
int sample_batch(int n_seq, const char *const *seqs, const int *lens, double temp, double scale_factor, long long workspace_bytes, int n_samples,
                 const unsigned long long *seeds, rafft_sample_seq *seq_out, char *const *db_out, int *const *dcal_out)
{
    if (int rc = check_temp(temp)) return rc;
    if (n_seq == 0) return 0;
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);
    auto dot_rows = [&](int s) { for (int k = 0; k < n_samples; k++) dot_row(db_out[s] + (size_t)k * ((size_t)pk.len[s] + 1), pk.len[s]); };
    for (int s = 0; s < n_seq; s++) {
        seq_out[s] = rafft_sample_seq{pk.status[s], pk.len[s], 0, 0, 0.0};
        if (!pk.status[s]) continue;
        dot_rows(s);
        if (dcal_out && dcal_out[s]) memset(dcal_out[s], 0, (size_t)n_samples * sizeof(int));
    }
    g_err = pk.first_err;
    const std::vector<int> &order = pk.fold;
    if (order.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    PfFront f;
    const std::vector<size_t> row_costs = sample_row_costs(pk, n_samples);
    if (int rc = pf_front(sc, mem, pk, temp, scale_factor, workspace_bytes, 3, row_costs.data(), f)) return rc;
    const std::vector<PfSeq> &qs = f.qs;
    const SampleLayout y = sample_layout(pk, f.plan, n_samples, seeds);
    SampleSeq *d_smp; char *d_rows; int *d_dcal, *d_bad;
    if (int rc = mem.alloc(d_smp, y.smp.size() * sizeof(SampleSeq))) return rc;
    if (int rc = mem.alloc(d_rows, f.plan.max_cost2 + 16)) return rc;
    if (int rc = mem.alloc(d_dcal, y.max_seqs * (size_t)n_samples * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_bad, (size_t)n_seq * 4)) return rc;
    HIPCHK(hipMemcpyAsync(d_smp, y.smp.data(), y.smp.size() * sizeof(SampleSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_bad, 0, (size_t)n_seq * 4, st));
    std::vector<PfRec> rec(n_seq);
    std::vector<int> bad(n_seq);
    std::string err = pk.first_err;
    for (const ChunkPlan::Range &c : f.plan.chunks) {
        const ChunkView v = chunk_view(c, f.d_order, order, pk);
        if (int rc = pf_front_inside(st, f, v)) return rc;
        if (n_samples > 0) {
            hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n_samples + SAMPLE_NT / 64 - 1) / (SAMPLE_NT / 64)), v.ny), dim3(SAMPLE_NT),
                               (size_t)sample_lds_bytes(v.Lmax), st, g.T, f.d_qs, v.ord, f.d_codes, f.d_ws, f.d_aux, f.t.beta, f.d_rec, d_smp, n_samples,
                               v.Lmax, d_rows, d_dcal, d_bad);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(rec.data(), f.d_rec, qs.size() * sizeof(PfRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(bad.data(), d_bad, (size_t)n_seq * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = c.a; k < c.b; k++) {
            const int s = order[k];
            seq_out[s].mfe_dcal = f.mfe[s].dcal;
            if (bad[s]) return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + (bad[s] == SAMPLE_BAD_STACK ? ": the sampling stack is full" : ": a sampled cell has no candidate"));
            if (rec[s].status) {
                dot_rows(s);
                pf_left_range(s, seq_out[s].status, err, dcal_out ? dcal_out[s] : nullptr, (size_t)n_samples * sizeof(int));
                continue;
            }
            seq_out[s].energy = rec[s].energy;
            seq_out[s].n_samples = n_samples;
            if (n_samples == 0) continue;
            HIPCHK(hipMemcpy(db_out[s], d_rows + y.smp[s].row_off, y.row_bytes[k], hipMemcpyDeviceToHost));
            if (dcal_out && dcal_out[s]) HIPCHK(hipMemcpy(dcal_out[s], d_dcal + y.smp[s].dcal_off, (size_t)n_samples * sizeof(int), hipMemcpyDeviceToHost));
        }
    }
    g_err = err;
    return 0;
}

// ---- every structure within an energy band

constexpr int SUBOPT_POLL_LEVELS = 8;       // levels between two reads of the chunk's "sequences that go on" word

// what a rafft_subopt_result points into; rafft_subopt_free deletes it
struct SuboptOwner {
    rafft_subopt_result res;
    std::vector<rafft_subopt_seq> seq;
    std::vector<std::vector<char>> db;
    std::vector<std::vector<int32_t>> dcal;
};

// of the last call: levels, kernel launches of the enumeration, launches of the table fill, chunks, sequences over their capacity,
// microseconds of the fill, microseconds of the enumeration with its copies (tools/subopt_measure.py)
long long g_subopt_counters[7];

// rafft_subopt_batch (arguments validated by the entry point).  One pack, one guard, one upload of the bases.  Chunks of whole
// sequences in input order: three L x L int32 tables a sequence as the primary cost, its two frontier buffers of max_structs states
// and its max_structs counts as the second.  Per chunk: the tables (mfe_fill_chunk), the exterior energies and the first state
// (subopt_init_kernel), then levels of count / scan / emit until the word read back every SUBOPT_POLL_LEVELS levels says that no
// sequence goes on; the finished states are packed on the device and copied.  Every offset is subopt_layout's.  The final order -
// a stable sort on dcal of rows that arrive in enumeration order - is an index permutation on the host, applied while the result is
// filled.
int subopt_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int delta, int max_structs, long long workspace_bytes,
                 rafft_subopt_result **out)
{
    *out = nullptr;
    if (int rc = check_temp(temp)) return rc;
    for (long long &c : g_subopt_counters) c = 0;
    std::unique_ptr<SuboptOwner> own(new SuboptOwner);
    own->seq.resize(n_seq); own->db.resize(n_seq); own->dcal.resize(n_seq);
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_MFE_MAX_LEN);
    int n_failed = 0;
    for (int s = 0; s < n_seq; s++) {
        own->db[s].assign(1, 0); own->dcal[s].assign(1, 0);
        own->seq[s] = rafft_subopt_seq{pk.status[s], pk.len[s], 0, 0, 0, own->db[s].data(), own->dcal[s].data()};
        n_failed += pk.status[s] != 0;
    }
    auto finish = [&](const std::string &err) {
        own->res = rafft_subopt_result{n_seq, n_failed, own->seq.data(), own.get()};
        *out = &own->res;
        own.release();
        g_err = err;
        return 0;
    };
    const std::vector<int> &order = pk.fold;
    if (order.empty()) return finish(pk.first_err);
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    const uint8_t *d_codes = sc.d_codes;
    const SuboptLayout y = subopt_layout(pk, max_structs, workspace_budget(workspace_bytes));
    const std::vector<SuboptSeq> &qs = y.qs;
    const ChunkPlan &plan = y.plan;
    MfeSeq *d_mq; SuboptSeq *d_qs; SuboptRec *d_rec; int *d_order, *d_ws, *d_f, *d_open; unsigned char *d_front;
    if (int rc = mem.alloc(d_mq, y.mq.size() * sizeof(MfeSeq))) return rc;
    if (int rc = mem.alloc(d_qs, qs.size() * sizeof(SuboptSeq))) return rc;
    if (int rc = mem.alloc(d_rec, qs.size() * sizeof(SuboptRec))) return rc;
    if (int rc = mem.alloc(d_order, order.size() * 4)) return rc;
    if (int rc = mem.alloc(d_f, y.n_f * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_open, 16)) return rc;
    if (int rc = mem.alloc(d_ws, plan.max_cost + 16)) return rc;
    if (int rc = mem.alloc(d_front, plan.max_cost2 + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_mq, y.mq.data(), y.mq.size() * sizeof(MfeSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_qs, qs.data(), qs.size() * sizeof(SuboptSeq), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, qs.size() * sizeof(SuboptRec), st));
    const unsigned nx = (unsigned)std::min((max_structs + SUBOPT_NT / 64 - 1) / (SUBOPT_NT / 64), 1024);
    std::vector<SuboptRec> rec(y.max_seqs);
    std::vector<char> rows;
    std::vector<int> dc, perm;
    std::string err = pk.first_err;
    using clk = std::chrono::steady_clock;
    auto us = [](clk::time_point a, clk::time_point b) { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
    g_subopt_counters[3] = (long long)plan.chunks.size();
    for (const ChunkPlan::Range &c : plan.chunks) {
        const ChunkView v = chunk_view(c, d_order, order, pk);
        const clk::time_point t0 = clk::now();
        if (int rc = mfe_fill_chunk(st, d_mq, v, d_codes, d_ws)) return rc;
        hipLaunchKernelGGL(subopt_init_kernel, dim3(v.ny), dim3(64), 0, st, g.T, d_qs, v.ord, d_codes, d_ws, d_f, d_front, d_rec);
        HIPCHK(hipGetLastError());
        int open = (int)v.ny;
        HIPCHK(hipMemcpyAsync(d_open, &open, 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        const clk::time_point t1 = clk::now();
        g_subopt_counters[2] += v.Lmax + 1;
        g_subopt_counters[5] += us(t0, t1);
        // a step fixes a pair, an unpaired base or a split: fewer than 3 L + 8 of them lead to any structure
        const int max_levels = 3 * v.Lmax + 8;
        int level = 0;
        while (open > 0) {
            if (level > max_levels) return fail(RAFFT_ERR_HIP, "internal: the enumeration did not end after " + std::to_string(level) + " levels");
            for (int r = 0; r < SUBOPT_POLL_LEVELS; r++, level++) {
                const int src = level & 1;
                hipLaunchKernelGGL(subopt_level_kernel<false>, dim3(nx, v.ny), dim3(SUBOPT_NT), 0, st, g.T, d_qs, v.ord, d_codes, d_ws, d_f, d_front, (int *)d_front, d_rec, src, delta);
                hipLaunchKernelGGL(subopt_scan_kernel, dim3(v.ny), dim3(SUBOPT_SCAN_NT), 0, st, d_qs, v.ord, (int *)d_front, d_rec, src, max_structs, d_open);
                hipLaunchKernelGGL(subopt_level_kernel<true>, dim3(nx, v.ny), dim3(SUBOPT_NT), 0, st, g.T, d_qs, v.ord, d_codes, d_ws, d_f, d_front, (int *)d_front, d_rec, src, delta);
            }
            HIPCHK(hipGetLastError());
            g_subopt_counters[1] += 3 * SUBOPT_POLL_LEVELS;
            HIPCHK(hipMemcpyAsync(&open, d_open, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        hipLaunchKernelGGL(subopt_pack_kernel, dim3(nx, v.ny), dim3(SUBOPT_NT), 0, st, d_qs, v.ord, d_front, d_rec);
        HIPCHK(hipGetLastError());
        g_subopt_counters[1] += 1;
        // (the records of a chunk's sequences are not contiguous in d_rec: one copy each)
        for (size_t k = c.a; k < c.b; k++) HIPCHK(hipMemcpyAsync(&rec[k - c.a], d_rec + order[k], sizeof(SuboptRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = c.a; k < c.b; k++) {
            const int s = order[k], L = pk.L[s];
            const SuboptRec &r = rec[k - c.a];
            rafft_subopt_seq &o = own->seq[s];
            o.mfe_dcal = r.mfe;
            g_subopt_counters[0] = std::max(g_subopt_counters[0], (long long)r.levels);
            if (r.state == SUBOPT_BROKEN || r.state == SUBOPT_ACTIVE)
                return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + (r.bad == SUBOPT_BAD_STACK ? ": the stack of pending segments is full"
                                           : r.bad == SUBOPT_BAD_CELL ? ": a kept state has no candidate within the band" : ": the enumeration stopped early"));
            if (r.state == SUBOPT_OVER) {
                o.status = RAFFT_ERR_CAPACITY;
                o.n_reached = r.n_reached;
                n_failed++;
                g_subopt_counters[4]++;
                if (err.empty())
                    err = "sequence " + std::to_string(s) + ": at least " + std::to_string(r.n_reached) + " structures within the band, max_structs is " + std::to_string(max_structs);
                continue;
            }
            const int n = r.n[r.final_buf];
            const size_t rb = (size_t)n * ((size_t)L + 1);
            rows.resize(rb); dc.resize(n); perm.resize(n);
            const unsigned char *src = d_front + qs[s].buf_off[r.final_buf ^ 1];
            HIPCHK(hipMemcpy(rows.data(), src, rb, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(dc.data(), src + subopt_pack_dcal_off(n, L), (size_t)n * 4, hipMemcpyDeviceToHost));
            for (int x = 0; x < n; x++) perm[x] = x;
            std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return dc[a] < dc[b]; });
            own->db[s].resize(rb); own->dcal[s].resize(n);
            for (int x = 0; x < n; x++) {
                memcpy(own->db[s].data() + (size_t)x * (L + 1), rows.data() + (size_t)perm[x] * (L + 1), (size_t)L + 1);
                own->dcal[s][x] = dc[perm[x]];
            }
            o.n_structs = n;
            o.db = own->db[s].data(); o.dcal = own->dcal[s].data();
        }
        g_subopt_counters[6] += us(t1, clk::now());
    }
    return finish(err);
}

// ---- folding barriers between structure pairs

// of the last call: chunks, levels over all chunks, kernel launches, problems that ran
long long g_findpath_counters[4];

// rafft_findpath_batch (arguments validated by the entry point).  One pack of the sequences; per problem without a sequence error
// the moves and conflict masks (findpath_moves), then the capacity check; the problems that are left are laid out in chunks
// (findpath_layout).  Per chunk: one upload of the inputs, findpath_init_kernel, per level of the chunk's largest d
// findpath_expand_kernel over (states, problems) and findpath_select_kernel over problems, findpath_trace_kernel, one download of the
// outputs and of the records, one synchronise.
int findpath_batch(int n_paths, const char *const *seqs, const int *lens, const char *const *starts, const char *const *ends, const int *widths,
                   double temp, long long workspace_bytes, rafft_findpath_rec *rec_out, int *const *moves_out, int *const *dcal_out)
{
    if (int rc = check_temp(temp)) return rc;
    for (long long &c : g_findpath_counters) c = 0;
    if (n_paths == 0) return 0;
    const SeqPack pk = pack_sequences(n_paths, seqs, lens, RAFFT_FINDPATH_MAX_LEN);
    std::string err = pk.first_err.empty() ? std::string() : "problem " + pk.first_err.substr(9);      // ("sequence N: ..." of the pack)
    std::vector<FpMoves> mv(n_paths);
    std::vector<int> run, d(n_paths, 0), n_rem(n_paths, 0);
    for (int p = 0; p < n_paths; p++) {
        rec_out[p] = rafft_findpath_rec{pk.status[p], 0, 0, 0, 0, 0, 0, 0};
        if (pk.status[p]) continue;
        const std::string who = "problem " + std::to_string(p);
        if (int st = findpath_moves(pk.codes.data() + pk.code_off[p], pk.L[p], starts[p], ends[p], mv[p])) {
            rec_out[p].status = st;
            if (err.empty()) err = who + ": a row is malformed, of another length than the sequence, or holds a non-canonical pair";
            continue;
        }
        d[p] = rec_out[p].dist = mv[p].d; n_rem[p] = mv[p].n_rem;
        if ((long long)widths[p] * d[p] > RAFFT_FINDPATH_MAX_CANDIDATES) {
            rec_out[p].status = RAFFT_ERR_CAPACITY;
            if (err.empty())
                err = who + ": width " + std::to_string(widths[p]) + " x " + std::to_string(d[p]) + " moves is above RAFFT_FINDPATH_MAX_CANDIDATES";
            continue;
        }
        run.push_back(p);
    }
    g_err = err;
    if (run.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    const FpLayout y = findpath_layout(n_paths, run, pk.L.data(), d.data(), n_rem.data(), widths, pk.code_off.data(), workspace_budget(workspace_bytes));
    FpProb *d_ps; FpRec *d_rec; int *d_order; unsigned char *d_in, *d_out, *d_ws;
    if (int rc = mem.alloc(d_ps, y.ps.size() * sizeof(FpProb))) return rc;
    if (int rc = mem.alloc(d_rec, y.ps.size() * sizeof(FpRec))) return rc;
    if (int rc = mem.alloc(d_order, run.size() * 4)) return rc;
    if (int rc = mem.alloc(d_in, y.max_in + 16)) return rc;
    if (int rc = mem.alloc(d_out, y.max_out + 16)) return rc;
    if (int rc = mem.alloc(d_ws, y.plan.max_cost + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_ps, y.ps.data(), y.ps.size() * sizeof(FpProb), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_order, run.data(), run.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_rec, 0, y.ps.size() * sizeof(FpRec), st));
    std::vector<unsigned char> in(y.max_in + 16), out(y.max_out + 16);
    std::vector<FpRec> rec(n_paths);
    g_findpath_counters[0] = (long long)y.plan.chunks.size();
    g_findpath_counters[3] = (long long)run.size();
    for (size_t ci = 0; ci < y.plan.chunks.size(); ci++) {
        const ChunkPlan::Range &c = y.plan.chunks[ci];
        const unsigned ny = (unsigned)(c.b - c.a);
        int Lmax = 0, Wmax = 0;
        for (size_t k = c.a; k < c.b; k++) {
            const int p = run[k], L = pk.L[p];
            const FpProb &q = y.ps[p];
            const FpMoves &m = mv[p];
            unsigned char *at = in.data() + q.in_off;
            memset(at, 0, (size_t)fp_in_conf_off(L, q.d));
            memcpy(at, m.pt_a.data(), (size_t)L * 2);
            memcpy(at + fp_in_pt_bytes(L), m.pt_b.data(), (size_t)L * 2);
            if (q.d) memcpy(at + fp_in_moves_off(L), m.moves.data(), (size_t)q.d * 4);
            if (!m.conf.empty()) memcpy(at + fp_in_conf_off(L, q.d), m.conf.data(), m.conf.size() * 8);
            Lmax = std::max(Lmax, L);
            Wmax = std::max(Wmax, q.d < 30 ? std::min(widths[p], 1 << q.d) : widths[p]);      // (a level holds at most 2^d states)
        }
        const int *ord = d_order + c.a;
        const int dmax = y.chunk_dmax[ci], lds_pt = fp_expand_lds_pt(Lmax);
        HIPCHK(hipMemcpyAsync(d_in, in.data(), y.chunk_in[ci], hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(findpath_init_kernel<0>, dim3(ny), dim3(64), 0, st, g.T, d_ps, ord, sc.d_codes, d_in, d_ws, d_rec);
        HIPCHK(hipGetLastError());
        for (int level = 0; level < dmax; level++) {
            hipLaunchKernelGGL(findpath_expand_kernel<0>, dim3((unsigned)Wmax, ny), dim3(64), (size_t)fp_expand_lds_bytes(Lmax, dmax), st, g.T, d_ps, ord, sc.d_codes,
                               d_in, d_ws, d_rec, level, lds_pt);
            hipLaunchKernelGGL(findpath_select_kernel<0>, dim3(ny), dim3(FP_SEL_NT), 0, st, d_ps, ord, d_ws, d_rec, level);
        }
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(findpath_trace_kernel<0>, dim3((ny + 63) / 64), dim3(64), 0, st, (int)ny, d_ps, ord, d_in, d_ws, d_out, d_rec);
        HIPCHK(hipGetLastError());
        g_findpath_counters[1] += dmax;
        g_findpath_counters[2] += 2 + 2 * (long long)dmax;
        HIPCHK(hipMemcpyAsync(out.data(), d_out, y.chunk_out[ci], hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(rec.data(), d_rec, y.ps.size() * sizeof(FpRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = c.a; k < c.b; k++) {
            const int p = run[k];
            const FpProb &q = y.ps[p];
            const FpRec &r = rec[p];
            const std::string who = "problem " + std::to_string(p);
            if (r.flags & (FP_BAD_PAIR | FP_STUCK)) return fail(RAFFT_ERR_HIP, "internal: " + who + ((r.flags & FP_STUCK) ? ": a level without a candidate" : ": a non-canonical pair on the device"));
            if (r.flags & FP_RANGE) {
                rec_out[p].status = RAFFT_ERR_CAPACITY;
                if (err.empty()) err = who + ": an energy of the path is outside what the sort key holds (|energy| >= " + std::to_string(FINDPATH_BIAS) + " dcal)";
                continue;
            }
            if (r.end != r.end_eval) return fail(RAFFT_ERR_HIP, "internal: " + who + ": the path ends at another energy than the end structure has");
            rec_out[p] = rafft_findpath_rec{0, q.d, q.d, r.start, r.end, r.saddle, r.saddle_step, 0};
            if (moves_out && moves_out[p] && q.d) memcpy(moves_out[p], out.data() + q.out_off, (size_t)q.d * 8);
            if (dcal_out && dcal_out[p]) memcpy(dcal_out[p], out.data() + q.out_off + fp_out_dcal_off(q.d), ((size_t)q.d + 1) * 4);
        }
    }
    g_err = err;
    return 0;
}

// ---- the row drivers: descend, barriers, kinfold.  Their row intake (row_ptr, ROW_PARSE_ERR, copy_row_back, FirstError) is host-pure.

// The pair table of row r of sequence s again, when its chunk is staged: the first pass over the rows keeps none.
static int restage_row(const SeqPack &pk, const char *const *rows, const int *row_stride, int s, int r, int L, std::vector<int16_t> &pt)
{
    if (descend_parse_row(pk.codes.data() + pk.code_off[s], L, row_ptr(rows, row_stride, s, r), pt)) return fail(RAFFT_ERR_PARAM, "a row changed during the call");
    return 0;
}

// ---- gradient walks to local minima

// of the last call: chunks, kernel launches, walks that ran, steps over all walks
long long g_descend_counters[4];

// rafft_descend_batch (arguments validated by the entry point).  One pack of the sequences; every row of a sequence without an
// error is checked (descend_parse_row; its pair table is formed again when its chunk is staged); the walks that are left are laid out in chunks (descend_layout).  Per chunk: one upload of
// the pair tables, one launch of descend_kernel (one wavefront per walk), one download of the end rows, of the records and - when
// any walk of the chunk has a move buffer - of the moves, one synchronise.
int descend_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                  double temp, int max_steps, long long workspace_bytes, rafft_descend_seq *seq_out, rafft_descend_row *row_out,
                  char *const *db_out, int *const *moves_out)
{
    if (int rc = check_temp(temp)) return rc;
    for (long long &c : g_descend_counters) c = 0;
    if (n_seq == 0) return 0;
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_DESCEND_MAX_LEN);
    FirstError err(pk);                 // (items: rows)
    struct Where { int s, r; };
    std::vector<Where> run;
    std::vector<int> wL, wbound;
    std::vector<unsigned long long> wcode;
    std::vector<unsigned char> wmoves;
    std::vector<int16_t> pt;            // (one table, filled again per row: a call of millions of rows keeps none)
    int row0 = 0;
    for (int s = 0; s < n_seq; s++) {
        const int len = pk.len[s], L = pk.L[s];
        seq_out[s] = rafft_descend_seq{pk.status[s], len, n_rows[s], row0};
        for (int r = 0; r < n_rows[s]; r++) {
            rafft_descend_row &o = row_out[row0 + r];
            char *db = db_out[s] + (size_t)r * ((size_t)len + 1);
            o = rafft_descend_row{pk.status[s], 0, 0, 0};
            if (pk.status[s]) { dot_row(db, len); continue; }
            const char *row = row_ptr(rows, row_stride, s, r);
            if (int st = descend_parse_row(pk.codes.data() + pk.code_off[s], L, row, pt)) {
                o.status = st;
                copy_row_back(db, row, L);
                err.note(s, r, "sequence " + std::to_string(s) + " row " + std::to_string(r) + ROW_PARSE_ERR);
                continue;
            }
            run.push_back(Where{s, r});
            wL.push_back(L); wbound.push_back(descend_bound(L, max_steps)); wcode.push_back(pk.code_off[s]);
            wmoves.push_back(moves_out && moves_out[s] ? 1 : 0);
        }
        row0 += n_rows[s];
    }
    g_err = err.text();
    if (run.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    const DsLayout y = descend_layout(run.size(), wL.data(), wbound.data(), wcode.data(), wmoves.data(), workspace_budget(workspace_bytes));
    DsWalk *d_ws; DsRec *d_rec; unsigned char *d_io, *d_mv = nullptr;
    if (int rc = mem.alloc(d_ws, run.size() * sizeof(DsWalk))) return rc;
    if (int rc = mem.alloc(d_rec, run.size() * sizeof(DsRec))) return rc;
    if (int rc = mem.alloc(d_io, y.max_io + 16)) return rc;
    if (y.max_mv) if (int rc = mem.alloc(d_mv, y.max_mv + 16)) return rc;      // (no caller asked for moves: no buffer)
    HIPCHK(hipMemcpyAsync(d_ws, y.ws.data(), run.size() * sizeof(DsWalk), hipMemcpyHostToDevice, st));
    std::vector<unsigned char> io(y.max_io + 16), mv(y.max_mv + 16);
    std::vector<DsRec> rec(run.size());
    g_descend_counters[0] = (long long)y.plan.chunks.size();
    g_descend_counters[2] = (long long)run.size();
    for (size_t ci = 0; ci < y.plan.chunks.size(); ci++) {
        const ChunkPlan::Range &c = y.plan.chunks[ci];
        const size_t nw = c.b - c.a;
        for (size_t k = c.a; k < c.b; k++) {
            if (int rc = restage_row(pk, rows, row_stride, run[k].s, run[k].r, wL[k], pt)) return rc;
            memcpy(io.data() + y.ws[k].io_off, pt.data(), (size_t)wL[k] * 2);
        }
        HIPCHK(hipMemcpyAsync(d_io, io.data(), y.chunk_io[ci], hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(descend_kernel<0>, dim3((unsigned)nw), dim3(64), (size_t)descend_lds_bytes(y.chunk_lmax[ci]), st, g.T, d_ws + c.a, sc.d_codes,
                           d_io, d_mv, d_rec + c.a);
        HIPCHK(hipGetLastError());
        g_descend_counters[1]++;
        HIPCHK(hipMemcpyAsync(io.data(), d_io, y.chunk_io[ci], hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(rec.data() + c.a, d_rec + c.a, nw * sizeof(DsRec), hipMemcpyDeviceToHost, st));
        if (y.chunk_mv[ci]) HIPCHK(hipMemcpyAsync(mv.data(), d_mv, y.chunk_mv[ci], hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = c.a; k < c.b; k++) {
            const int s = run[k].s, r = run[k].r, L = wL[k];
            const DsRec &d = rec[k];
            const std::string who = "sequence " + std::to_string(s) + " row " + std::to_string(r);
            if (d.flags & DS_BAD_PAIR) return fail(RAFFT_ERR_HIP, "internal: " + who + ": a non-canonical pair on the device");
            if (d.n_steps < 0 || d.n_steps > wbound[k]) return fail(RAFFT_ERR_HIP, "internal: " + who + ": more steps than the bound");
            rafft_descend_row &o = row_out[seq_out[s].row0 + r];
            o = rafft_descend_row{(d.flags & DS_MORE) ? RAFFT_ERR_CAPACITY : 0, d.n_steps, d.start, d.end};
            if (d.flags & DS_MORE) err.note(s, r, who + ": not at a minimum after " + std::to_string(d.n_steps) + " steps (max_steps)");
            memcpy(db_out[s] + (size_t)r * ((size_t)L + 1), io.data() + y.ws[k].io_off, (size_t)L + 1);
            if (wmoves[k] && d.n_steps)
                memcpy(moves_out[s] + (size_t)r * 2 * (size_t)wbound[k], mv.data() + y.ws[k].mv_off, (size_t)d.n_steps * 8);
            g_descend_counters[3] += d.n_steps;
        }
    }
    g_err = err.text();
    return 0;
}

// ---- exact barrier trees of energy bands

constexpr size_t BARRIERS_WORKSPACE_MAX = (size_t)64 << 30;        // (a chunk's rows are numbered in 31 bits: at 56 bytes a row and more, this holds them)

// what a rafft_barriers_result points into; rafft_barriers_free deletes it
struct BarriersOwner {
    rafft_barriers_result res;
    std::vector<rafft_barriers_seq> seq;
    std::vector<std::vector<rafft_barriers_min>> minima;
    std::vector<std::vector<rafft_barriers_edge>> edges;
    std::vector<std::vector<int32_t>> basin;
};

// of the last call: chunks, kernel launches, rows that ran, neighbour probes that hit, minima, edges
long long g_barriers_counters[6];

// rafft_barriers_batch (arguments validated by the entry point).  One pack of the sequences; every row of a sequence without an
// error is checked (descend_parse_row; its pair table is formed again when its chunk is staged) and so is the order of its dcal;
// the sequences that are left are laid out in chunks (barriers_layout).  Per chunk: one upload of the pair tables, the five
// launches of rafft_barriers.hip, one download of basin (as ranks of minima), of the edge table and of the records, one
// synchronise; then, per sequence on the host, the minima numbered by rank, the basin sizes, the edges compacted and sorted, and
// the tree (barriers_tree).  No energy table is read: the call has no temperature.
int barriers_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                   const int *const *dcal, int max_edges, long long workspace_bytes, rafft_barriers_result **out)
{
    *out = nullptr;
    for (long long &c : g_barriers_counters) c = 0;
    std::unique_ptr<BarriersOwner> own(new BarriersOwner);
    own->seq.resize(n_seq); own->minima.resize(n_seq); own->edges.resize(n_seq); own->basin.resize(n_seq);
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_BARRIERS_MAX_LEN);
    const size_t budget = std::min(workspace_budget(workspace_bytes), BARRIERS_WORKSPACE_MAX);
    FirstError err(pk);                 // (no items: every error is its sequence's)
    auto note = [&](int s, int status, const std::string &msg) {
        own->seq[s].status = status;
        err.note(s, -1, "sequence " + std::to_string(s) + ": " + msg);
    };
    std::vector<int> run, rL, rn;
    std::vector<unsigned long long> rcode;
    std::vector<int16_t> pt;
    for (int s = 0; s < n_seq; s++) {
        const int L = pk.L[s];
        own->seq[s] = rafft_barriers_seq{pk.status[s], pk.len[s], n_rows[s], 0, 0, 0, nullptr, nullptr, nullptr};
        if (pk.status[s]) continue;
        if (n_rows[s] == 0) { note(s, RAFFT_ERR_EMPTY, "no rows"); continue; }
        if (n_rows[s] > RAFFT_BARRIERS_MAX_ROWS) { note(s, RAFFT_ERR_CAPACITY, "more than RAFFT_BARRIERS_MAX_ROWS rows"); continue; }
        int bad = -1, dec = -1;
        for (int r = 0; r < n_rows[s] && bad < 0 && dec < 0; r++) {
            if (descend_parse_row(pk.codes.data() + pk.code_off[s], L, row_ptr(rows, row_stride, s, r), pt)) bad = r;
            else if (r > 0 && dcal[s][r] < dcal[s][r - 1]) dec = r;
        }
        if (bad >= 0) { note(s, RAFFT_ERR_STRUCT, "row " + std::to_string(bad) + ROW_PARSE_ERR); continue; }
        if (dec >= 0) { note(s, RAFFT_ERR_STRUCT, "row " + std::to_string(dec) + ": its dcal is below that of the row before it"); continue; }
        const unsigned long long area = barriers_area_bytes(L, n_rows[s], barriers_edge_cap(n_rows[s], max_edges));
        if (area > (unsigned long long)budget) {
            note(s, RAFFT_ERR_CAPACITY, "its work area needs " + std::to_string(area) + " bytes, workspace_bytes is " + std::to_string(budget));
            continue;
        }
        run.push_back(s); rL.push_back(L); rn.push_back(n_rows[s]); rcode.push_back(pk.code_off[s]);
    }
    auto finish = [&]() {
        int n_failed = 0;
        for (int s = 0; s < n_seq; s++) {
            rafft_barriers_seq &o = own->seq[s];
            n_failed += o.status != 0;
            if (o.status) { own->minima[s].clear(); own->edges[s].clear(); own->basin[s].clear(); o.n_minima = o.n_edges = 0; }
            // (never a null pointer, as rafft_subopt_seq: an empty list points at one spare element)
            if (own->minima[s].empty()) own->minima[s].reserve(1);
            if (own->edges[s].empty()) own->edges[s].reserve(1);
            if (own->basin[s].empty()) own->basin[s].reserve(1);
            o.minima = own->minima[s].data(); o.edges = own->edges[s].data(); o.basin = own->basin[s].data();
        }
        own->res = rafft_barriers_result{n_seq, n_failed, own->seq.data(), own.get()};
        *out = &own->res;
        own.release();
        g_err = err.text();
        return 0;
    };
    if (run.empty()) return finish();
    SeamGuard sg;
    DevScratch mem;
    if (int rc = sg.enter()) return rc;
    hipStream_t st = sg.stream;
    const BarLayout y = barriers_layout(run.size(), rL.data(), rn.data(), rcode.data(), max_edges, budget);
    uint8_t *d_codes; BarSeq *d_qs; BarRec *d_rec; unsigned char *d_pt; uint64_t *d_keys; unsigned long long *d_tab, *d_ekeys; unsigned *d_evals; int *d_down, *d_basin;
    if (int rc = mem.alloc(d_codes, pk.codes.size())) return rc;
    if (int rc = mem.alloc(d_qs, run.size() * sizeof(BarSeq))) return rc;
    if (int rc = mem.alloc(d_rec, run.size() * sizeof(BarRec))) return rc;
    if (int rc = mem.alloc(d_pt, y.max_pt + 16)) return rc;
    if (int rc = mem.alloc(d_keys, y.max_rows * 16 + 16)) return rc;
    if (int rc = mem.alloc(d_tab, y.max_tab * 8)) return rc;
    if (int rc = mem.alloc(d_ekeys, y.max_edge * 8)) return rc;
    if (int rc = mem.alloc(d_evals, y.max_edge * 4)) return rc;
    if (int rc = mem.alloc(d_down, y.max_rows * 4 + 16)) return rc;
    if (int rc = mem.alloc(d_basin, y.max_rows * 4 + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_codes, pk.codes.data(), pk.codes.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_qs, y.qs.data(), run.size() * sizeof(BarSeq), hipMemcpyHostToDevice, st));
    std::vector<BarRec> rec(run.size(), BarRec{BAR_EMPTY, 0, 0, 0});
    HIPCHK(hipMemcpyAsync(d_rec, rec.data(), run.size() * sizeof(BarRec), hipMemcpyHostToDevice, st));
    std::vector<unsigned char> hpt(y.max_pt + 16);
    std::vector<int> hbasin(y.max_rows);
    std::vector<unsigned long long> hek(y.max_edge);
    std::vector<unsigned> hev(y.max_edge);
    std::vector<int32_t> index, father, saddle;
    g_barriers_counters[0] = (long long)y.plan.chunks.size();
    for (size_t ci = 0; ci < y.plan.chunks.size(); ci++) {
        const ChunkPlan::Range &c = y.plan.chunks[ci];
        const int nq = (int)(c.b - c.a);
        const unsigned nr = (unsigned)y.chunk_rows[ci];
        for (size_t k = c.a; k < c.b; k++) {
            const int s = run[k];
            const BarSeq &q = y.qs[k];
            for (int r = 0; r < q.n_rows; r++) {
                if (int rc = restage_row(pk, rows, row_stride, s, r, q.L, pt)) return rc;
                memcpy(hpt.data() + q.pt_off + (size_t)r * (size_t)q.pt_stride, pt.data(), (size_t)q.L * 2);
            }
        }
        HIPCHK(hipMemcpyAsync(d_pt, hpt.data(), y.chunk_pt[ci], hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_tab, 0xff, y.chunk_tab[ci] * 8, st));
        HIPCHK(hipMemsetAsync(d_ekeys, 0xff, y.chunk_edge[ci] * 8, st));
        HIPCHK(hipMemsetAsync(d_evals, 0xff, y.chunk_edge[ci] * 4, st));
        const size_t lds = (size_t)barriers_lds_bytes(y.chunk_lmax[ci]);
        const unsigned nb = (nr + 255u) / 256u;
        const BarSeq *qs = d_qs + c.a;
        BarRec *rc = d_rec + c.a;
        hipLaunchKernelGGL(barriers_keys_kernel<0>, dim3(nr), dim3(64), 0, st, qs, nq, d_pt, d_keys);
        hipLaunchKernelGGL(barriers_insert_kernel<0>, dim3(nb), dim3(256), 0, st, qs, nq, nr, d_keys, d_tab, rc);
        hipLaunchKernelGGL(barriers_scan_kernel<BAR_DOWN>, dim3(nr), dim3(64), lds, st, qs, nq, d_codes, d_pt, d_keys, d_tab, d_down, d_basin, d_ekeys, d_evals, rc);
        hipLaunchKernelGGL(barriers_basin_kernel<0>, dim3(nb), dim3(256), 0, st, qs, nq, nr, d_down, d_basin, rc);
        hipLaunchKernelGGL(barriers_scan_kernel<BAR_EDGES>, dim3(nr), dim3(64), lds, st, qs, nq, d_codes, d_pt, d_keys, d_tab, d_down, d_basin, d_ekeys, d_evals, rc);
        HIPCHK(hipGetLastError());
        g_barriers_counters[1] += 5;
        g_barriers_counters[2] += nr;
        HIPCHK(hipMemcpyAsync(hbasin.data(), d_basin, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hek.data(), d_ekeys, y.chunk_edge[ci] * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hev.data(), d_evals, y.chunk_edge[ci] * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(rec.data() + c.a, rc, (size_t)nq * sizeof(BarRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = c.a; k < c.b; k++) {
            const int s = run[k];
            const BarSeq &q = y.qs[k];
            const BarRec &d = rec[k];
            const int n = q.n_rows;
            g_barriers_counters[3] += (long long)d.hits;
            if (d.flags & BAR_TABLE_BAD) return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + ": the row table is inconsistent");
            if (d.dup != BAR_EMPTY) {
                note(s, RAFFT_ERR_STRUCT, "rows " + std::to_string((unsigned)d.dup) + " and " + std::to_string((unsigned)(d.dup >> 32)) + " are the same structure");
                continue;
            }
            if (d.flags & BAR_EDGES_FULL) {
                note(s, RAFFT_ERR_CAPACITY, "more than " + std::to_string(q.edge_cap) + " edges between basins: raise max_edges");
                continue;
            }
            // minima by ascending rank, basins as their indices, basin sizes
            const int *bs = hbasin.data() + q.row0;
            std::vector<rafft_barriers_min> &mn = own->minima[s];
            std::vector<int32_t> &basin = own->basin[s];
            index.assign((size_t)n, -1);
            for (int x = 0; x < n; x++) {
                if (bs[x] < 0 || bs[x] > x) return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + ": a basin outside the rows");
                if (bs[x] == x) { index[x] = (int32_t)mn.size(); mn.push_back(rafft_barriers_min{x, -1, -1, dcal[s][x], 0, 0}); }
            }
            basin.resize((size_t)n);
            for (int x = 0; x < n; x++) {
                const int32_t m = index[bs[x]];
                if (m < 0) return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + ": a basin that is no minimum");
                basin[x] = m;
                mn[m].basin_size++;
            }
            // the edge table, compacted and sorted
            std::vector<rafft_barriers_edge> &ed = own->edges[s];
            for (size_t e = q.edge_off; e <= q.edge_off + q.edge_mask; e++) {
                if (hek[e] == BAR_EMPTY) continue;
                const unsigned a = (unsigned)(hek[e] >> 32), b = (unsigned)hek[e];
                if (a >= (unsigned)n || b >= (unsigned)n || hev[e] >= (unsigned)n || index[a] < 0 || index[b] < 0)
                    return fail(RAFFT_ERR_HIP, "internal: sequence " + std::to_string(s) + ": an edge outside the minima");
                ed.push_back(rafft_barriers_edge{index[a], index[b], (int32_t)hev[e]});
            }
            std::sort(ed.begin(), ed.end(), [](const rafft_barriers_edge &u, const rafft_barriers_edge &v) {
                return u.saddle_rank != v.saddle_rank ? u.saddle_rank < v.saddle_rank : u.a != v.a ? u.a < v.a : u.b < v.b;
            });
            barriers_tree((int)mn.size(), ed, father, saddle);
            for (size_t m = 0; m < mn.size(); m++) {
                mn[m].father = father[m]; mn[m].saddle_rank = saddle[m];
                mn[m].saddle_dcal = saddle[m] >= 0 ? dcal[s][saddle[m]] : 0;
            }
            own->seq[s].n_minima = (int32_t)mn.size();
            own->seq[s].n_edges = (int32_t)ed.size();
            g_barriers_counters[4] += (long long)mn.size();
            g_barriers_counters[5] += (long long)ed.size();
        }
    }
    return finish();
}

// ---- stochastic folding trajectories

// of the last call: chunks, kernel launches, trajectories that ran, steps over all trajectories
long long g_kinfold_counters[4];

// rafft_kinfold_batch (arguments validated by the entry point).  One pack of the sequences; the watched rows of every sequence
// without an error become pair tables (a bad one is the sequence's error); every start row of what is left is checked
// (descend_parse_row; its pair table is formed again when its chunk is staged, once for its n_rep trajectories); the trajectories
// are laid out in chunks (kinfold_layout).  Per call: one upload of the weight table, the sample times and the watched tables.  Per
// chunk: one upload of the pair tables, one launch of kinfold_kernel (one wavefront per trajectory), one download of the end rows,
// the records, the sample records and - when any trajectory of the chunk has a log - the logs, one synchronise.
int kinfold_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                  int n_rep, const int *n_watch, const int *n_stop, const char *const *watch, const int *watch_stride,
                  const unsigned long long *seeds, double temp, double kt, double t_max, int max_steps, int n_times, const double *sample_times,
                  long long workspace_bytes, rafft_kinfold_seq *seq_out, rafft_kinfold_traj *traj_out, char *const *db_out,
                  int32_t *const *samples_out, int *const *moves_out, double *const *times_out)
{
    if (int rc = check_temp(temp)) return rc;
    for (long long &c : g_kinfold_counters) c = 0;
    if (n_seq == 0) return 0;
    std::vector<uint64_t> wtab(RAFFT_KINFOLD_NW);
    if (!kinfold_weights(temp, kt, wtab.data())) return fail(RAFFT_ERR_PARAM, "kT is not above 0");
    const SeqPack pk = pack_sequences(n_seq, seqs, lens, RAFFT_KINFOLD_MAX_LEN);
    FirstError err(pk);                 // (items: trajectories)
    const int bound = kinfold_bound(max_steps);
    struct Where { int s, k; };
    std::vector<Where> run;
    std::vector<int> wL, wnw, wns;
    std::vector<unsigned> wk;
    std::vector<unsigned long long> wcode, wwt, wseed;
    std::vector<unsigned char> wlog;
    std::vector<int16_t> pt, watch_pt;  // (pt: one table, filled again per row; watch_pt: the watched tables of the call)
    int traj0 = 0;
    for (int s = 0; s < n_seq; s++) {
        const int len = pk.len[s], L = pk.L[s], nw = n_watch ? n_watch[s] : 0, ns = n_watch ? n_stop[s] : 0;
        const int n_traj = n_rows[s] * n_rep;
        int status = pk.status[s];
        const unsigned long long wt_off = watch_pt.size();
        for (int w = 0; w < nw && !status; w++) {
            if (descend_parse_row(pk.codes.data() + pk.code_off[s], L, row_ptr(watch, watch_stride, s, w), pt)) {
                status = RAFFT_ERR_STRUCT;
                watch_pt.resize(wt_off);
                err.note(s, -1, "sequence " + std::to_string(s) + " watched row " + std::to_string(w) + ROW_PARSE_ERR);
            } else watch_pt.insert(watch_pt.end(), pt.begin(), pt.end());
        }
        seq_out[s] = rafft_kinfold_seq{status, len, n_traj, traj0};
        for (int r = 0; r < n_rows[s]; r++) {
            int st = status;
            const char *row = row_ptr(rows, row_stride, s, r);
            if (!st && descend_parse_row(pk.codes.data() + pk.code_off[s], L, row, pt)) {
                st = RAFFT_ERR_STRUCT;
                err.note(s, (long long)r * n_rep, "sequence " + std::to_string(s) + " row " + std::to_string(r) + ROW_PARSE_ERR);
            }
            for (int rep = 0; rep < n_rep; rep++) {
                const int k = r * n_rep + rep;
                traj_out[traj0 + k] = rafft_kinfold_traj{st, 0, 0, 0, 0, -1, 0.0};
                if (!st) {
                    run.push_back(Where{s, k});
                    wL.push_back(L); wk.push_back((unsigned)k); wcode.push_back(pk.code_off[s]); wwt.push_back(wt_off);
                    wseed.push_back(seeds ? seeds[s] : 0ull); wnw.push_back(nw); wns.push_back(ns);
                    wlog.push_back(moves_out && times_out && moves_out[s] && times_out[s] ? 1 : 0);
                    continue;
                }
                char *db = db_out[s] + (size_t)k * ((size_t)len + 1);
                if (status) dot_row(db, len);
                else copy_row_back(db, row, L);
                if (n_times && samples_out && samples_out[s])
                    for (int t = 0; t < n_times; t++) { int32_t *o = samples_out[s] + ((size_t)k * n_times + t) * 2; o[0] = INT32_MIN; o[1] = -2; }
            }
        }
        traj0 += n_traj;
    }
    g_err = err.text();
    if (run.empty()) return 0;
    SeqCall sc;
    DevScratch mem;
    if (int rc = sc.open(mem, pk, temp)) return rc;
    hipStream_t st = sc.st;
    const KfLayout y = kinfold_layout(run.size(), wL.data(), wk.data(), wcode.data(), wwt.data(), wseed.data(), wnw.data(), wns.data(), wlog.data(),
                                      bound, n_times, workspace_budget(workspace_bytes));
    KfTraj *d_ws; KfRec *d_rec; KfSample *d_smp; unsigned char *d_io, *d_log = nullptr;
    unsigned long long *d_wtab; double *d_times; int16_t *d_watch;
    if (int rc = mem.alloc(d_ws, run.size() * sizeof(KfTraj))) return rc;
    if (int rc = mem.alloc(d_rec, run.size() * sizeof(KfRec))) return rc;
    if (int rc = mem.alloc(d_smp, y.max_traj * (size_t)n_times * sizeof(KfSample) + 16)) return rc;
    if (int rc = mem.alloc(d_io, y.max_io + 16)) return rc;
    if (y.max_log) if (int rc = mem.alloc(d_log, y.max_log + 16)) return rc;   // (no caller asked for a log: no buffer)
    if (int rc = mem.alloc(d_wtab, wtab.size() * sizeof(uint64_t))) return rc;
    if (int rc = mem.alloc(d_times, (size_t)n_times * sizeof(double) + 16)) return rc;
    if (int rc = mem.alloc(d_watch, watch_pt.size() * sizeof(int16_t) + 16)) return rc;
    HIPCHK(hipMemcpyAsync(d_ws, y.ws.data(), run.size() * sizeof(KfTraj), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_wtab, wtab.data(), wtab.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (n_times) HIPCHK(hipMemcpyAsync(d_times, sample_times, (size_t)n_times * sizeof(double), hipMemcpyHostToDevice, st));
    if (!watch_pt.empty()) HIPCHK(hipMemcpyAsync(d_watch, watch_pt.data(), watch_pt.size() * sizeof(int16_t), hipMemcpyHostToDevice, st));
    std::vector<unsigned char> io(y.max_io + 16), lg(y.max_log + 16);
    std::vector<KfRec> rec(run.size());
    std::vector<KfSample> smp(y.max_traj * (size_t)n_times + 1);
    g_kinfold_counters[0] = (long long)y.plan.chunks.size();
    g_kinfold_counters[2] = (long long)run.size();
    for (size_t ci = 0; ci < y.plan.chunks.size(); ci++) {
        const ChunkPlan::Range &c = y.plan.chunks[ci];
        const size_t nt = c.b - c.a;
        for (size_t t = c.a; t < c.b; t++) {
            const int s = run[t].s, r = run[t].k / n_rep;
            if (t == c.a || run[t - 1].s != s || run[t - 1].k / n_rep != r)
                if (int rc = restage_row(pk, rows, row_stride, s, r, wL[t], pt)) return rc;
            memcpy(io.data() + y.ws[t].io_off, pt.data(), (size_t)wL[t] * 2);
        }
        HIPCHK(hipMemcpyAsync(d_io, io.data(), y.chunk_io[ci], hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(kinfold_kernel<0>, dim3((unsigned)nt), dim3(64), (size_t)kinfold_lds_bytes(y.chunk_lmax[ci]), st, g.T, d_ws + c.a, sc.d_codes,
                           d_io, d_log, d_watch, d_wtab, d_times, n_times, t_max, d_smp, d_rec + c.a);
        HIPCHK(hipGetLastError());
        g_kinfold_counters[1]++;
        HIPCHK(hipMemcpyAsync(io.data(), d_io, y.chunk_io[ci], hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(rec.data() + c.a, d_rec + c.a, nt * sizeof(KfRec), hipMemcpyDeviceToHost, st));
        if (n_times) HIPCHK(hipMemcpyAsync(smp.data(), d_smp, nt * (size_t)n_times * sizeof(KfSample), hipMemcpyDeviceToHost, st));
        if (y.chunk_log[ci]) HIPCHK(hipMemcpyAsync(lg.data(), d_log, y.chunk_log[ci], hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t t = c.a; t < c.b; t++) {
            const int s = run[t].s, k = run[t].k, L = wL[t];
            const KfRec &d = rec[t];
            const std::string who = "sequence " + std::to_string(s) + " trajectory " + std::to_string(k);
            if (d.flags & KF_BAD_PAIR) return fail(RAFFT_ERR_HIP, "internal: " + who + ": a non-canonical pair on the device");
            if (d.flags & KF_STUCK) return fail(RAFFT_ERR_HIP, "internal: " + who + ": the drawn number met no move");
            if (d.n_steps < 0 || d.n_steps > bound) return fail(RAFFT_ERR_HIP, "internal: " + who + ": more steps than the bound");
            traj_out[seq_out[s].traj0 + k] = rafft_kinfold_traj{(d.flags & KF_MORE) ? RAFFT_ERR_CAPACITY : 0, d.flags, d.n_steps, d.start, d.end, d.stop, d.time};
            if (d.flags & KF_MORE) err.note(s, k, who + ": not ended after " + std::to_string(d.n_steps) + " steps (max_steps)");
            memcpy(db_out[s] + (size_t)k * ((size_t)L + 1), io.data() + y.ws[t].io_off, (size_t)L + 1);
            if (n_times && samples_out && samples_out[s])
                memcpy(samples_out[s] + (size_t)k * n_times * 2, smp.data() + (t - c.a) * (size_t)n_times, (size_t)n_times * sizeof(KfSample));
            if (wlog[t] && d.n_steps) {
                memcpy(moves_out[s] + (size_t)k * 2 * (size_t)bound, lg.data() + y.ws[t].log_off, (size_t)d.n_steps * 8);
                memcpy(times_out[s] + (size_t)k * (size_t)bound, lg.data() + y.ws[t].log_off + 8ull * (size_t)bound, (size_t)d.n_steps * 8);
            }
            g_kinfold_counters[3] += d.n_steps;
        }
    }
    g_err = err.text();
    return 0;
}

} // namespace
