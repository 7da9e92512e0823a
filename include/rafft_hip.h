/*
 * rafft_hip.h - C-ABI of libraffthip.so, the MI355X (gfx950) RAFFT folding engine.
 *
 * The reference (lemerleau/RAFFT) is pure Python and has no FFI; its seam for the
 * fold hot path is the Python API + CLI + fast-folding-graph text format
 * (SURVEY.md section 8b).  This header is what a maintainer of the reference binds
 * with ctypes to make `rafft.fold()` / `bin/rafft` run on the
 * GPU.  Plain C types only; no exceptions cross the boundary; the library allocates
 * results and the caller frees them with rafft_free_result().
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference tree).
 */
#ifndef RAFFT_HIP_H
#define RAFFT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (per call and per sequence) */
enum {
    RAFFT_OK = 0,
    RAFFT_ERR_BAD_CHAR = 1,      /* reference: KeyError from prep_sequence, rafft/utils.py:73-80 */
    RAFFT_ERR_EMPTY = 2,         /* reference: numpy AxisError from flip(), rafft/utils.py:83 */
    RAFFT_ERR_TOO_LONG = 3,      /* L > RAFFT_MAX_LEN (the LDS plan of the biggest regions: 2 bytes per position; 16-bit pair tables) */
    RAFFT_ERR_TEMP = 4,          /* temp != 37 with the built-in 37 C tables (no enthalpies): load a parameter file first */
    RAFFT_ERR_CAPACITY = 5,      /* an HBM arena overflowed even after regrowth */
    RAFFT_ERR_PARAM = 6,         /* unsupported parameter combination (e.g. max_branch+2*max_stack too large) */
    RAFFT_ERR_HIP = 7,           /* HIP runtime error; see rafft_last_error() */
    RAFFT_ERR_STRUCT = 8,        /* malformed dot-bracket / non-canonical pair in rafft_eval_structure */
    RAFFT_ERR_NO_DEVICE = 9,
    RAFFT_ERR_INFEASIBLE = 10    /* rafft_mfe_constrained_batch: no structure satisfies the sequence's hard constraints */
};

#define RAFFT_MAX_LEN 32768

/* Mirrors the argument list of rafft.fold(), rafft/rafft.py:219-221 (and
 * Glob_parms, rafft/utils.py:9-21). */
typedef struct {
    int32_t nb_mode;     /* -n  : number of positional lags searched per unpaired region */
    int32_t max_stack;   /* -ms : beam width */
    int32_t max_branch;  /* --max_branch */
    int32_t min_hp;      /* -mh */
    double min_nrj;      /* -mn */
    int32_t traj;        /* 0: final beam only; 1: beam of every folding step */
    int32_t _pad;
    double temp;         /* md.temperature (rafft/utils.py:18); != 37.0 needs rafft_load_params() (enthalpy tables) */
    double gc_wei, au_wei, gu_wei;
} rafft_params;

/* Per-sequence result: the fast-folding graph (bin/rafft:73-79) as arrays.
 * n_steps == 1 when params.traj == 0 (the final beam). */
typedef struct {
    int32_t status;
    int32_t length;
    int32_t n_steps;
    int32_t n_structs;        /* total rows over all steps */
    const int32_t *step_size; /* [n_steps] */
    const int32_t *step_off;  /* [n_steps] first row of each step */
    const char *db;           /* n_structs rows of (length+1) bytes, NUL terminated dot-brackets */
    const int32_t *dcal;      /* [n_structs] free energy in dcal/mol; kcal/mol = (float)dcal/100 as
                                 ViennaRNA's eval_structure returns it (rafft/utils.py:135-138) */
} rafft_seq_result;

typedef struct {
    int32_t n_seq;
    int32_t n_failed;         /* sequences whose status != RAFFT_OK */
    rafft_seq_result *seq;    /* [n_seq] in input order */
    void *_owner;             /* private */
} rafft_result;

/* Kernel timing / traffic counters of the last rafft_fold_batch() on this thread's
 * device (HIP events on the library's own stream).  Timing events are not free (a pair around every
 * kernel costs ~7 % of a benchmark batch), so by default only ms_total and ms_expand are measured;
 * the other ms_* fields are filled when the environment has RAFFT_SPANS=2 (or RAFFT_TRACE) at the
 * time of the call, and stay 0 otherwise.  RAFFT_SPANS=0 switches ms_expand off as well. */
typedef struct {
    double ms_total;          /* wall time of the call, host side */
    double ms_expand;         /* sum of the durations of the dominant kernel, expand_kernel<64,true,16,0,1>: regions of 33..256 positions
                                 with up to 128 branches, sixteen one-wavefront teams per workgroup (HIP events on its own stream) */
    double ms_expand_c1;      /* expand_small_kernel<16|32>: regions of up to 32 positions whose every lag is searched, teams of 16 / 32 lanes */
    double ms_expand_c2;      /* expand_kernel<256,...>: regions of up to 1024 positions that do not fit the one-wavefront class; runs concurrently */
    double ms_expand_c3;      /* regions of 1025..4096 positions (expand_kernel<256,false,1,2,3>: direct correlation, lag values in HBM; the LDS FFT
                                 plan expand_kernel<512,...> with RAFFT_C3_DIRECT=0) and the class for regions beyond 4096 positions; concurrently */
    double ms_expand_wall;    /* fork->join wall time of the concurrent expand launches of every step */
    double ms_beam;           /* sum of beam-step kernel durations */
    double ms_materialize;    /* sum of materialize kernel durations */
    double ms_output;         /* output formatting kernel */
    int64_t n_expand_launches; /* launches of the dominant kernel (steps with few new structures send their regions to one of the
                                 wide kernels instead) */
    int64_t n_steps;          /* folding steps executed (max over sequences) */
    int64_t n_node_expansions;/* regions really expanded (identical loops are expanded once) */
    int64_t n_nodes_created;  /* region records written: one per (parent region, candidate, side) that a beam member picked, whoever picked it first */
    int64_t n_nodes_aliased;  /* ... of these: loops reached before along another path, which re-use that region's expansion */
    int64_t sum_node_len;     /* sum of n over expansions */
    int64_t sum_lags;         /* sum of min(nb_mode, 2n-1) over expansions */
    int64_t n_structs;        /* structures materialized (beam survivors) */
    int64_t n_children;       /* children accepted by the combine step */
    int64_t sum_struct_len;   /* sum of L over materialized structures */
    int64_t alg_bytes;        /* algorithmic HBM bytes, SURVEY.md section 8d formula */
    int64_t alg_bytes_expand; /* the part of the dominant kernel expand_kernel<64> (its regions; 3L per structure pro rata) */
    int64_t alg_bytes_expand_all; /* all three expand size classes */
    int64_t n_regrows;        /* times a wave of the call overflowed its HBM arenas and was re-run with larger ones */
    int64_t alg_bytes_expand_small; /* algorithmic bytes of the small-region classes (expand_small_kernel; ms_expand_c1 is their time) */
    int64_t alg_bytes_expand_c2;    /* ... of expand_kernel<256> (ms_expand_c2) */
    int64_t alg_bytes_expand_c3;    /* ... of expand_kernel<512> (ms_expand_c3) */
    int64_t alg_bytes_beam;         /* 2L + 8 per new structure: beam_step_kernel + materialize_kernel (ms_beam + ms_materialize) */
    int64_t n_node_instances;       /* (structure, region) pairs: entries of the structures' node lists (n_nodes_created of them needed a record) */
    int64_t n_dE_evals;             /* built-in tables only (0 with a loaded parameter file): candidate stems whose dE was evaluated, */
    int64_t n_dE_guessed;           /* ... those whose dE read an interior-loop table entry that no reference-held energy row exercises */
    int64_t n_kept_guessed;         /* ... and the ones of these that passed the filter dE < min_nrj (rafft/rafft.py:102): candidates a beam member may pick */
    int64_t n_regrows_prod;         /* ... of n_regrows: a structure had more productive regions than the short lists hold (same arenas, long lists) */
    int64_t n_waves_long_lists;     /* waves of the call folded with the long productive-region lists (1024 per structure instead of 64: a structure with
                                       more than 64 was met under these parameters; eight such waves in a row that never needed them switch back) */
} rafft_stats;

/* Select the GPU (HIP ordinal) and upload the energy tables.  Optional: every other
 * entry point initialises lazily on device 0. */
int rafft_init(int device);

/* Replaces: one rafft.fold() call per sequence (rafft/rafft.py:219-239), i.e. the
 * body of benchmark_results/bench_fft.py:8-22 for a whole batch.  `device` < 0 keeps
 * the current device.  Sequences are independent; results come back in input order. */
int rafft_fold_batch(const rafft_params *p, int n_seq, const char *const *seqs,
                     const int *lens, int device, rafft_result **out);

void rafft_free_result(rafft_result *r);

/* Waits for the batches in flight, stops the library's scheduler thread and joins it.  Registered with atexit() when the
 * first batch is submitted; call it by hand before dlclose().  Later calls start a fresh scheduler. */
void rafft_shutdown(void);

/* Allocation counters of the library, process-wide and monotonic: out[0] device buffers allocated so far (hipMalloc calls),
 * out[1] their bytes, out[2] the slowest of those calls in microseconds, out[3] pinned host chunks allocated, out[4] their
 * bytes.  Workspaces are sized once for the biggest wave the scheduler may merge and are kept, so a steady stream of equal
 * batches allocates nothing after its first waves; a caller that times a region (bench.py) takes the difference around
 * it and reports it - a hipMalloc of gigabytes takes seconds now and then (tools/micro/malloc_busy.hip).
 * No counterpart in the reference (Python objects; benchmark_results/bench_fft.py:10-22 starts a process per sequence). */
void rafft_alloc_counters(unsigned long long out[5]);

/* The same, asynchronously - continuous batching.  rafft_fold_submit() copies the sequences, queues the batch and
 * returns at once; rafft_fold_wait() blocks until that batch is done and hands over its result (then the job
 * handle is gone).  One library thread drives all batches in flight: the last folding steps of a batch - which only
 * its longest sequences still need and which leave the GPU nearly idle - run beside the busy first steps of the
 * next one.  rafft_fold_batch() is submit + wait.  The analogue in the reference is the process pool of
 * benchmark_results/bench_fft.py:17-21, which also keeps several folds in flight.  Batches complete in any order;
 * every job must be waited for exactly once. */
typedef struct rafft_job rafft_job;
int rafft_fold_submit(const rafft_params *p, int n_seq, const char *const *seqs, const int *lens, int device,
                      rafft_job **job);
int rafft_fold_wait(rafft_job *job, rafft_result **out);

/* Thread-local message of the last failing call. */
const char *rafft_last_error(void);

/* Replaces: RNA.fold_compound(seq, md).eval_structure(db), the ViennaRNA call of
 * rafft/utils.py:135-138 (also benchmark_results/scoring.py:125).  Evaluated on the
 * GPU with the same device functions the fold kernels use. */
int rafft_eval_structure(const char *seq, const char *db, int *dcal_out);
int rafft_eval_structures(int n, const char *const *seqs, const char *const *dbs, int *dcal_out,
                          int *status_out);
/* the same at md.temperature = temp (rafft/utils.py:18) */
int rafft_eval_structures_at(double temp, int n, const char *const *seqs, const char *const *dbs, int *dcal_out,
                             int *status_out);

/* The same at 37 C, and for every structure whether its energy reads an entry of the built-in interior-loop tables (1x1, 2x1, 2x2,
 * the interior mismatches, bulge / interior sizes) that no reference-held (sequence, structure, energy) row exercises - a rule or
 * model value, right in ~9 of 10 cases: guessed_out[i] = 1.  Always 0 with a loaded parameter file.  No
 * counterpart in the reference, whose ViennaRNA has the real tables (rafft/utils.py:135-138). */
int rafft_eval_structures_info(int n, const char *const *seqs, const char *const *dbs, int *dcal_out, int *status_out,
                               int *guessed_out);
/* counts[0..2] = entries of the current 1x1 / 2x1 / 2x2 tables that are such rule / model values (0 with a loaded file) */
int rafft_params_unpinned(int counts[3]);

/* Energy parameters.  Replaces: the parameter set behind RNA.md() / RNA.fold_compound(sequence, md)
 * (rafft/utils.py:17-21) - ViennaRNA's compiled-in Turner 2004 set, or whatever the user loaded with
 * RNA.params_load(), rescaled to md.temperature.  rafft_load_params() reads the file format ViennaRNA 2.x reads and
 * writes ("## RNAfold parameter file v2.0": misc/rna_turner2004.par, RNA.params_save()), so ViennaRNA is touched
 * once, up front, for the tables and never inside the fold.  Without it the built-in 37 C tables are used
 * (DESIGN.md section 2 says how those are pinned).  Loading, inspecting and saving need no GPU; the device tables
 * are rebuilt by the next fold/eval call.  Not thread-safe against a fold running in another thread of the process
 * beyond the library's own lock (calls are serialised). */
int rafft_load_params(const char *path);
int rafft_load_params_text(const char *text, const char *source_name);
int rafft_reset_params(void);                                   /* back to the built-in tables */
int rafft_save_params(const char *path);                        /* counterpart of RNA.params_save(path) */
int rafft_params_info(char *source, int source_cap, int *has_enthalpies);
/* one entry of the current set: ViennaRNA table name ("stack", "int21", "mismatch_multi", "ml_closing", ...),
 * 37 C value or enthalpy, flat row-major index in ViennaRNA's array shape (pair axes 0..7, base axes 0..4) */
int rafft_param_value(const char *table, int enthalpy, long index, int *value_out);

/* Kernel-level seam for parity tests; replaces create_childs' search part:
 * auto_cor (rafft/utils.py:125-132) + ranking (rafft/rafft.py:117-118,92) +
 * window_slide (rafft/rafft.py:36-83) + the energy filter/sort of
 * find_best_consecutives (rafft/rafft.py:86-109) for ONE unpaired region `pos[0..n)`
 * of the structure `db`.  Output arrays must hold min(nb_mode, 2n-1) entries.
 * RAFFT_ERR_PARAM when the region's loop has more than 4095 branch helices. */
int rafft_expand_node(const rafft_params *p, const char *seq, const char *db, const int *pos, int n,
                      int *n_ranked, int *lag, double *corval, int *nb, int *mi, int *mj,
                      double *score, int *ddcal, int *n_kept, int *kept);

int rafft_get_stats(rafft_stats *out);

/* Kinetics on the fast-folding graph (the "next" row 8f-2).  Replaces: get_connected_prev + get_transition_mat,
 * rafft/rafft_kin.py:48-56,68-91 - the O(steps * ms^2 * L) pair-set inclusion search and the Metropolis rate matrix.
 * Input: the graph as the fold returns it (n_steps beams, `rows` = all their dot-brackets back to back, L bytes each,
 * no terminator), `uid[r]` = index of row r in the list of unique structures in order of first appearance
 * (rafft_kin.py:106-112), `energy[u]` = energy of unique structure u, kt = 0.61 in the reference.
 * Output: the dense n_unique x n_unique rate matrix (row-major doubles, diagonal = -row sum) in DEVICE memory
 * `rate_device` (HIP pointer of the caller, e.g. a torch tensor's data_ptr) - at ms=1000 it has 10^8 entries and goes
 * straight into the dense solver. */
int rafft_kin_rate_matrix(int n_steps, const int *step_size, int L, const char *rows, const int *uid, int n_unique,
                          const double *energy, double kt, double *rate_device);

/* The kinetics of a whole batch of fast-folding graphs in one call.  Replaces, per graph: get_connected_prev +
 * get_transition_mat + kinetics, rafft/rafft_kin.py:48-56,68-150 - which rows are the same structure (rafft_kin.py:106-112), the
 * Metropolis rate matrix, and the populations p(t) of dp/dt = rate^T p with everything on unique structure 0 at t = 0 (the
 * reference's default initial population).  Where the reference solves with eig/inv - numerically wrong on its own example - this
 * integrates with TR-BDF2, `m[k]` sub-steps of `h[k]` from times[k-1] (0 for k = 0) to times[k]; the caller computes the schedule
 * (rafft_amd.rafft_kin.kinetics_schedule), so m[k] * h[k] = times[k] - times[k-1].  The generator has non-negative off-diagonals and
 * zero column sums, so every stage matrix is strictly column-diagonally dominant and is inverted without pivoting.
 * Built for many small graphs: one with more than RAFFT_KIN_BATCH_MAX_STATES unique structures gets RAFFT_ERR_CAPACITY and goes
 * through rafft_kin_rate_matrix and a solver of the caller's instead (its matrix and the inverse would no longer stay in the L2:
 * 2 x 8 MB at 1024 states).
 * Per graph g, in the shape of rafft_score_rows: lens[g] positions; n_steps[g] beams of step_size[g][i] rows; rows[g] = the rows
 * of all its steps, row_stride[g] bytes apart (lens[g] back to back, lens[g] + 1 for rafft_seq_result.db, taken from where the fold left
 * them: the host packs them once for the upload); energy[g][row] = the energy the caller chose for each row (the first appearance of a structure counts, rafft_kin.py:115).
 * kt = 0.61 in the reference.  times: n_times ascending positive sample times.  workspace_bytes: device memory for the matrices of
 * the graphs solved together (0: the default, 512 MiB); graphs are processed in chunks that fit, one graph at least.
 * Outputs (host): graph_out[g]; uid_out[row0 + r] = index of row r in the list of the graph's unique structures in order of first
 * appearance; first_row_out[row0 + u] = row (numbered inside the graph) where unique structure u first appears, -1 beyond
 * n_unique; pop_out + n_times * row0 = n_times rows of n_unique doubles, each normalised to sum 1 (the caller sizes uid_out and
 * first_row_out for the rows of all graphs, pop_out for n_times times as many); rate_out (may be NULL, and so may rate_out[g]) =
 * per graph a host buffer for the n_unique x n_unique row-major rate matrix, diagonal = -row sum.
 * Same input, same bits: every sum has a fixed order, and a graph's results do not depend on the rest of the batch.
 * A malformed row (RAFFT_ERR_STRUCT) or too many unique structures (RAFFT_ERR_CAPACITY) is an error of that graph only - the call
 * returns RAFFT_OK, rafft_last_error() names the first such graph, the graph's uid_out / first_row_out are -1 and its populations 0.
 * RAFFT_ERR_PARAM, before anything is launched: a null argument, a negative count, a length above 32767, a stride below the
 * length, times that do not ascend from above 0, kt, m[k] or h[k] not positive. */
#define RAFFT_KIN_BATCH_MAX_STATES 1024
typedef struct {
    int32_t status;
    int32_t n_rows;      /* rows over all steps */
    int32_t row0;        /* index of the graph's first row in uid_out / first_row_out; its populations start at n_times * row0 */
    int32_t n_unique;    /* unique structures (also set with RAFFT_ERR_CAPACITY) */
    int32_t n_edges;     /* non-zero off-diagonal rates */
    int32_t _pad;
} rafft_kin_graph;       /* 24 bytes */
int rafft_kin_batch(int n_graphs, const int *lens, const int *n_steps, const int *const *step_size, const char *const *rows,
                    const int *row_stride, const double *const *energy, double kt, int n_times, const double *times, const int *m,
                    const double *h, long long workspace_bytes, rafft_kin_graph *graph_out, int *uid_out, int *first_row_out,
                    double *pop_out, double *const *rate_out);

/* Folding landscape of a fast-folding graph.  Replaces the arithmetic of utility/surface.py; the drawing
 * stays in Python.  All matrices live in DEVICE memory of the caller (HIP pointers, e.g. a torch tensor's data_ptr); the
 * caller's own stream must be done with them.  Same input, same bits: every floating-point sum has a fixed order.
 *
 * rafft_landscape_distances - get_distance_matrix, surface.py:19-26.  `rows` = n dot-bracket rows of L bytes back to back
 * (host; the unique structures of the graph, surface.py:29-40).  Output: the n x n base-pair distances, row-major 16-bit
 * unsigned, zero diagonal: |A| + |B| - 2 |A n B|, the number of pairs in exactly one of the two structures (at most L).
 * RAFFT_ERR_STRUCT for a malformed row, RAFFT_ERR_PARAM for n < 1 or L > 32767. */
int rafft_landscape_distances(int n, int L, const char *rows, uint16_t *dist_device);
/* rafft_landscape_mds - manifold.MDS(n_components=2, dissimilarity="precomputed").fit_transform, surface.py:98-101: metric
 * SMACOF as sklearn.manifold._mds._smacof_single runs it (unnormalised stress), for n_init independent starts at once.
 * x_init (host): n_init initial configurations of n x 2 doubles - the caller draws them, so the call is a deterministic
 * function of its inputs.  A start stops after the first iteration >= 2 whose relative stress decrease is below eps, or
 * after max_iter; the decision is taken on the device, the host looks at it every 64 iterations.  Output: x_device
 * (n_init x n x 2 doubles, device), stress_out / n_iter_out (host, per start).  Two components only. */
int rafft_landscape_mds(int n, const uint16_t *dist_device, int n_init, const double *x_init, int max_iter, double eps,
                        double *x_device, double *stress_out, int *n_iter_out);
/* rafft_landscape_surface - interpolate.Rbf(x, y, e, function="thin_plate") and its evaluation on meshgrid(ti, ti),
 * ti = linspace(lo, hi, grid), surface.py:107-111; phi(r) = r^2 log r, phi(0) = 0.  x_device: n x 2 positions.
 * phi_device != NULL: the n x n system matrix phi(||X_i - X_j||) is written there (solve it for the weights with the dense
 * solver of your choice).  z_device != NULL: z[gy][gx] = sum_k w_device[k] phi(||(ti[gx], ti[gy]) - X_k||), grid x grid
 * doubles.  Either may be NULL. */
int rafft_landscape_surface(int n, const double *x_device, const double *w_device, int grid, double lo, double hi,
                            double *z_device, double *phi_device);
/* out[0..3] = MDS calls, SMACOF passes enqueued, host read-backs of the per-start `done` words, passes of the last call */
int rafft_landscape_counters(long long out[4]);

/* Accuracy of predicted structures against known ones.  Both entry points replace test_one_seq,
 * benchmark_results/scoring.py:76-94: one RNAstructure `scorer` process per structure of a beam (PPV and sensitivity with one
 * position of slip: a pair (i,j) is found when the other structure holds (i,j), (i+-1,j) or (i,j+-1)), then the last structure
 * that reaches the highest PPV (`>=`), or the first structure with --one.  Integer counts come back; the caller forms
 * PPV = 100 hit_pred / n_pred and sensitivity = 100 hit_known / n_known (0 when the denominator is 0, scoring.py:70-72), and
 * ViennaRNA's bp_distance to the known structure is n_pred + n_known - 2 n_exact. */
typedef struct {
    int32_t n_pred;      /* pairs of the predicted row */
    int32_t hit_pred;    /* ... found in the known structure */
    int32_t hit_known;   /* pairs of the known structure found in the predicted row */
    int32_t n_exact;     /* pairs in both, no slip */
    int32_t status;      /* RAFFT_ERR_STRUCT: the row holds something else than ( ) . or is unbalanced (counts are 0) */
} rafft_score_row;       /* 20 bytes */

typedef struct {
    int32_t status;      /* RAFFT_ERR_STRUCT: malformed known structure or one of another length than the sequence (see
                            rafft_last_error() for the position); rafft_score_result: the fold's status when it failed */
    int32_t n_known;     /* pairs of the known structure */
    int32_t n_rows;
    int32_t row0;        /* index of the sequence's first record in row_out */
    int32_t pick_ppv;    /* last row with the highest PPV among the rows that parsed (PPVs compared as integer fractions, a row
                            without pairs counts as 0; a beam without any hit picks its last row); -1 when there is none */
    int32_t pick_first;  /* 0 (--one), or -1 for a sequence without rows */
    rafft_score_row best;    /* the record of row pick_ppv */
    rafft_score_row first;   /* the record of row 0 */
} rafft_score_seq;       /* 64 bytes */

/* rows[s]: the n_rows[s] dot-bracket rows of sequence s, lens[s] characters each (( ) . only), row_stride[s] bytes apart
 * (lens[s] for rows back to back, lens[s] + 1 for rafft_seq_result.db).  known[s]: the known structure, NUL terminated, lens[s]
 * characters of ( ) < > [ ] . read as rafft/utils.py:53-67 reads them (two stacks: ( and < share one, [ has its own).
 * row_out (may be NULL): one record per row, sequence after sequence in input order; seq_out: one record per sequence.
 * A malformed row or known structure is an error of that row / sequence only: the call still returns RAFFT_OK.
 * RAFFT_ERR_PARAM: n_seq < 0, a length above 32767, a negative count, a stride below the length. */
int rafft_score_rows(int n_seq, const int *lens, const int *n_rows, const char *const *rows, const int *row_stride,
                     const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out);
/* The same for the final beam of every sequence of a fold result, read where the fold left it (the result's pinned rows go
 * to the device as they lie, no repacking).  known[s] as above, one per sequence of `r`.  A sequence whose fold failed keeps
 * that status and has no rows.  row_out (may be NULL) holds the sum of the final beams' sizes. */
int rafft_score_result(const rafft_result *r, const char *const *known, rafft_score_row *row_out, rafft_score_seq *seq_out);

/* Minimum-free-energy structures of a batch.  Replaces: RNA.fold(seq), benchmark_results/src/vrna_mfe.py:25,
 * which benchmark_results/bench_mfe.py:11-15 runs with one process per sequence to make the comparison column mfe_scores.csv.
 * RNA.fold's defaults are dangles=2, lonely pairs allowed and interior loops of up to 30 unpaired positions; so is this: Zuker's
 * recurrences in integer dcal over the loop energies rafft_eval_structure uses, hence dcal = the minimum of rafft_eval_structure
 * over all structures with canonical pairs, hairpins of at least 3 and interior loops of at most 30, and rafft_eval_structure of
 * the returned row gives dcal again.  Among structures of equal energy the traceback's fixed candidate order decides: the row is a
 * function of the sequence and the energy tables alone - not of the batch, its order, the size class or the workspace.
 * Sequences of up to rafft_mfe_lds_len() nt keep their tables in LDS, one workgroup each; longer ones (up to RAFFT_MFE_MAX_LEN)
 * have 3 x L x L int32 tables in device memory and are processed in chunks that fit workspace_bytes (0: 512 MiB; one sequence at
 * least - 192 MiB at 4096 nt).  max_lds_len: 0 for the library's bound; a lower value sends shorter sequences through the
 * device-memory class as well (tests, measurements).  temp as in rafft_params.
 * Outputs (host): seq_out[s]; db_out[s] = lens[s] + 1 bytes for the NUL-terminated dot-bracket row.
 * RAFFT_ERR_BAD_CHAR, RAFFT_ERR_EMPTY and RAFFT_ERR_TOO_LONG (above RAFFT_MFE_MAX_LEN) are errors of that sequence only: its row
 * is all dots, the call returns RAFFT_OK and rafft_last_error() names the first such sequence.  RAFFT_ERR_PARAM, before anything
 * is launched: a null argument, a negative count, max_lds_len above rafft_mfe_lds_len().  RAFFT_ERR_TEMP as for the fold. */
#define RAFFT_MFE_MAX_LEN 4096
typedef struct {
    int32_t status;
    int32_t length;
    int32_t dcal;        /* minimum free energy in dcal/mol (<= 0: the open chain has 0) */
    int32_t n_pairs;     /* pairs of the row */
} rafft_mfe_seq;         /* 16 bytes */
int rafft_mfe_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                    int max_lds_len,            /* 0: the library's bound; lower values route shorter sequences through the HBM class (tests, measurements) */
                    long long workspace_bytes,  /* 0: 512 MiB */
                    rafft_mfe_seq *seq_out, char *const *db_out /* db_out[s]: lens[s] + 1 bytes, NUL terminated */);
/* the longest sequence whose tables fit the LDS class */
int rafft_mfe_lds_len(void);

/* Minimum-free-energy structures under a maximum base-pair span, for sequences of up to RAFFT_MFE_SPAN_MAX_LEN nt (DESIGN.md
 * section 18; what `RNAfold --maxBPspan` is used for).  A pair (i, j), i < j, is allowed iff j - i + 1 <= max_span; everything
 * else is rafft_mfe_batch's ensemble and energy, and the exterior loop is not restricted.  dcal is the minimum of
 * rafft_eval_structure over that ensemble and rafft_eval_structure of the returned row gives dcal again.  The candidate order of
 * the traceback is rafft_mfe_batch's, the exterior stems that end at j being visited with i ascending from
 * max(0, j - max_span + 1): a sequence with lens[s] <= max_span gets the row, dcal and n_pairs of rafft_mfe_batch byte for byte.
 * max_span of 1 to 4 gives the open chain.  The result is a function of the sequence, the energy tables, temp and max_span alone.
 * The work is O(L W^2), W = min(max_span, L), in W launches of up to L cells; a sequence has 4 x L x W int32 tables in device
 * memory (75 MiB at 32768 nt and span 150) and sequences are processed in chunks that fit workspace_bytes (0: 512 MiB; one
 * sequence at least).
 * Outputs and the errors of a sequence (RAFFT_ERR_TOO_LONG: above RAFFT_MFE_SPAN_MAX_LEN) as rafft_mfe_batch.  RAFFT_ERR_PARAM,
 * before anything is launched: a null argument, a negative count or workspace, max_span outside 1 .. RAFFT_MFE_MAX_LEN.
 * RAFFT_ERR_TEMP as for the fold. */
#define RAFFT_MFE_SPAN_MAX_LEN RAFFT_MAX_LEN
int rafft_mfe_span_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                         int max_span,               /* 1 .. RAFFT_MFE_MAX_LEN */
                         long long workspace_bytes,  /* 0: 512 MiB; one sequence at least */
                         rafft_mfe_seq *seq_out, char *const *db_out /* db_out[s]: lens[s] + 1 bytes, NUL terminated */);

/* Minimum-free-energy structures under hard constraints and soft terms (what `RNAfold -C
 * --enforceConstraint` and `RNAfold --shape` are used for), for the two size classes of rafft_mfe_batch.  Every sequence may carry
 * any of three inputs; an absent one (a null array, a null entry) is neutral.
 * constraints[s]: a NUL-terminated string of lens[s] characters, all of them enforced:
 *     .  nothing            x  unpaired            |  paired, any partner
 *     <  paired with a partner downstream (the 5' end of its pair)       >  paired with a partner upstream
 *     ( ) matched brackets: this pair is in the structure
 * The ensemble is exactly the set of structures of rafft_mfe_batch (canonical pairs, hairpins of at least 3, interior loops of at
 * most 30) that satisfy every character.
 * soft_unpaired[s] (u) and soft_stack[s] (b): lens[s] values in dcal each, |value| <= RAFFT_MFE_SOFT_MAX.  u[k] is added for every
 * unpaired position k; b follows the Deigan convention: a pair (i,j) stacked directly on (i+1,j-1) adds b[i] + b[j] + b[i+1] + b[j-1].
 * With up(k): constraints[k] is . or x; free(a,b): up on all of a..b (the empty range is free); U(a,b) = u[a] + .. + u[b];
 * ok(i,j): canonical, j - i - 1 >= 3, constraints[i] one of . | < or a ( whose partner is j, constraints[j] one of . | > or a )
 * whose partner is i - the recurrences of rafft_mfe_batch become (a cell with !ok(i,j) has C = no structure):
 *     C[i][j]:  the hairpin only if free(i+1,j-1), plus U(i+1,j-1); an interior loop with (p,q) only if free(i+1,p-1) and
 *               free(q+1,j-1), plus both U terms, plus the stack term when p = i+1 and q = j-1; the multiloop term unchanged
 *     M1[i][j] = min(C[i][j] + stem, M1[i][j-1] + ml_base + u[j] if up(j))
 *     M[i][j]  = min(M1[i][j], M[i+1][j] + ml_base + u[i] if up(i), splits)
 *     F[j]     = min(F[j-1] + u[j] if up(j), stems),  F[-1] = 0
 * A pair that crosses a forced pair needs no test: one end of the forced pair lies inside it and can neither pair nor stay unpaired.
 * dcal is the minimum of rafft_eval_structure(row) + soft terms(row) over the ensemble and may be positive; pseudo_dcal is the soft
 * part of dcal for the returned row, so rafft_eval_structure(row) == dcal - pseudo_dcal.  The traceback's candidate order is
 * rafft_mfe_batch's; a candidate the constraints remove is not a candidate.  A sequence without any constraint, or with an all-'.'
 * string and zero arrays, gets the row, dcal and n_pairs of rafft_mfe_batch byte for byte, and the result of a sequence is a
 * function of the sequence, its constraints, the energy tables and temp - not of the batch, its order, the size class or the chunks.
 * Size classes, max_lds_len, workspace_bytes, outputs and the errors of a sequence as rafft_mfe_batch.  Errors of that sequence
 * only as well (all-dot row, the call returns RAFFT_OK, rafft_last_error() names the first): RAFFT_ERR_STRUCT, found on the host - a
 * string of another length than the sequence, a character outside the seven, unbalanced brackets, a bracket pair that is not
 * canonical or encloses fewer than 3 positions; RAFFT_ERR_INFEASIBLE - no structure satisfies the constraints.  RAFFT_ERR_PARAM,
 * before anything is launched: as rafft_mfe_batch, and a soft value beyond RAFFT_MFE_SOFT_MAX (at 4096 nt a position counts once in
 * u or at most twice in b: 4096 x 2 x 20000 = 1.6e8 stays below the 5e8 guard of section 9).  RAFFT_ERR_TEMP as for the fold. */
#define RAFFT_MFE_SOFT_MAX 20000
typedef struct {
    int32_t status;
    int32_t length;
    int32_t dcal;        /* the objective: loop energies plus soft terms of the row, in dcal/mol */
    int32_t n_pairs;     /* pairs of the row */
    int32_t pseudo_dcal; /* the soft terms of the row */
    int32_t _pad;
} rafft_mfe_con_seq;     /* 24 bytes */
int rafft_mfe_constrained_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                                const char *const *constraints,      /* may be NULL; entries may be NULL */
                                const int32_t *const *soft_unpaired, /* may be NULL; entries may be NULL; lens[s] dcal values */
                                const int32_t *const *soft_stack,    /* the same */
                                int max_lds_len,            /* as rafft_mfe_batch */
                                long long workspace_bytes,  /* 0: 512 MiB */
                                rafft_mfe_con_seq *seq_out, char *const *db_out /* db_out[s]: lens[s] + 1 bytes, NUL terminated */);

/* Minimum-free-energy folds of two-strand dimers: what RNAcofold's MFE answers - a miRNA and its target, an
 * antisense oligo, a probe, a primer dimer.  seqs[s] is the concatenation S = A B of the two strands, no separator, lens[s] = L =
 * La + Lb <= RAFFT_MFE_MAX_LEN, cuts[s] = c = La: position c is the first base of B, the nick is the missing backbone bond between
 * c-1 and c.  cuts == NULL or cuts[s] == 0: a single strand, which gets the row, dcal and n_pairs of rafft_mfe_batch byte for byte.
 * Ensemble: canonical, non-crossing pairs; a pair (i,j) with both ends on one strand needs j - i - 1 >= 3, a pair with i < c <= j
 * any j - i >= 1; real interior loops have at most 30 unpaired positions, as in rafft_mfe_batch.
 * Energy of a structure: the nick lies in exactly one loop - the exterior loop if no pair spans the nick, else the loop closed by the
 * innermost spanning pair.  Every loop that does not hold the nick has the energy rafft_eval_structure gives it.  The loop that holds
 * the nick and the exterior loop are both scored as exterior loops: 0 for unpaired positions and e_stem(.., ext = true) for every
 * stem in them (dangles=2), the pair that closes the nick loop read from inside - its reversed type with neighbours S[j-1], S[i+1].
 * A neighbour across a strand end does not exist: the 5' neighbour of p exists iff p > 0 && p != c, the 3' neighbour of q iff
 * q < L-1 && q + 1 != c.  duplex_init is added once iff at least one pair spans the nick.  There is no symmetry correction for
 * A == B (RNAcofold's MFE has none either).
 * duplex_init is the loaded parameter file's DuplexInit, scaled with its enthalpy to temp like every other scalar; with the built-in
 * tables Turner 2004's 410 dcal at 37 C.  rafft_cofold_duplex_init returns the value in force (RAFFT_ERR_TEMP as for the fold).
 * The row is traced in one fixed, documented order (section 22) and is a function of A, B, the tables and temp - not of the batch,
 * its order, the size class or the chunks.  n_inter is the number of pairs of the row that span the nick.
 * Size classes, max_lds_len, workspace_bytes and every error as rafft_mfe_batch; a cuts[s] outside 0 .. lens[s]-1 is
 * RAFFT_ERR_STRUCT of that sequence only, found on the host (all-dot row, the call returns RAFFT_OK).
 * Not here: the dimer partition function and concentrations, constraints, SHAPE or a span with a cut, more than two strands. */
typedef struct {
    int32_t status;
    int32_t length;
    int32_t dcal;        /* the minimum free energy of the dimer in dcal/mol, duplex_init included when n_inter > 0 */
    int32_t n_pairs;     /* pairs of the row */
    int32_t cut;         /* the cut the sequence was folded with (0: a single strand, and for a sequence with an error) */
    int32_t n_inter;     /* pairs of the row that span the nick */
} rafft_cofold_seq;      /* 24 bytes */
int rafft_cofold_batch(int n_seq, const char *const *seqs /* A then B, no separator */, const int *lens, const int *cuts /* may be NULL */,
                       double temp, int max_lds_len /* as rafft_mfe_batch */, long long workspace_bytes /* 0: 512 MiB */,
                       rafft_cofold_seq *seq_out, char *const *db_out /* db_out[s]: lens[s] + 1 bytes, NUL terminated, no separator */);
int rafft_cofold_duplex_init(double temp, int *dcal_out);

/* Partition function, base-pair probabilities and centroid structures of a batch (McCaskill).  Replaces:
 * RNA.fold_compound(seq, md).pf() / bpp(), the calls beside the RNA.fold of benchmark_results/src/vrna_mfe.py:25.
 * The ensemble is the one rafft_mfe_batch minimises over: canonical pairs, hairpins of at least 3, interior loops of at most 30
 * unpaired positions, lonely pairs allowed, dangles=2.  The weight of a structure is exp(-dcal / (100 kT)), dcal the integer
 * rafft_eval_structure returns for it, kT = (temp + 273.15) * 1.98717e-3 kcal/mol.  Z is the sum of these weights over every
 * structure of the ensemble, P(i,j) the weight share of the structures that hold the pair (i,j), and the centroid row holds every
 * pair with P > 0.5 (such pairs cannot cross or share a base).
 * The sums are scaled fp64: the call first runs the MFE path on the same sequences and divides every table cell by
 * scale^(positions it covers), scale = exp(-scale_factor * (mfe_dcal / 100) / (kT * length)), as ViennaRNA's pf_scale with sfact
 * 1.07.  The results do not depend on scale_factor beyond rounding; a sequence's bits depend on the sequence, the energy tables,
 * temp and scale_factor only - not on the batch, its order or the workspace.
 * Every sequence has six L x L fp64 tables in device memory; the batch is processed in chunks of whole sequences, in input order,
 * that fit workspace_bytes (0: 512 MiB; one sequence at least - 768 MiB at 4096 nt).
 * Outputs (host): seq_out[s]; db_out[s] = lens[s] + 1 bytes for the NUL-terminated centroid row; prob_out may be NULL and so may
 * prob_out[s], else lens[s] x lens[s] doubles, row-major, P(i pairs j) at [i][j] for i < j and 0 elsewhere.
 * RAFFT_ERR_BAD_CHAR, RAFFT_ERR_EMPTY and RAFFT_ERR_TOO_LONG (above RAFFT_PF_MAX_LEN) are errors of that sequence only: its row is
 * all dots, its energy and its probabilities are 0, the call returns RAFFT_OK and rafft_last_error() names the first such sequence.
 * So is RAFFT_ERR_CAPACITY: the scaled tables of that sequence left the fp64 range (its exterior sum is zero or not finite, or a
 * probability is not finite) - never a silent inf or nan.  RAFFT_ERR_PARAM, before anything is launched: a null argument, a
 * negative count, a scale_factor that is negative or not finite.  RAFFT_ERR_TEMP as for the fold. */
#define RAFFT_PF_MAX_LEN RAFFT_MFE_MAX_LEN
typedef struct {
    int32_t status;
    int32_t length;
    int32_t mfe_dcal;      /* the MFE the scale was taken from (what rafft_mfe_batch returns) */
    int32_t n_pairs;       /* pairs of the centroid row */
    double  energy;        /* ensemble free energy -kT ln Z, kcal/mol */
    double  mfe_frequency; /* exp((energy - mfe_dcal/100) / kT): share of the MFE structure in the ensemble */
} rafft_pf_seq;            /* 32 bytes */
int rafft_pf_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                   double scale_factor,        /* 0: 1.07; tests pass other values */
                   long long workspace_bytes,  /* 0: 512 MiB; one sequence at least */
                   rafft_pf_seq *seq_out,
                   char *const *db_out,        /* db_out[s]: lens[s]+1 bytes, the centroid row, NUL terminated */
                   double *const *prob_out     /* may be NULL, and so may prob_out[s]: lens[s] x lens[s] doubles, row-major,
                                                  P(i pairs j) at [i][j] for i < j, 0 elsewhere */);

/* Partition function, base-pair probabilities, centroid and unpaired probabilities under hard constraints and soft terms (DESIGN.md
 * section 21; what `RNAfold -p -C --enforceConstraint` and `RNAfold -p --shape` are used for): how sure each pair is given what is
 * known, and the modelled accessibility to set beside a probe.  constraints, soft_unpaired (u) and soft_stack (b) are those of
 * rafft_mfe_constrained_batch, an absent one neutral; scale_factor, workspace_bytes, seq_out, db_out and prob_out those of
 * rafft_pf_batch.
 * The ensemble is the one rafft_mfe_constrained_batch minimises over: every one of the seven characters is enforced.  The weight of
 * a structure is exp(-(rafft_eval_structure(row) + soft(row)) / (100 kT)), soft = u[k] for every unpaired position k plus Deigan's
 * b[i] + b[j] + b[i+1] + b[j-1] for every pair (i,j) stacked directly on (i+1,j-1); |value| <= RAFFT_MFE_SOFT_MAX.
 * With w(e) = exp(-e / (100 kT)), b = w(ml_base) and ok, up, free, U, stack of rafft_mfe_constrained_batch, the sums of
 * rafft_pf_batch become:
 *     C[i][j]    0 unless ok(i,j); the hairpin only if free(i+1,j-1): w(hairpin + U(i+1,j-1)); an interior loop with (p,q) only if
 *                free(i+1,p-1) and free(q+1,j-1): w(interior + both U + stack when p = i+1, q = j-1) C[p][q]; the multiloop term unchanged
 *     M1[i][j]   = C[i][j] w(stem) + [up(j)] M1[i][j-1] b w(u[j])
 *     M[i][j]    = sum_{k=i..j} ([free(i,k-1)] b^(k-i) w(U(i,k-1)) + M[i][k-1]) M1[k][j]
 *     F[j]       = [up(j)] F[j-1] w(u[j]) + sum_i F[i-1] C[i][j] w(stem_ext);  Fr the same from the 3' end
 *     Mo         unchanged
 *     M1o[k][j]  = [up(j+1)] b w(u[j+1]) M1o[k][j+1] + (the Co term, unchanged) + sum_{i<=k} Mo[i][j] ([free(i,k-1)] b^(k-i) w(U(i,k-1)) + M[i][k-1])
 *     Co[i][j]   0 unless ok(i,j) - a weight there would leak into the pairs inside a removed pair; else F[i-1] w(stem_ext) Fr[j+1]
 *                + sum over enclosing (p,q) with free(p+1,i-1) and free(j+1,q-1) of Co[p][q] w(interior + soft) + w(stem) M1o[i][j]
 *     P(i,j)     = C[i][j] Co[i][j] / Z;   unpaired[k] = 1 - sum_j P(k,j) - sum_i P(i,k)
 * A pair that every structure holds has P = 1 up to rounding; under constraints a P above 1 is returned as 1.0.
 * Outputs: seq_out[s].mfe_dcal is the constrained objective (dcal of rafft_mfe_constrained_batch; the call runs that fold first and
 * takes the scale from it), energy = -kT ln Z, mfe_frequency the share of that optimum.  The centroid row holds every pair with
 * P > 0.5; it need NOT satisfy a `|` (a position that must pair may have no partner above one half).  unpaired_out may be NULL and
 * so may unpaired_out[s], else lens[s] doubles, each summed in an order that lens[s] fixes.  rafft_mea_probs_batch over prob_out is
 * the MEA row under the data.
 * Errors of a sequence (all-dot row, zeros, the call returns RAFFT_OK): those of rafft_pf_batch and of
 * rafft_mfe_constrained_batch - RAFFT_ERR_STRUCT, found on the host; RAFFT_ERR_INFEASIBLE, from the MFE front: such a sequence takes
 * no part in the sums.  Soft terms far from physical values can push the scaled sums out of the fp64 range: RAFFT_ERR_CAPACITY for
 * that sequence, never a silent inf or nan.  RAFFT_ERR_PARAM, before anything is launched: the cases of both calls.
 * A sequence with no constraint, or with an all-'.' string and zero arrays, gets the bits of rafft_pf_batch - energy, share, every P
 * and the row; a sequence's bits depend on the sequence, its constraints, the energy tables, temp and scale_factor - not on the
 * batch, its order or the workspace. */
int rafft_pf_constrained_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                               const char *const *constraints,      /* as rafft_mfe_constrained_batch */
                               const int32_t *const *soft_unpaired,
                               const int32_t *const *soft_stack,
                               double scale_factor,        /* as rafft_pf_batch */
                               long long workspace_bytes,
                               rafft_pf_seq *seq_out, char *const *db_out, double *const *prob_out,
                               double *const *unpaired_out /* may be NULL, entries may be NULL: lens[s] doubles */);

/* Partition function, base-pair probabilities, centroid and unpaired probabilities under a maximum base-pair span, for sequences
 * of up to RAFFT_MFE_SPAN_MAX_LEN nt (what `RNAfold -p --maxBPspan` and `RNAplfold -L` are used for on long
 * RNAs).  The ensemble is rafft_pf_batch's restricted to the structures whose pairs (i, j), i < j, all have j - i + 1 <= max_span;
 * the exterior loop is not restricted.  Weights, kT and dangles=2 are rafft_pf_batch's.  Z is the sum of the weights over that
 * ensemble, P(i,j) the weight share of its structures that hold (i,j), energy = -kT ln Z, the centroid row holds the pairs with
 * P > 0.5, mfe_dcal is what rafft_mfe_span_batch returns for the same max_span (the call runs it first; the scale comes from it)
 * and mfe_frequency = exp((energy - mfe_dcal/100) / kT).  unpaired[i] = 1 - sum_j P(i,j) - sum_h P(h,i), clamped to [0, 1], each
 * position summed in an order that lens[s] and max_span fix.  max_span of 1 to 4 gives the open chain: energy 0, every P 0.
 * Every sequence has six L x W fp64 tables in device memory, W = min(max_span, L): 48 L W + 8 (3 L + 2 W + 6) + 8 (L + 1) + L + 1
 * bytes with its other arrays (226 MiB at 32768 nt and span 150); chunks of whole sequences, in input order, that fit
 * workspace_bytes (0: 512 MiB; one sequence at least).  The band cells are scaled fp64 as rafft_pf_batch's; the exterior sums,
 * which cover the whole sequence, are held as a mantissa and a binary exponent per position, so their range does not limit L.
 * Outputs (host): seq_out[s] and db_out[s] as rafft_pf_batch.  prob_out may be NULL and so may prob_out[s], else it is BANDED:
 * lens[s] x W_s doubles, W_s = min(max_span, lens[s]), P(i, i + d) at [i * W_s + d]; entries with d < 4 or i + d >= lens[s] are
 * 0 (a dense matrix at 32768 nt would be 8 GiB).  unpaired_out may be NULL and so may unpaired_out[s], else lens[s] doubles.
 * Errors of a sequence as rafft_pf_batch (RAFFT_ERR_TOO_LONG: above RAFFT_MFE_SPAN_MAX_LEN; the buffers of such a sequence are
 * not written): its row is all dots, its numbers are 0, its neighbours are untouched, rafft_last_error() names the first such
 * sequence.  RAFFT_ERR_CAPACITY: a band cell left the fp64 range - the mantissa of Z is not finite and positive, Z is below the
 * weight of the MFE structure, or a probability is not finite; heterogeneous sequences at very wide spans can meet it.
 * RAFFT_ERR_PARAM, before anything is launched: a null argument, a negative count or workspace, a scale_factor that is negative
 * or not finite, max_span outside 1 .. RAFFT_MFE_MAX_LEN.  RAFFT_ERR_TEMP as for the fold.  A sequence's bits depend on the
 * sequence, the energy tables, temp, scale_factor and max_span only - not on the batch, its order, the chunks or the workspace. */
int rafft_pf_span_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                        double scale_factor,        /* 0: 1.07 */
                        int max_span,               /* 1 .. RAFFT_MFE_MAX_LEN */
                        long long workspace_bytes,  /* 0: 512 MiB; one sequence at least */
                        rafft_pf_seq *seq_out,
                        char *const *db_out,        /* db_out[s]: lens[s]+1 bytes, the centroid row, NUL terminated */
                        double *const *prob_out,    /* may be NULL, and so may prob_out[s]: lens[s] x W_s doubles, banded */
                        double *const *unpaired_out /* may be NULL, and so may unpaired_out[s]: lens[s] doubles */);

/* Maximum-expected-accuracy (MEA) structures and the ensemble diversity of a batch.  Replaces: what
 * `RNAfold -p --MEA` prints beside the centroid.  rafft_mea_batch is rafft_pf_batch plus the recursion below on the device's own
 * P; rafft_mea_probs_batch runs the same recursion on matrices the caller brings - pair probabilities, or pair frequencies of
 * sampled rows, of a beam, of an energy band (the row is then their consensus structure).
 * Definition, exact - same input, same bits.  For P(i,j), i < j, positions from 0, and gamma > 0 (0 means 1.0):
 *   q_i = max(0, 1 - s_i), s_i the sum of P over the partners of i in ascending partner index; formed once and stored.
 *   W(i,j) = (gamma + gamma) * P(i,j), one rounded multiply, formed once and stored.  (k,j) is a candidate iff P(k,j) > 0.
 *   E[i][j] = 0 for j < i; else the maximum of E[i][j-1] + q_j and, over the candidates (k,j) with i <= k < j, of
 *   (E[i][k-1] + W(k,j)) + E[k+1][j-1] in this association.  mea = E[0][L-1].
 *   The row: intervals from (0, L-1); of (i,j), j is unpaired when E[i][j] == E[i][j-1] + q_j (go on with (i, j-1)), else j pairs
 *   with the first k ascending whose candidate has the bits of E[i][j] (go on with (i, k-1) and (k+1, j-1)).  A cell that nothing
 *   reproduces is RAFFT_ERR_HIP with a message, never a silently wrong row.
 *   diversity = sum over i < j of 2 P(i,j) (1 - P(i,j)): per position the terms of its partners above it in ascending order, then
 *   the positions' sums lane-strided over 64 lanes and a butterfly - an order that depends on the length only.
 * rafft_mea_batch: arguments, chunks, errors of a sequence (RAFFT_ERR_CAPACITY included: all-dot row, zeros, the call returns
 * RAFFT_OK) and RAFFT_ERR_TEMP as rafft_pf_batch; energy, mfe_dcal and prob_out have the bits rafft_pf_batch returns.  P > 0 holds
 * only for canonical pairs with j - i > 3, so the row holds only such pairs; as in ViennaRNA it may hold an interior loop of more
 * than 30 unpaired positions, which the ensemble does not; dcal is what rafft_eval_structure gives for the row.  RAFFT_ERR_PARAM,
 * before anything is launched: rafft_pf_batch's cases and a gamma that is negative or not finite.
 * rafft_mea_probs_batch: prob_in[s] is lens[s] x lens[s] doubles, row-major; only [i][j] with i < j is read.  Four L x L fp64
 * tables a matrix, in chunks of whole matrices that fit workspace_bytes (0: 512 MiB; one matrix at least).  RAFFT_ERR_PARAM, before
 * anything is launched and naming (sequence, i, j) in rafft_last_error(): an entry with i < j that is not finite, below 0, above 1,
 * or non-zero with j - i <= 3; also a null argument, a negative count or workspace_bytes, a gamma that is negative or not finite.
 * Row sums are not checked (frequencies of crossing rows are a legitimate input; q is clamped).  lens[s] <= 0 is RAFFT_ERR_EMPTY
 * and a length above RAFFT_PF_MAX_LEN RAFFT_ERR_TOO_LONG: errors of that matrix only.
 * Both: a sequence's result depends on its own inputs only, not on the batch, its order, the chunks or the workspace.
 * Outputs (host): seq_out[s]; db_out[s] = lens[s] + 1 bytes, the MEA row; unpaired_out may be NULL and so may unpaired_out[s],
 * else lens[s] doubles, q. */
typedef struct {
    int32_t status, length, mfe_dcal, n_pairs;
    int32_t dcal, _pad;          /* energy of the MEA row */
    double  energy;              /* ensemble free energy: the bits rafft_pf_batch returns */
    double  mea, diversity;
} rafft_mea_seq;                 /* 48 bytes */
int rafft_mea_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                    double scale_factor, long long workspace_bytes, double gamma /* 0: 1.0 */,
                    rafft_mea_seq *seq_out, char *const *db_out /* the MEA row */,
                    double *const *prob_out /* may be NULL / hold NULLs */,
                    double *const *unpaired_out /* may be NULL / hold NULLs: lens[s] doubles, q */);
typedef struct { int32_t status, length, n_pairs, _pad; double mea, diversity; } rafft_mea_probs_seq;   /* 32 bytes */
int rafft_mea_probs_batch(int n, const int *lens, const double *const *prob_in /* L x L row-major, [i][j], i<j read */,
                          double gamma, long long workspace_bytes,
                          rafft_mea_probs_seq *seq_out, char *const *db_out, double *const *unpaired_out);

/* Structures drawn from the Boltzmann ensemble of a batch (stochastic traceback).  Replaces:
 * RNA.fold_compound(seq, md).pbacktrack(n) / `RNAsubopt -p n`, what a user of the reference takes from ViennaRNA to compare
 * fast-folding paths with the thermodynamic ensemble.
 * The ensemble, the weights, kT and the scaling are rafft_pf_batch's: row k of sequence s is ONE structure, drawn with probability
 * exp(-dcal / (100 kT)) / Z.  The call runs the MFE path and the inside pass of rafft_pf_batch (three L x L fp64 tables a sequence,
 * in chunks of whole sequences whose tables and whose rows fit workspace_bytes each; one sequence at least) and then walks the
 * tables once per sample; dcal_out[s][k] is the sum of the integer loop energies of the terms the walk picked - rafft_eval_structure
 * of the row gives the same number.  seq_out[s].energy and mfe_dcal have the bits rafft_pf_batch returns.
 * Random numbers: Philox4x32-10 under the key seeds[s], counter (k, number of the choice within the sample) - nothing is stored.
 * Same input, same bits: row k of a sequence depends on the sequence, the energy tables, temp, scale_factor, the sequence's seed
 * and k only - not on the batch, its order, the workspace or n_samples: the first n rows of a call with n_samples = m > n are the
 * rows of a call with n_samples = n.  Two equal sequences with equal seeds get equal rows: give every copy a seed of its own when
 * independent samples are wanted.
 * Outputs (host): seq_out[s]; db_out[s] = n_samples rows, lens[s] + 1 bytes apart, NUL terminated; dcal_out may be NULL and so
 * may dcal_out[s], else n_samples ints.  n_samples = 0 is valid: the records are filled, no row is touched.
 * RAFFT_ERR_BAD_CHAR, RAFFT_ERR_EMPTY, RAFFT_ERR_TOO_LONG (above RAFFT_PF_MAX_LEN) and RAFFT_ERR_CAPACITY (the scaled exterior
 * sum left the fp64 range) are errors of that sequence only: its record has n_samples = 0, its rows are all dots and its dcal 0,
 * the call returns RAFFT_OK and rafft_last_error() names the first such sequence.  RAFFT_ERR_PARAM, before anything is launched:
 * a null seq_out, a null db_out with n_samples > 0, a negative n_seq or n_samples, n_samples above RAFFT_SAMPLE_MAX, a
 * scale_factor that is negative or not finite.  RAFFT_ERR_TEMP as for the fold. */
#define RAFFT_SAMPLE_MAX (1 << 20)
typedef struct {
    int32_t status;      /* as rafft_pf_seq: BAD_CHAR / EMPTY / TOO_LONG / CAPACITY stay with their sequence */
    int32_t length;
    int32_t mfe_dcal;    /* the MFE the scale was taken from */
    int32_t n_samples;   /* rows written: n_samples of the call, or 0 when status != 0 */
    double  energy;      /* ensemble free energy, the same bits rafft_pf_batch returns */
} rafft_sample_seq;      /* 24 bytes */
int rafft_sample_batch(int n_seq, const char *const *seqs, const int *lens, double temp,
                       double scale_factor,        /* 0: 1.07 */
                       long long workspace_bytes,  /* 0: 512 MiB; one sequence at least */
                       int n_samples,
                       const unsigned long long *seeds /* [n_seq]; NULL: all 0 */,
                       rafft_sample_seq *seq_out,
                       char *const *db_out         /* db_out[s]: n_samples rows, lens[s]+1 bytes apart, NUL terminated */,
                       int *const *dcal_out        /* may be NULL and so may dcal_out[s]: n_samples ints */);

/* Every structure of a batch within an energy band above the minimum (Wuchty et al. 1999).  Replaces:
 * `RNAsubopt -e delta -s`, the producer of the file the reference's landscape tool reads with --sub (utility/surface.py:54-63).
 * The ensemble is rafft_mfe_batch's: canonical pairs, hairpins of at least 3, interior loops of at most 30 unpaired positions,
 * lonely pairs allowed, dangles=2.  The number of rows is not known before the call, so the library owns the result, as
 * rafft_fold_batch does: free it with rafft_subopt_free.
 * Completeness and energies: the rows of a sequence are exactly the structures of the ensemble with rafft_eval_structure(row) <=
 * mfe_dcal + delta_dcal, none twice.  dcal[k] is the sum of the integer loop terms the enumeration took - rafft_eval_structure of
 * the row gives the same number.
 * Order: rows are sorted by dcal ascending; among equal energies they come in enumeration order, the left-to-right order of the
 * leaves of the decision tree of DESIGN.md section 12.
 * Same input, same bits: a sequence's rows are a function of the sequence, the energy tables, temp and delta_dcal only - not of
 * the batch, its order, the workspace, the chunking, or max_structs when it is large enough.
 * Capacity: a sequence with more than max_structs structures in the band gets RAFFT_ERR_CAPACITY, no rows, and n_reached; the
 * call still returns RAFFT_OK, its neighbours are unaffected and rafft_last_error() names the first such sequence.  Exactly
 * max_structs structures is not an error.
 * Device memory: every sequence keeps three L x L int32 tables and two buffers of max_structs partial structures (DESIGN.md
 * section 12 states their bytes); sequences are taken in chunks of whole sequences in input order whose tables and whose buffers
 * fit workspace_bytes each, one sequence at least.
 * RAFFT_ERR_BAD_CHAR, RAFFT_ERR_EMPTY and RAFFT_ERR_TOO_LONG (above RAFFT_SUBOPT_MAX_LEN) are errors of that sequence only, as in
 * rafft_mfe_batch: the call returns RAFFT_OK and rafft_last_error() names the first such sequence.  RAFFT_ERR_PARAM, before
 * anything is launched: a null argument, a negative n_seq or workspace_bytes, delta_dcal outside [0, RAFFT_SUBOPT_MAX_DELTA],
 * max_structs outside [1, RAFFT_SUBOPT_MAX_STRUCTS].  RAFFT_ERR_TEMP as for the fold.  A batch of nothing but erroneous sequences
 * never touches the device.  An internal inconsistency (a partial structure without a continuation, a full stack) is
 * RAFFT_ERR_HIP with a message, never a short list.  On any error of the call *out is NULL. */
#define RAFFT_SUBOPT_MAX_LEN     RAFFT_MFE_MAX_LEN
#define RAFFT_SUBOPT_MAX_STRUCTS (1 << 24)
#define RAFFT_SUBOPT_MAX_DELTA   1000000          /* dcal: mfe + delta stays far below the 5e8 guard of section 9 */
typedef struct {
    int32_t status;        /* BAD_CHAR / EMPTY / TOO_LONG / CAPACITY stay with their sequence */
    int32_t length;
    int32_t mfe_dcal;      /* what rafft_mfe_batch returns */
    int32_t n_structs;     /* rows; 0 when status != 0 */
    int64_t n_reached;     /* CAPACITY only: the count that first exceeded max_structs - a lower bound of the true count */
    const char *db;        /* n_structs rows, length + 1 bytes apart, NUL terminated */
    const int32_t *dcal;   /* [n_structs] */
} rafft_subopt_seq;        /* 40 bytes */
typedef struct { int32_t n_seq, n_failed; rafft_subopt_seq *seq; void *_owner; } rafft_subopt_result;
int  rafft_subopt_batch(int n_seq, const char *const *seqs, const int *lens, double temp, int delta_dcal,
                        int max_structs, long long workspace_bytes /* 0: 512 MiB */, rafft_subopt_result **out);
void rafft_subopt_free(rafft_subopt_result *r);
/* of the last rafft_subopt_batch: levels of the deepest sequence, kernel launches of the enumeration, launches of the table fill,
 * chunks, sequences that ended in RAFFT_ERR_CAPACITY, microseconds spent filling the tables, microseconds spent enumerating and
 * copying */
int  rafft_subopt_counters(long long out[7]);

/* Folding barriers between pairs of structures (direct paths).  Replaces: RNA.fold_compound(seq).path_findpath(A, B,
 * width) / ViennaRNA's `findpath` (Flamm et al. 2001), what a user of the reference takes from ViennaRNA to ask how high the
 * way from one structure of a fast-folding graph to another, or to the MFE structure, climbs.
 * One call, n_paths independent problems: sequence seqs[p] (lens[p] characters), start row starts[p] and end row ends[p] (NUL
 * terminated dot-brackets of ( ) . with lens[p] characters), widths[p] partial paths kept per step.
 * A direct path removes the pairs of A that are not in B and adds the pairs of B that are not in A, one pair per step, every
 * intermediate being a secondary structure: d = |A \ B| + |B \ A| <= lens[p] moves, d + 1 structures.
 * The search is defined exactly, so same input, same bits.  Moves are numbered removals first (ascending 5' end), then additions
 * (ascending 5' end).  A removal is always legal; an addition is legal once every removal that crosses it or shares a base with it
 * is applied.  A state is the set of applied moves with its energy and its saddle so far (the highest energy on its way, both
 * ends included).  Level 0 holds A.  The candidates of the next level are every (state of the beam, legal unapplied move), sorted
 * ascending by (saddle, energy, rank of the parent in its beam, move number); they are taken in that order, a candidate whose set
 * of applied moves equals that of one already taken is skipped (sets are compared, not hashes), and the level is full at
 * widths[p] states.  After d levels every state is B; the first one is the result.  The energy of a candidate is its parent's plus
 * the change of the loops the move touches, from the loop energies rafft_eval_structure uses: rafft_eval_structure of any row of
 * the path gives the path's energy at that step.
 * Outputs (host): rec_out[p]; moves_out may be NULL and so may moves_out[p], else 2 * dist ints (room for 2 * lens[p]): move k is
 * (moves_out[p][2k], moves_out[p][2k+1]) = (i, j) 0-based for an added pair, (-i-1, -j-1) for a removed one; dcal_out may be NULL
 * and so may dcal_out[p], else dist + 1 ints (room for lens[p] + 1): the energy of A, then after every move.
 * dist = 0 (A equals B) is valid: no moves, one energy, saddle = start.
 * Errors of that problem only - the call returns RAFFT_OK, the record has length 0, nothing is written to its path and
 * rafft_last_error() names the first such problem: RAFFT_ERR_EMPTY, RAFFT_ERR_BAD_CHAR (the sequence), RAFFT_ERR_TOO_LONG (above
 * RAFFT_FINDPATH_MAX_LEN), RAFFT_ERR_STRUCT (a malformed row, a row of another length than the sequence, a non-canonical pair in A
 * or B), RAFFT_ERR_CAPACITY (widths[p] x dist above RAFFT_FINDPATH_MAX_CANDIDATES - dist is reported - or an energy that the
 * 22-bit fields of the sort key cannot hold, |energy| >= 2^21 dcal: a hairpin of fewer than 3, for instance; never a silently
 * wrong order).  RAFFT_ERR_PARAM, before anything is launched: a null argument, a negative n_paths or workspace_bytes, a width
 * outside [1, RAFFT_FINDPATH_MAX_WIDTH].  RAFFT_ERR_TEMP as for the fold.  A batch of nothing but erroneous problems never touches
 * the device.  A problem's bits depend on its sequence, A, B, width, temp and the energy tables only - not on the batch, its order,
 * the chunking or the workspace.
 * Device memory: problems are taken in chunks of whole problems in input order whose work areas fit workspace_bytes (0: 512 MiB),
 * one problem at least; a problem's work area is 16 x width x dist bytes and its two beams. */
#define RAFFT_FINDPATH_MAX_LEN        RAFFT_MFE_MAX_LEN
#define RAFFT_FINDPATH_MAX_WIDTH      1024
#define RAFFT_FINDPATH_MAX_CANDIDATES (1 << 20)
typedef struct {
    int32_t status;
    int32_t length;        /* moves of the returned path: dist, or 0 when status != 0 */
    int32_t dist;          /* d = |A \ B| + |B \ A| (also set with RAFFT_ERR_CAPACITY) */
    int32_t start_dcal;    /* energy of A */
    int32_t end_dcal;      /* energy of B */
    int32_t saddle_dcal;   /* the highest energy over the dist + 1 structures of the path, both ends included */
    int32_t saddle_step;   /* the first structure of the path that reaches it: 0 is A, k the structure after move k - 1 */
    int32_t _pad;
} rafft_findpath_rec;      /* 32 bytes */
int rafft_findpath_batch(int n_paths, const char *const *seqs, const int *lens, const char *const *starts, const char *const *ends,
                         const int *widths, double temp, long long workspace_bytes /* 0: 512 MiB */,
                         rafft_findpath_rec *rec_out, int *const *moves_out, int *const *dcal_out);
/* of the last rafft_findpath_batch: chunks, levels over all chunks, kernel launches, problems that ran */
int rafft_findpath_counters(long long out[4]);

/* Gradient walks to local minima.  Replaces: RNA.fold_compound(seq).path_gradient(pt) / ViennaRNA's
 * vrna_path_gradient, RNAlocmin and the flooding of `barriers`, what a user of the reference takes from ViennaRNA to ask which
 * basin of the energy landscape a structure belongs to.
 * One call, n_seq sequences with n_rows[s] start rows each, in the shape of rafft_score_rows: rows[s] holds the rows of sequence s,
 * lens[s] characters of ( ) . each, row_stride[s] >= lens[s] bytes apart - as rafft_sample_batch, rafft_subopt_seq.db and
 * rafft_seq_result.db leave them.  Every row is walked on its own.
 * The walk is defined exactly, so same input, same bits.  The neighbours of a structure (ViennaRNA's default move set: insertion
 * and deletion, lonely pairs allowed) are the removal of any of its pairs and the addition of any (i, j), i < j, whose positions are
 * both unpaired and lie in the same loop (nothing present crosses the new pair), with j - i > 3 and a canonical pair of bases (AU,
 * UA, GC, CG, GU, UG; N pairs with nothing).  The change dE of a neighbour is formed from the loop energies rafft_eval_structure
 * uses - the enclosing loop before and after the move and the moved pair's own loop - so whatever rafft_eval_structure allows is
 * allowed on the way (interior loops above 30 among it).  A step takes, among the neighbours with dE < 0, the one with the smallest
 * (dE, i, j); a position pair is either a removal or an addition, so the key is unique.  With no neighbour below 0 the structure is
 * the end: a local minimum.  Plateaus (dE = 0) are not walked; the energy strictly falls, so the walk ends.
 * max_steps: a walk that has taken max_steps steps and could take another stops with RAFFT_ERR_CAPACITY; the row it reached, its
 * energy and n_steps are returned and the caller may continue from there.  0 means 2 * lens[s] + 16.
 * Outputs (host): seq_out[s]; row_out[seq_out[s].row0 + r]; db_out[s] = n_rows[s] rows, lens[s] + 1 bytes apart, NUL terminated;
 * moves_out may be NULL and so may moves_out[s] (then no device buffer for moves exists), else n_rows[s] blocks of 2 * bound ints,
 * bound = max_steps or 2 * lens[s] + 16: step k of row r is (block[2k], block[2k+1]) = (i, j) 0-based for an added pair,
 * (-i-1, -j-1) for a removed one.  rafft_eval_structure of the start row gives start_dcal, of the end row end_dcal, of any row of
 * the path the running sum.
 * Errors of that sequence only (status in seq_out[s] and in each of its row records, its rows all dots): RAFFT_ERR_BAD_CHAR,
 * RAFFT_ERR_EMPTY, RAFFT_ERR_TOO_LONG (above RAFFT_DESCEND_MAX_LEN).  Errors of that row only: RAFFT_ERR_STRUCT (a character
 * outside ( ) . - a NUL before lens[s] among them - an unbalanced row, a non-canonical pair, a hairpin of fewer than 3; the row
 * comes back as it went in) and RAFFT_ERR_CAPACITY as above.  For these the call returns RAFFT_OK, the neighbours are untouched and
 * rafft_last_error() names the first such item.  RAFFT_ERR_PARAM, before anything is launched: a null argument, a negative count, a
 * stride below the length, a negative max_steps or workspace_bytes.  RAFFT_ERR_TEMP as for the fold.  A batch of nothing but
 * erroneous items never touches the device.  A row's result depends on the sequence, the row, temp, max_steps and the energy tables
 * only - not on the batch, its order, the chunking or the workspace.
 * Device memory: walks are taken in chunks of whole walks in input order whose rows (2 * lens[s] bytes) and move buffers fit
 * workspace_bytes (0: 512 MiB), one walk at least. */
#define RAFFT_DESCEND_MAX_LEN RAFFT_MFE_MAX_LEN
typedef struct {
    int32_t status;
    int32_t length;        /* lens[s] as reported (0 for a negative one) */
    int32_t n_rows;
    int32_t row0;          /* index of the sequence's first record in row_out */
} rafft_descend_seq;       /* 16 bytes */
typedef struct {
    int32_t status;
    int32_t n_steps;       /* steps taken */
    int32_t start_dcal;    /* energy of the start row */
    int32_t end_dcal;      /* energy of the row returned */
} rafft_descend_row;       /* 16 bytes */
int rafft_descend_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows,
                        const int *row_stride, double temp, int max_steps, long long workspace_bytes /* 0: 512 MiB */,
                        rafft_descend_seq *seq_out, rafft_descend_row *row_out, char *const *db_out, int *const *moves_out);
/* of the last rafft_descend_batch: chunks, kernel launches, walks that ran, steps over all walks */
int rafft_descend_counters(long long out[4]);

/* Exact barrier trees of energy bands.  Replaces: `RNAsubopt -e D -s | barriers`, what a user of the
 * reference takes from ViennaRNA to ask for the local minima of a band, the exact saddle that joins each to a deeper one, the
 * basin of every structure, and the tree treekin starts from.
 * Input, per sequence s: the sequence; n_rows[s] rows of ( ) . , lens[s] characters each, row_stride[s] >= lens[s] bytes apart (the
 * shape of rafft_descend_batch; what rafft_subopt_seq.db holds); dcal[s][0 .. n_rows[s]), their energies, non-decreasing (what
 * rafft_subopt_seq.dcal holds).  The RANK of a row is its index.  The landscape is exactly the rows handed over: no energy is
 * evaluated again, and the list need not be a complete band - a deduplicated, sorted sample is a valid input whose missing
 * structures simply are not there.
 * The result is defined exactly, so same input, same bits:
 *   Neighbours: two rows whose pair sets differ by exactly one pair, under rafft_descend_batch's rule - an added pair (i, j) has
 *     both ends unpaired and in the same loop, j - i > 3 and a canonical pair of bases; N pairs with nothing.
 *   Minimum: a row with no neighbour of lower rank.  Equal energies are ordered by rank (as `barriers` orders them: by the list),
 *     so rank 0 is always a minimum.  Minima are numbered by ascending rank.
 *   Gradient basin: down[x] is the lowest-ranked neighbour of x if its rank is below x, else x; basin[x] is the (index of the)
 *     minimum the chain of down reaches; basin_size[m] the number of rows with basin[x] == m.
 *   Tree: for a minimum m let t be the smallest rank such that, in the graph of the rows of rank <= t, the component of m holds a
 *     row of rank below m's.  No such t: father = saddle_rank = -1, a root (minimum 0 is one, and so is whatever the rows do not
 *     connect).  Otherwise saddle_rank = t and father is the minimum index of the lowest-ranked row of that component; father < m,
 *     the barrier is dcal[t] - dcal[rank of m]; saddle_dcal = dcal[t], 0 for a root.  This is what the flooding of `barriers` gives.
 *   Edges: for every unordered pair of distinct gradient basins a < b (minimum indices) with a row x in one that has a neighbour
 *     of lower rank in the other, one edge (a, b, the smallest such x), sorted by (saddle_rank, a, b): the direct saddles between
 *     adjacent basins.  The tree is the minimax closure over them.
 * Identity of a row is the 128-bit commutative hash of its pair set, as for the fold's `seen` table (section 5): two rows of one
 * sequence with the same hash are reported as a duplicate.
 * max_edges: the distinct edges a sequence may have; 0 means 4 * n_rows[s]; values below 1024 count as 1024, above 2^30 as 2^30.  workspace_bytes (0:
 * 512 MiB): sequences are taken in chunks of whole sequences in input order whose work areas (pair tables, keys, the row table,
 * down, basin and the edge table; DESIGN.md section 15 states the bytes) fit it together, one sequence at least.
 * The library owns the result (the number of minima is not known before the call): free it with rafft_barriers_free.
 * Errors of that sequence only (status in seq[s], no minima; the call returns RAFFT_OK, the neighbours are untouched,
 * rafft_last_error() names the first): RAFFT_ERR_BAD_CHAR, RAFFT_ERR_EMPTY (n_rows[s] == 0 too), RAFFT_ERR_TOO_LONG (above
 * RAFFT_BARRIERS_MAX_LEN); RAFFT_ERR_STRUCT for a malformed row (rafft_descend_batch's verdict), a dcal that decreases, a duplicate
 * row (the message names both ranks); RAFFT_ERR_CAPACITY for more than RAFFT_BARRIERS_MAX_ROWS rows, more than max_edges edges
 * (raise max_edges) and a work area above the workspace (the message states the bytes).  RAFFT_ERR_PARAM, before anything is
 * launched: a null argument, a negative count, a stride below the length, a negative max_edges or workspace_bytes.  A batch of
 * nothing but erroneous sequences never touches the device.  A sequence's result depends on its rows and dcal only - not on the
 * batch, its order, the chunking, the workspace, or max_edges when it is large enough.  On any error of the call *out is NULL. */
#define RAFFT_BARRIERS_MAX_LEN  RAFFT_MFE_MAX_LEN
#define RAFFT_BARRIERS_MAX_ROWS RAFFT_SUBOPT_MAX_STRUCTS
typedef struct { int32_t rank, father, saddle_rank, dcal, saddle_dcal, basin_size; } rafft_barriers_min;   /* 24 bytes */
typedef struct { int32_t a, b, saddle_rank; } rafft_barriers_edge;                                          /* 12 bytes */
typedef struct { int32_t status, length, n_rows, n_minima, n_edges, _pad;
                 const rafft_barriers_min *minima; const rafft_barriers_edge *edges; const int32_t *basin /* [n_rows]: minimum index */; } rafft_barriers_seq;
typedef struct { int32_t n_seq, n_failed; rafft_barriers_seq *seq; void *_owner; } rafft_barriers_result;
int  rafft_barriers_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows,
                          const int *row_stride, const int *const *dcal, int max_edges, long long workspace_bytes,
                          rafft_barriers_result **out);
void rafft_barriers_free(rafft_barriers_result *r);
/* of the last rafft_barriers_batch: chunks, kernel launches, rows that ran, neighbour probes that hit (of the pass that finds
 * down), minima, edges */
int  rafft_barriers_counters(long long out[6]);

/* Stochastic folding trajectories.  Replaces: ViennaRNA's Kinfold, what a user of the reference runs to
 * simulate folding on the full move set: continuous-time Monte Carlo (Gillespie) over insertion and deletion of single pairs,
 * from the open chain or any structure, with first-passage times to stop structures and the state at given times.
 * One call, n_seq sequences with n_rows[s] start rows each in the shape of rafft_descend_batch (rows, row_stride), and n_rep >= 1
 * trajectories per row: trajectory k = r * n_rep + rep of sequence s starts from row r.
 * The process is defined exactly, so same input, same bits.
 *  - Neighbours and dE: exactly rafft_descend_batch's (insertion and deletion, lonely pairs allowed; dE from the three loop terms).
 *  - Rates: Metropolis, min(1, exp(-dE / (100 kT))), dE in dcal, kT in kcal/mol = kt, or 1.98717e-3 * (temp + 273.15) when kt is 0.
 *  - Weights: rates are integer weights W[d] of a table of RAFFT_KINFOLD_NW = 4096 uint64 entries the host builds once per call
 *    (rafft_kinfold_weights): W[0] = 2^32 for every dE <= 0 - the table is uint64 so that it holds it -, W[d] = floor(2^32 *
 *    exp(-d / (100 kT)) + 0.5), weight 0 for dE >= 4096.  A move of weight 0 is never taken: relative rates below 2^-33 are dropped.
 *  - Step number t (from 0) of trajectory k: the Philox4x32-10 block of counter (k, t, 0, 0) under seeds[s] gives u = the 53-bit
 *    uniform of words 0-1 (rafft_sample_batch's draw t of sample k) and v = word 2 << 32 | word 3.  Wtot = the sum of the weights
 *    of all neighbours (64 bits).  Wtot == 0: the state is absorbing, the trajectory ends with time = t_max and
 *    RAFFT_KINFOLD_ABSORBED.  dt = -log(1 - u) * 2^32 / Wtot in double; time + dt > t_max: it ends in the current state with
 *    time = t_max and RAFFT_KINFOLD_TIME.  Otherwise, max_steps steps taken already: it ends with RAFFT_KINFOLD_MORE, status
 *    RAFFT_ERR_CAPACITY and time = the time of its last jump (0: max_steps is RAFFT_KINFOLD_DEFAULT_STEPS).  Otherwise r = the
 *    upper 64 bits of v * Wtot, the move is the first in ascending (i, j) whose inclusive cumulative weight exceeds r (bias at most
 *    Wtot / 2^64), it is applied and time += dt.
 *  - Watched rows: watch[s] holds n_watch[s] <= 64 rows of sequence s, watch_stride[s] apart, parsed as start rows are; the first
 *    n_stop[s] of them are absorbing: a trajectory that arrives at one ends with RAFFT_KINFOLD_STOP, stop_index = its index (the
 *    lowest, should two be equal) and time = the arrival time; a start row that is a stop row ends at time 0 with 0 steps.
 *    n_watch may be NULL (nothing is watched anywhere).
 *  - Sample grid: sample_times[n_times] ascending within [0, t_max]; for every tau a trajectory records the state it is in at tau
 *    (after every jump at a time <= tau): its energy and the lowest watched row it equals, or -1.  After STOP or ABSORBED the last
 *    state holds; after MORE the times not below the jump that was not taken hold (INT32_MIN, -2).
 * Outputs (host): seq_out[s]; traj_out[seq_out[s].traj0 + k]; db_out[s] = n_rows[s] * n_rep end rows, lens[s] + 1 bytes apart, NUL
 * terminated; samples_out[s] (may be NULL when n_times is 0) = per trajectory n_times pairs of int32 (dcal, watch index);
 * moves_out / times_out may be NULL and so may their entries (both or neither per sequence; then no device buffer for logs
 * exists), else per trajectory a block of 2 * bound ints as rafft_descend_batch's moves and a block of bound doubles, the time of
 * every jump; bound = max_steps or RAFFT_KINFOLD_DEFAULT_STEPS.
 * Errors of that sequence only (its rows all dots, its samples (INT32_MIN, -2)): RAFFT_ERR_BAD_CHAR, RAFFT_ERR_EMPTY,
 * RAFFT_ERR_TOO_LONG (above RAFFT_KINFOLD_MAX_LEN), RAFFT_ERR_STRUCT for a malformed watched row.  Errors of that start row only
 * (all its trajectories): RAFFT_ERR_STRUCT as in rafft_descend_batch (the row comes back as it went in); of that trajectory:
 * RAFFT_ERR_CAPACITY as above.  For these the call returns RAFFT_OK, the neighbours are untouched and rafft_last_error() names the
 * first such item.  RAFFT_ERR_PARAM, before anything is launched: a null argument, a negative count, a stride below the length,
 * n_rep < 1, n_watch > 64, n_stop > n_watch, t_max negative or not finite, a grid that descends, is negative or exceeds t_max,
 * kt negative or not finite, a negative max_steps or workspace_bytes.  RAFFT_ERR_TEMP as for the fold.  A batch of nothing but
 * erroneous items never touches the device.  A trajectory depends on the sequence, its start row, the energy tables, temp, kt, the
 * seed, k, t_max, max_steps, the watched rows and the grid only - not on the batch, its order, the chunking or the workspace.
 * Device memory: trajectories are taken in chunks of whole trajectories in input order whose rows, samples and logs fit
 * workspace_bytes (0: 512 MiB), one at least; the watched rows and the weight table lie beside them for the whole call. */
#define RAFFT_KINFOLD_MAX_LEN RAFFT_DESCEND_MAX_LEN
#define RAFFT_KINFOLD_NW 4096
#define RAFFT_KINFOLD_MAX_WATCH 64
#define RAFFT_KINFOLD_DEFAULT_STEPS (1 << 20)
#define RAFFT_KINFOLD_TIME 1
#define RAFFT_KINFOLD_STOP 2
#define RAFFT_KINFOLD_ABSORBED 4
#define RAFFT_KINFOLD_MORE 8
typedef struct {
    int32_t status;
    int32_t length;        /* lens[s] as reported (0 for a negative one) */
    int32_t n_traj;        /* n_rows[s] * n_rep */
    int32_t traj0;         /* index of the sequence's first record in traj_out */
} rafft_kinfold_seq;       /* 16 bytes */
typedef struct {
    int32_t status;
    int32_t flags;         /* RAFFT_KINFOLD_*: why it ended */
    int32_t n_steps;       /* jumps taken */
    int32_t start_dcal;    /* energy of the start row */
    int32_t end_dcal;      /* energy of the row returned */
    int32_t stop_index;    /* the stop row it arrived at, or -1 */
    double time;           /* arrival (STOP), last jump (MORE), else t_max */
} rafft_kinfold_traj;      /* 32 bytes */
int rafft_kinfold_batch(int n_seq, const char *const *seqs, const int *lens, const int *n_rows, const char *const *rows,
                        const int *row_stride, int n_rep, const int *n_watch, const int *n_stop, const char *const *watch,
                        const int *watch_stride, const unsigned long long *seeds /* [n_seq]; NULL: all 0 */, double temp, double kt,
                        double t_max, int max_steps, int n_times, const double *sample_times, long long workspace_bytes /* 0: 512 MiB */,
                        rafft_kinfold_seq *seq_out, rafft_kinfold_traj *traj_out, char *const *db_out, int32_t *const *samples_out,
                        int *const *moves_out, double *const *times_out);
/* the weight table of a call at (temp, kt): RAFFT_KINFOLD_NW entries; RAFFT_ERR_PARAM for a null pointer, a kt that is negative
 * or not finite, or a kT that is not above 0.  Host only: needs no device. */
int rafft_kinfold_weights(double temp, double kt, uint64_t *out /* RAFFT_KINFOLD_NW */);
/* of the last rafft_kinfold_batch: chunks, kernel launches, trajectories that ran, steps over all trajectories */
int rafft_kinfold_counters(long long out[4]);

/* library / build information: "gfx950 ..." */
const char *rafft_version(void);

#ifdef __cplusplus
}
#endif
#endif
