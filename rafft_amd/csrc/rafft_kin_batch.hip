// rafft_kin_batch.hip - the folding kinetics of a whole batch of fast-folding graphs (C-ABI rafft_kin_batch).
//
// Many small graphs, a few hundred states each, in one call: which rows are the same structure (rafft/rafft_kin.py:106-112), the
// rate matrix of every graph (rafft_kin.py:48-56,68-91 - the device bodies of rafft_kin.hip, per graph) and the master equation
// dp/dt = rate^T p from the unfolded state (rafft_kin.py:94-150), integrated with the TR-BDF2 scheme of
// rafft_kin.solve_master_equation(method="implicit").
//   rows      all graphs' dot-bracket rows packed back to back: graph g's rows start at byte KinGraph::off, L bytes each; the pair
//             tables use the same offsets (in 16-bit entries).  Row arrays are indexed by the row's number in the whole batch.
//   identity  a 64-bit hash per row, then for every row a wavefront scans the earlier rows of its graph for an equal hash AND equal
//             bytes - exact, not probabilistic.  uid = rank of the first appearance.
//   matrices  per graph and per chunk of the workspace three S x S blocks: R (the rate matrix, row-major as rafft_kin_rate_matrix
//             gives it), A = R^T (the generator) and W.
//   solve     one workgroup per graph.  A has non-negative off-diagonals and zero column sums, so M = I - c h A is strictly
//             column-diagonally dominant: elimination needs no pivoting.  Per output interval W = M^-1 by Gauss-Jordan in place,
//             then every sub-step is three matrix-vector products (a triangular solve would be a chain of S barriers, twice per
//             stage).  W lives in LDS for graphs of up to KIN_BATCH_LDS_STATES states.
// Every floating-point sum has a fixed order that depends on the graph alone: a graph's populations are the same bits wherever it
// sits in a batch and whatever else the batch holds.  Every loop bound is known at launch.  fp64 vector work: no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

struct KinGraph {
    unsigned long long off;     // first byte of the graph's rows in the packed buffer (= first entry of its pair tables)
    unsigned long long mat;     // first double of its three S x S blocks in the chunk's workspace
    int L, n_rows, row0;        // row0: number of its first row in the batch
    int S;                      // unique structures; 0 until they are known and for a graph that is not solved
};

#define KIN_BATCH_LDS_STATES 128
#define KINB_NT 1024
#define KINB_NW (KINB_NT / 64)

// pair table and hash of every row: one thread per row
__global__ void kin_batch_pair_table_kernel(int n, const KinGraph *graphs, const int *row_graph, const char *rows, int16_t *pt, int16_t *stack,
                                            unsigned long long *hash, int *bad)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int g = row_graph[r];
    const KinGraph G = graphs[g];
    const size_t at = (size_t)G.off + (size_t)(r - G.row0) * G.L;
    if (!kin_pair_table_row(G.L, rows + at, pt + at, stack + at)) bad[g] = 1;
    unsigned long long h = 0xcbf29ce484222325ull;             // FNV-1a
    for (int x = 0; x < G.L; x++) h = (h ^ (unsigned char)rows[at + x]) * 0x100000001b3ull;
    hash[r] = h;
}

// first[r] = the earliest row of r's graph with the same bytes (numbered inside the graph), r itself when there is none.
// One wavefront per row, four per workgroup; nothing waits on another wavefront.
__global__ __launch_bounds__(256) void kin_batch_identity_kernel(int n, const KinGraph *graphs, const int *row_graph, const char *rows,
                                                                 const unsigned long long *hash, int *first)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const KinGraph G = graphs[row_graph[r]];
    const int L = G.L, lr = r - G.row0;
    const char *base = rows + (size_t)G.off, *me = base + (size_t)lr * L;
    const unsigned long long hme = hash[r];
    int found = lr;
    for (int j0 = 0; j0 < lr && found == lr; j0 += 64) {
        const int j = j0 + lane;
        unsigned long long cand = __ballot(j < lr && hash[G.row0 + j] == hme);
        while (cand && found == lr) {                         // at most 64 rounds, earliest row first
            const int b = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const char *other = base + (size_t)(j0 + b) * L;
            bool same = true;
            for (int x0 = 0; x0 < L && same; x0 += 64) {
                const int x = x0 + lane;
                if (__ballot(x < L && other[x] != me[x])) same = false;
            }
            if (same) found = j0 + b;
        }
    }
    if (lane == 0) first[r] = found;
}

// rank of every first appearance in its graph: one workgroup per graph walks its rows 256 at a time.  rank[r] for the rows that are
// a first appearance; for unique u of the graph first_row[row0 + u] and energy_u[row0 + u] (the energy of that row,
// rafft_kin.py:115); n_unique[g].
__global__ __launch_bounds__(256) void kin_batch_rank_kernel(const KinGraph *graphs, const int *first, const double *energy_row, int *rank, int *first_row,
                                                             double *energy_u, int *n_unique)
{
    __shared__ int wtot[4];
    const KinGraph G = graphs[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int base = 0;
    for (int r0 = 0; r0 < G.n_rows; r0 += 256) {
        const int lr = r0 + (int)threadIdx.x;
        const bool is_first = lr < G.n_rows && first[G.row0 + lr] == lr;
        const unsigned long long bal = __ballot(is_first);
        if (lane == 0) wtot[wv] = __popcll(bal);
        __syncthreads();
        int before = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; w++) before += wtot[w];
        if (is_first) {
            rank[G.row0 + lr] = before;
            first_row[G.row0 + before] = lr;
            energy_u[G.row0 + before] = energy_row[G.row0 + lr];
        }
        base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) n_unique[blockIdx.x] = base;
}

__global__ void kin_batch_uid_kernel(int n, const KinGraph *graphs, const int *row_graph, const int *first, const int *rank, int *uid)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int row0 = graphs[row_graph[r]].row0;
    uid[r] = rank[row0 + first[r]];
}

// rates: one workgroup per row r = ra + blockIdx.x of the chunk, against the rows of the step before its own (row_prev0[r],
// row_nprev[r]: the LAST step for a row of step 0, rafft_kin.py:75).  The inclusion search is kin_rates_row of rafft_kin.hip.
__global__ __launch_bounds__(KIN_NT) void kin_batch_rates_kernel(int ra, const KinGraph *graphs, const int *row_graph, const int *row_prev0, const int *row_nprev,
                                                                 const int16_t *pt, const int *uid, const double *energy_u, double kt, double *ws)
{
    extern __shared__ int16_t cur[];
    const int r = ra + blockIdx.x;
    const KinGraph G = graphs[row_graph[r]];
    const int n_prev = row_nprev[r];
    if (G.S == 0 || n_prev == 0) return;
    const int16_t *gp = pt + (size_t)G.off;
    kin_rates_row(G.L, gp + (size_t)(r - G.row0) * G.L, gp + (size_t)(row_prev0[r] - G.row0) * G.L, n_prev, uid[r], uid + row_prev0[r],
                  energy_u + G.row0, kt, G.S, ws + G.mat, cur);
}

// diagonal = -(row sum) in the order of kin_row_sum, the non-zero off-diagonals counted, the row written into A = R^T.
// One workgroup per (graph, unique structure): block ra + blockIdx.x stands for unique u = its row number inside the graph.
__global__ __launch_bounds__(256) void kin_batch_diag_kernel(int ra, const KinGraph *graphs, const int *row_graph, double *ws, int *n_edges)
{
    __shared__ double part[256];
    __shared__ int cnt;
    const int r = ra + blockIdx.x, g = row_graph[r];
    const KinGraph G = graphs[g];
    const int S = G.S, u = r - G.row0;
    if (u >= S) return;
    double *R = ws + G.mat, *A = R + (size_t)S * S;
    const double *row = R + (size_t)u * S;
    if (threadIdx.x == 0) cnt = 0;
    const double s = kin_row_sum(S, row, part);               // (the diagonal entry is still 0)
    int mine = 0;
    for (int c = threadIdx.x; c < S; c += 256) {
        const double v = row[c];
        if (c != u) { mine += v != 0.0; A[(size_t)c * S + u] = v; }
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        R[(size_t)u * S + u] = -s;
        A[(size_t)u * S + u] = -s;
        if (cnt) atomicAdd(&n_edges[g], cnt);
    }
}

// out[i] = sum_j M[i][j] x[j]: a wavefront per row, lanes over the columns, a butterfly over the lanes; done(i, sum) by lane 0
template <class F> __device__ __forceinline__ void kin_batch_matvec(int S, const double *M, const double *x, F done)
{
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < S; i += KINB_NW) {
        const double *row = M + (size_t)i * S;
        double s = 0.0;
        for (int j = lane; j < S; j += 64) s += row[j] * x[j];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) done(i, s);
    }
}

// TR-BDF2 from each output time to the next (rafft_kin.solve_master_equation, "implicit": gamma = 2 - sqrt 2, both stages solve with
// I - c h A, c = 1 - 1/sqrt 2), everything on structure 0 at t = 0.  One workgroup per graph, graph order[blockIdx.x]: the host
// lists the chunk's graphs of up to KIN_BATCH_LDS_STATES states for the instantiation with W in LDS and the rest for the other one.
// pop: graph g's block at n_times * (row0 - ra) doubles, n_times rows of S.
template <bool LDSW> __global__ __launch_bounds__(KINB_NT) void kin_batch_integrate_kernel(const int *order, int ra, const KinGraph *graphs, double *ws, int n_times,
                                                                                            const int *msub, const double *hsub, double *pop)
{
    extern __shared__ double kb_lds[];
    const KinGraph G = graphs[order[blockIdx.x]];
    const int S = G.S;
    if (S == 0 || (S <= KIN_BATCH_LDS_STATES) != LDSW) return;
    constexpr int VS = LDSW ? KIN_BATCH_LDS_STATES : RAFFT_KIN_BATCH_MAX_STATES;
    double *y = kb_lds, *v = y + VS, *u = v + VS, *prow = u + VS, *red = prow + VS;      // red: one double
    const double *A = ws + G.mat + (size_t)S * S;
    double *W = LDSW ? red + 1 : ws + G.mat + 2 * (size_t)S * S;
    double *out = pop + (size_t)n_times * (size_t)(G.row0 - ra);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double gm = 2.0 - sqrt(2.0), c = 1.0 - 0.5 * sqrt(2.0);
    const double s2a = gm * (2.0 - gm), s2b = (1.0 - gm) * (1.0 - gm) / (gm * (2.0 - gm));
    for (int i = tid; i < S; i += KINB_NT) y[i] = i == 0 ? 1.0 : 0.0;
    for (int k = 0; k < n_times; k++) {
        const double h = hsub[k], ch = c * h, s1 = 0.5 * gm * h;
        const int m = msub[k];
        for (int e = tid; e < S * S; e += KINB_NT) W[e] = (e / S == e % S ? 1.0 : 0.0) - ch * A[e];
        __syncthreads();
        // W <- W^-1, Gauss-Jordan in place without pivoting: column kk of the identity replaces column kk of W
        for (int kk = 0; kk < S; kk++) {
            const double p = 1.0 / W[(size_t)kk * S + kk];
            for (int j = tid; j < S; j += KINB_NT) prow[j] = j == kk ? p : W[(size_t)kk * S + j] * p;
            __syncthreads();
            for (int i = wv; i < S; i += KINB_NW) {
                double *row = W + (size_t)i * S;
                if (i == kk) {
                    for (int j = lane; j < S; j += 64) row[j] = prow[j];
                    continue;
                }
                double f = lane == 0 ? row[kk] : 0.0;         // one lane reads the multiplier before the update below overwrites it
                f = __shfl(f, 0);
                if (f == 0.0) continue;                       // (a function of the graph's own matrix: x - 0 * y = x)
                for (int j = lane; j < S; j += 64) row[j] = (j == kk ? 0.0 : row[j]) - f * prow[j];
            }
            __syncthreads();
        }
        for (int sub = 0; sub < m; sub++) {
            kin_batch_matvec(S, A, y, [&](int i, double s) { v[i] = y[i] + s1 * s; });
            __syncthreads();
            kin_batch_matvec(S, W, v, [&](int i, double s) { u[i] = s / s2a - s2b * y[i]; });
            __syncthreads();
            kin_batch_matvec(S, W, u, [&](int i, double s) { y[i] = s; });
            __syncthreads();
        }
        if (wv == 0) {
            double s = 0.0;
            for (int j = lane; j < S; j += 64) s += y[j];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) red[0] = s;
        }
        __syncthreads();
        const double tot = red[0];
        for (int i = tid; i < S; i += KINB_NT) out[(size_t)k * S + i] = y[i] / tot;
        __syncthreads();
    }
}
