// rafft_landscape.hip - the folding landscape of a fast-folding graph on the GPU.
//
// Replaces the arithmetic of the reference's utility/surface.py (everything but the drawing):
//   get_distance_matrix   surface.py:19-26     base-pair distance between every two structures, one RNA.bp_distance call per
//                                              pair in a Python double loop
//   manifold.MDS(...)     surface.py:98-101    metric multidimensional scaling of that matrix onto a plane (scikit-learn's SMACOF,
//                                              max_iter=5000, eps=1e-9, several random starts)
//   interpolate.Rbf(...)  surface.py:107-111   thin-plate energy surface over the plane, evaluated on a regular grid
//
// Base-pair distance (ViennaRNA's bp_distance): the number of base pairs that are in exactly one of the two structures,
//   d(A, B) = |A| + |B| - 2 |A n B|.
// With the "opening table" t[x] = partner of x (1-based, so never 0) when x opens a pair, else 0 (16 bits per position),
// |A n B| is the number of positions x with tA[x] == tB[x] != 0.
//
// All floating-point work is fp64 (the reference's is) and every sum has a fixed order: no float atomics, so the same input
// gives the same bits.  MDS components: 2, the only value the reference uses.
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---------------------------------------------------------------------------------------------------------------- distances

// opening tables from pair tables (kin_pair_table_kernel: -1 = unpaired, else the 0-based partner).  One wavefront per row; rows of
// `open` are Lp = L rounded up to LS_CHUNK positions, the tail zero.  npairs[r] = |A|.
#define LS_CHUNK 64                      // positions of L per LDS stage (32 words of two positions)
#define LS_TILE 64                       // structures per tile side
#define LS_STRIDE (LS_TILE + 4)          // LDS row stride in words: 16-byte aligned rows, staging stores 2-way conflicted at most

__global__ __launch_bounds__(64) void landscape_open_table_kernel(int n, int L, int Lp, const int16_t *pt, uint16_t *open, int *npairs)
{
    const int r = blockIdx.x;
    if (r >= n) return;
    const int16_t *p = pt + (size_t)r * L;
    uint16_t *o = open + (size_t)r * Lp;
    int cnt = 0;
    for (int x = threadIdx.x; x < Lp; x += 64) {
        const int q = x < L ? (int)p[x] : -1;
        const bool opens = q > x;
        o[x] = opens ? (uint16_t)(q + 1) : (uint16_t)0;
        cnt += opens;
    }
    for (int o2 = 32; o2 > 0; o2 >>= 1) cnt += __shfl_down(cnt, o2, 64);
    if (threadIdx.x == 0) npairs[r] = cnt;
}

// bit 15 / bit 31 set where the low / high 16-bit half of x is zero (exact: no carry crosses the halves)
__device__ __forceinline__ uint32_t ls_zero_halves(uint32_t x)
{
    const uint32_t y = ((x & 0x7fff7fffu) + 0x7fff7fffu) | x;
    return ~y & 0x80008000u;
}

// All-pairs distance, shaped like a small GEMM: a workgroup of 256 owns a 64 x 64 tile of (structures x structures) on or above
// the diagonal, walks L in chunks of 64 positions staged in LDS ([word][structure], so that a thread reads its 4 structures with
// one 16-byte LDS load), and every thread keeps a 4 x 4 register tile of match counts.  Two positions per 32-bit operation: the
// column side is staged with its zero halves turned into 0xffff (never a partner), so a match is a zero half of a ^ b.
// dist: n x n row-major uint16; both halves are written.
__global__ __launch_bounds__(256) void landscape_distance_kernel(int n, int Lp, const uint16_t *open, const int *npairs, uint16_t *dist)
{
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ __attribute__((aligned(16))) uint32_t As[LS_CHUNK / 2][LS_STRIDE];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[LS_CHUNK / 2][LS_STRIDE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = bi * LS_TILE, j0 = bj * LS_TILE;
    const int words = Lp / 2;                                     // per row of `open`
    const uint32_t *ow = (const uint32_t *)open;
    int cnt[4][4] = {};
    for (int w0 = 0; w0 < words; w0 += LS_CHUNK / 2) {
        // stage: 64 rows x 32 words per side, 8 words per thread and side; a row's 32 words are one 128-byte line
        for (int k = tid; k < LS_TILE * (LS_CHUNK / 2); k += 256) {
            const int r = k >> 5, w = k & 31;
            const uint32_t a = i0 + r < n ? ow[(size_t)(i0 + r) * words + w0 + w] : 0u;
            uint32_t b = j0 + r < n ? ow[(size_t)(j0 + r) * words + w0 + w] : 0u;
            const uint32_t z = ls_zero_halves(b);
            b |= (z >> 15) * 0xffffu;
            As[w][r] = a;
            Bs[w][r] = b;
        }
        __syncthreads();
#pragma unroll 4
        for (int w = 0; w < LS_CHUNK / 2; w++) {
            const uint4 a4 = *(const uint4 *)&As[w][ty * 4];
            const uint4 b4 = *(const uint4 *)&Bs[w][tx * 4];
            const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int q = 0; q < 4; q++) cnt[p][q] += __popc(ls_zero_halves(a[p] ^ b[q]));
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int i = i0 + ty * 4 + p;
        if (i >= n) continue;
        const int ni = npairs[i];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int j = j0 + tx * 4 + q;
            if (j >= n) continue;
            const uint16_t d = (uint16_t)(ni + npairs[j] - 2 * cnt[p][q]);
            dist[(size_t)i * n + j] = d;
            dist[(size_t)j * n + i] = d;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- SMACOF

// per-start state of the iteration, in device memory; the host reads `done` between chunks of launches
struct LandscapeMdsState {
    int done;              // 1: finished, x_out / stress / n_iter are final
    int n_iter;            // iterations done (scikit-learn's n_iter_ once finished)
    double old_stress;     // stress of the previous iteration's result
    double stress;         // stress of the latest result
};

#define LS_SM_NT 1024                    // 16 wavefronts: one row of D per wavefront at a time

__device__ __forceinline__ double ls_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);      // fixed tree
    return v;
}

// One pass over D for `n_init` independent starts (blockIdx.y).  Pass p reads X_p (xbuf[p & 1]) and produces, per row i,
//   X_{p+1}[i]   = (1/S) sum_j ratio_ij (X_i - X_j),  ratio_ij = D_ij / dis_ij,  dis_ij == 0 -> 1e-5 in the ratio only
//                  (the Guttman transform of sklearn.manifold._mds._smacof_single, metric case)         -> xbuf[(p + 1) & 1]
//   rowsum[0][i] = sum_j (dis_ij - D_ij)^2       the stress of X_p, i.e. of the result of iteration p (before the factor 1/2)
//   rowsum[1][i] = sum_j dis_ij^2                the denominator of the stopping rule
// so one pass serves the transform of iteration p + 1 and the stress of iteration p.  `guttman` = 0 in the last pass (stress only).
// A wavefront owns a row: lanes stride j (D row read coalesced), X in LDS when XLDS (16 B per point), wave sums in a fixed tree.
template <bool XLDS>
__global__ __launch_bounds__(LS_SM_NT) void landscape_smacof_kernel(int S, const uint16_t *dist, double *xbuf, double *rowsum,
                                                                     const LandscapeMdsState *state, int pass, int guttman)
{
    extern __shared__ __attribute__((aligned(16))) double2 ls_x[];
    const int start = blockIdx.y;
    if (state[start].done) return;
    const double2 *xin = (const double2 *)xbuf + ((size_t)start * 2 + (pass & 1)) * S;
    double2 *xout = (double2 *)xbuf + ((size_t)start * 2 + ((pass + 1) & 1)) * S;
    double *rs_stress = rowsum + (size_t)start * 2 * S, *rs_sq = rs_stress + S;
    const double2 *xs = xin;
    if (XLDS) {
        for (int k = threadIdx.x; k < S; k += LS_SM_NT) ls_x[k] = xin[k];
        __syncthreads();
        xs = ls_x;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double inv_n = 1.0 / (double)S;
    for (int i = blockIdx.x * (LS_SM_NT / 64) + wv; i < S; i += gridDim.x * (LS_SM_NT / 64)) {
        const double2 xi = xs[i];
        const uint16_t *drow = dist + (size_t)i * S;
        double gx = 0.0, gy = 0.0, st = 0.0, sq = 0.0;
        for (int j = lane; j < S; j += 64) {
            const double d = (double)drow[j];
            const double2 xj = xs[j];
            const double dx = xi.x - xj.x, dy = xi.y - xj.y;
            const double d2 = dx * dx + dy * dy;
            const double dis = sqrt(d2);
            const double e = dis - d;
            st += e * e;
            sq += dis * dis;
            if (guttman) {
                const double ratio = d / (dis == 0.0 ? 1e-5 : dis);
                gx += ratio * dx;
                gy += ratio * dy;
            }
        }
        st = ls_wave_sum(st); sq = ls_wave_sum(sq);
        if (guttman) { gx = ls_wave_sum(gx); gy = ls_wave_sum(gy); }
        if (lane == 0) {
            rs_stress[i] = st; rs_sq[i] = sq;
            if (guttman) xout[i] = make_double2(inv_n * gx, inv_n * gy);
        }
    }
}

// The sequential rule of _smacof_single, taken on the device: one workgroup per start sums the row partials in a fixed order and
// decides.  After pass p >= 1: stress_p = stress of the result of iteration p; stop when p >= 2 and
// (stress_{p-1} - stress_p) / (sum_sq / 2) < eps, or when p == max_iter; the result is then X_p (xbuf[p & 1]), copied to x_out.
__global__ __launch_bounds__(256) void landscape_smacof_finalize_kernel(int S, const double *xbuf, const double *rowsum, LandscapeMdsState *state,
                                                                        int pass, int max_iter, double eps, double *x_out)
{
    __shared__ double pa[256], pb[256];
    __shared__ int finished;
    const int start = blockIdx.x;
    LandscapeMdsState *s = state + start;
    if (s->done || pass == 0) return;
    const double *rs_stress = rowsum + (size_t)start * 2 * S, *rs_sq = rs_stress + S;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < S; i += 256) { a += rs_stress[i]; b += rs_sq[i]; }
    pa[threadIdx.x] = a; pb[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { pa[threadIdx.x] += pa[threadIdx.x + o]; pb[threadIdx.x] += pb[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double stress = pa[0] / 2, sum_sq = pb[0];
        bool stop = pass >= max_iter;
        if (pass >= 2 && (s->old_stress - stress) / (sum_sq / 2) < eps) stop = true;
        s->old_stress = stress;
        s->stress = stress;
        s->n_iter = pass;
        finished = stop;
    }
    __syncthreads();
    if (!finished) return;
    const double *xin = xbuf + ((size_t)start * 2 + (pass & 1)) * S * 2;
    for (int k = threadIdx.x; k < 2 * S; k += 256) x_out[(size_t)start * 2 * S + k] = xin[k];
    __syncthreads();
    if (threadIdx.x == 0) s->done = 1;
}

// ------------------------------------------------------------------------------------------------------- thin-plate surface

// phi(r) = r^2 log r, phi(0) = 0  (scipy.interpolate.Rbf function="thin_plate": xlogy(r**2, r))
__device__ __forceinline__ double ls_tps(double dx, double dy)
{
    const double r = sqrt(dx * dx + dy * dy);
    return r == 0.0 ? 0.0 : (r * r) * log(r);
}

// (i) the S x S system matrix of the interpolation, row-major
__global__ __launch_bounds__(256) void landscape_tps_fill_kernel(int S, const double *x, double *phi)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= S) return;
    const double2 xi = ((const double2 *)x)[i], xj = ((const double2 *)x)[j];
    phi[(size_t)i * S + j] = ls_tps(xi.x - xj.x, xi.y - xj.y);
}

// (ii) z[gy][gx] = sum_k w_k phi(|| (ti[gx], ti[gy]) - X_k ||), ti = linspace(lo, hi, G): one thread per grid point, nodes and weights
// tiled through LDS, summed in node order
#define LS_TPS_TILE 256
__global__ __launch_bounds__(256) void landscape_tps_kernel(int S, const double *x, const double *w, int G, double lo, double hi, double *z)
{
    __shared__ double nx[LS_TPS_TILE], ny[LS_TPS_TILE], nw[LS_TPS_TILE];
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = gid < (long long)G * G;
    const int gy = live ? (int)(gid / G) : 0, gx = live ? (int)(gid % G) : 0;
    const double step = G > 1 ? (hi - lo) / (double)(G - 1) : 0.0;
    const double px = G > 1 && gx == G - 1 ? hi : lo + (double)gx * step;      // numpy.linspace: start + k * step, the last point = stop
    const double py = G > 1 && gy == G - 1 ? hi : lo + (double)gy * step;
    double acc = 0.0;
    for (int k0 = 0; k0 < S; k0 += LS_TPS_TILE) {
        const int k = k0 + threadIdx.x;
        if (k < S) { nx[threadIdx.x] = x[2 * k]; ny[threadIdx.x] = x[2 * k + 1]; nw[threadIdx.x] = w[k]; }
        __syncthreads();
        const int m = min(LS_TPS_TILE, S - k0);
        for (int t = 0; t < m; t++) acc += nw[t] * ls_tps(px - nx[t], py - ny[t]);
        __syncthreads();
    }
    if (live) z[gid] = acc;
}
