// rafft_pf_span.hip - partition function and pair probabilities under a base-pair span (gfx950): the ensemble of rafft_pf.hip
// restricted to structures whose pairs (i,j) all have j - i + 1 <= max_span, for sequences of up to RAFFT_MFE_SPAN_MAX_LEN.
// DESIGN.md section 19.  Included by rafft_api.hip after rafft_pf.hip, whose pf_cell and pf_out_cell run here unchanged over a
// banded view, and after rafft_mfe_span.hip, whose fold gives the scale.
//
// A cell (i,j) with d = j - i < W = min(max_span, L) reads, inside, only cells within (i,j) and, outside, only cells of a larger d
// that the view has (hi / lo / has): the tables are L x W, a pass is W launches, one per anti-diagonal.  The exterior loop is not
// restricted: F[j] looks at the stems (i,j) of the window i >= j - W + 1 and at F[j-1], Fr likewise from the 3' end.  F and Fr
// cover up to 32768 positions under one per-nucleotide scale, which no fp64 exponent holds: each is a mantissa in [1, 2) and a
// binary exponent per position (PfX), renormalised by powers of two only.  The outside tables are divided by 2^(exponent of Z), so
// the exterior term of Co, F[i] w Fr[j + 1] / 2^e_Z, and with it every outside cell is of the order of 1 / (its inside cell).
#pragma once

#include "rafft_batch_layout.h"     // PfSpanSeq

// The banded view (as MfeTabBand): a split reads M along a row and M1 along a column, so C, M, Co, Mo are stored by their 5' end
// as [i][d] and M1, M1o by their 3' end as [j][d]: the 64 lanes of a split read 64 consecutive doubles of each factor.  It has the
// cells with q - p < W; nothing reads beyond them (the loops of pf_out_cell are bounded by hi / lo / has, it does not rely on a
// zero read).
struct PfTabBand {
    double *t0;                     // table k (C, M, M1, Co, Mo, M1o) starts at t0 + k L W: one pointer in scalar registers, not six
    int L, W;
    __device__ __forceinline__ size_t n() const { return (size_t)L * W; }
    __device__ __forceinline__ size_t by5(int i, int j) const { return (size_t)i * W + (j - i); }
    __device__ __forceinline__ size_t by3(int i, int j) const { return (size_t)j * W + (j - i); }
    __device__ __forceinline__ double *tab(int k) const { return t0 + k * n(); }
    __device__ __forceinline__ double &c(int i, int j) const { return t0[by5(i, j)]; }
    __device__ __forceinline__ double &m(int i, int j) const { return t0[n() + by5(i, j)]; }
    __device__ __forceinline__ double &m1(int i, int j) const { return t0[2 * n() + by3(i, j)]; }
    __device__ __forceinline__ double &co(int i, int j) const { return t0[3 * n() + by5(i, j)]; }
    __device__ __forceinline__ double &mo(int i, int j) const { return t0[4 * n() + by5(i, j)]; }
    __device__ __forceinline__ double &m1o(int i, int j) const { return t0[5 * n() + by3(i, j)]; }
    __device__ __forceinline__ int hi(int i) const { return min(L, i + W); }
    __device__ __forceinline__ int lo(int j) const { return max(0, j - W + 1); }
    __device__ __forceinline__ bool has(int p, int q) const { return q - p < W; }
};
__device__ __forceinline__ PfTabBand pf_span_view(const PfSpanSeq &q, double *tabs)
{
    return PfTabBand{tabs + q.tab_off, q.L, q.W};
}

// the aux arrays of a sequence
struct PfSpanAux {
    double *ps, *pb, *mF, *mFr, *unp;
    int *eF, *eFr;
};
__device__ __forceinline__ PfSpanAux pf_span_aux(const PfSpanSeq &q, double *aux, int *exps)
{
    double *ps = aux + q.aux_off, *pb = ps + q.W + 2, *mF = pb + q.W + 2, *mFr = mF + q.L + 1;
    int *eF = exps + q.exp_off;
    return PfSpanAux{ps, pb, mF, mFr, mFr + q.L + 1, eF, eF + q.L + 1};
}

// ps[n] = scale^-n and pb[n] = (b / scale)^n, n = 0 .. W + 1, by repeated multiplication
__global__ __launch_bounds__(64) void pf_span_powers_kernel(const EnergyTables *ET, const PfSpanSeq *seqs, int n_seq, double *aux, double beta)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seq) return;
    const PfSpanSeq q = seqs[s];
    if (q.L == 0) return;
    double *ps = aux + q.aux_off, *pb = ps + q.W + 2;
    const double inv = 1.0 / q.scale, binv = pf_w(ET->s.ml_base, beta) * inv;
    ps[0] = pb[0] = 1.0;
    for (int n = 1; n <= q.W + 1; n++) { ps[n] = ps[n - 1] * inv; pb[n] = pb[n - 1] * binv; }
}

// anti-diagonal d of the sequences order[0 .. gridDim.y), four cells per workgroup and round.  Besides pf_cell's three tables, what
// the exterior sums read of the cell: C w(exterior stem), by the 5' end into the Co table and by the 3' end into the M1o table -
// the outside pass writes every cell of both before it reads it
__global__ __launch_bounds__(PF_NT) void pf_span_diag_kernel(const EnergyTables *ET, const PfSpanSeq *seqs, const int *order, const uint8_t *codes, double *tabs,
                                                             const double *aux, double beta, int d)
{
    const PfSpanSeq q = seqs[order[blockIdx.y]];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= q.W) return;
    const PfTabBand tb = pf_span_view(q, tabs);
    const uint8_t *S = codes + q.code_off;
    const double *ps = aux + q.aux_off, *pb = ps + q.W + 2;
    const SmallT *T = &ET->s;
    for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) {
        const int j = i + d;
        pf_cell(tb, MfeConNone(), T, &ET->b, S, L, ps, pb, beta, i, j, lane);
        if (lane == 0) {
            const double c = tb.c(i, j);
            const double x = c != 0.0 ? c * pf_w(mfe_stem_ext(T, S, L, i, j), beta) : 0.0;
            tb.co(i, j) = x; tb.m1o(i, j) = x;
        }
    }
}

// A sum of positive terms in an extended range: m 2^e, e = PFX_NONE while it is empty.  add() takes a plain double t and the
// exponent te its unit has (the term is t 2^te); the sum's unit follows its largest term, so a term far below it flushes to 0 in
// ldexp and no term lies above the unit it is added in.
#define PFX_NONE (-(1 << 29))
struct PfX {
    double m;
    int e;
    __device__ __forceinline__ void add(double t, int te)
    {
        if (t == 0.0) return;
        const double f = __builtin_amdgcn_frexp_mant(t);       // (frexp through a pointer costs a stack slot)
        te += __builtin_amdgcn_frexp_exp(t);
        if (te > e) { m = (e == PFX_NONE ? 0.0 : ldexp(m, e - te)) + f; e = te; }
        else m += ldexp(f, te - e);
    }
};
// the sum of the 64 lanes' sums, as a mantissa in [1, 2) and its exponent, the same bits in every lane (lane 0 holds a term)
__device__ __forceinline__ void pfx_wave_sum(const PfX &a, double &m, int &e)
{
    int top = a.e;
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    const double v = pf_wave_sum(a.e == PFX_NONE ? 0.0 : ldexp(a.m, a.e - top));
    m = 2.0 * __builtin_amdgcn_frexp_mant(v);
    e = top + __builtin_amdgcn_frexp_exp(v) - 1;
}

// One pass of the exterior sums of one sequence, n steps: value[k + 1] = value[k] / scale + sum over d = 4 .. min(k, W - 1) of
// value[k - d] X(k, d), value[0] = 1.  The last PF_SPAN_RING values live in the LDS ring rm / re (W <= PF_SPAN_RING: the slot step
// k + 1 writes is that of value[k + 1 - PF_SPAN_RING], which is read, if at all, earlier in the same step); every value goes to
// gm / ge.  FWD: the values are F, X(k, d) is row k of the table by the 3' end; else they are Fr counted from the 3' end (value[k]
// = Fr[L - k]) and X(k, d) is row L - 1 - k of the table by the 5' end.  The first round of step k + 1 is fetched while step k is
// reduced.
template <bool FWD>
__device__ inline void pf_span_exterior_pass(const double *X, int L, int W, double inv, double *rm, int *re, double *gm, int *ge, int lane)
{
    auto row = [&](int k) { return X + (size_t)(FWD ? k : L - 1 - k) * W; };
    auto out = [&](int k) { return FWD ? k : L - k; };
    if (lane == 0) { rm[0] = 1.0; re[0] = 0; gm[out(0)] = 1.0; ge[out(0)] = 0; }
    wave_sync();
    double nx = 0.0;
    for (int k = 0; k < L; k++) {
        const int dmax = min(W - 1, k);
        const double *xr = row(k);
        const double cur = nx;
        nx = k + 1 < L && 4 + lane <= min(W - 1, k + 1) ? row(k + 1)[4 + lane] : 0.0;
        PfX acc{0.0, PFX_NONE};
        if (lane == 0) acc.add(rm[k & (PF_SPAN_RING - 1)] * inv, re[k & (PF_SPAN_RING - 1)]);
        if (cur != 0.0) { const int at = (k - 4 - lane) & (PF_SPAN_RING - 1); acc.add(rm[at] * cur, re[at]); }
        for (int d = 4 + 64 + lane; d <= dmax; d += 64) {
            const double x = xr[d];
            if (x != 0.0) { const int at = (k - d) & (PF_SPAN_RING - 1); acc.add(rm[at] * x, re[at]); }
        }
        double m; int e;
        pfx_wave_sum(acc, m, e);
        wave_sync();                                // every lane has read the ring
        if (lane == 0) { rm[(k + 1) & (PF_SPAN_RING - 1)] = m; re[(k + 1) & (PF_SPAN_RING - 1)] = e; gm[out(k + 1)] = m; ge[out(k + 1)] = e; }
        wave_sync();
    }
}

// One wavefront per sequence: the exterior sums from both ends (F[j + 1]: positions 0..j; Fr[i]: positions i..L-1) in the extended
// range, the ensemble free energy -kT (ln m_Z + e_Z ln 2 + L ln scale), the share of the span MFE structure, the range check, and
// the all-dot row the centroid is written into.  The range check: the mantissa of Z is finite and positive (a band cell that left
// the range upwards makes it inf or nan), and Z is not below the weight of the MFE structure (band cells that left it downwards
// lose that structure first: F itself cannot underflow any more, so Z = 0 no longer shows it).
__global__ __launch_bounds__(64) void pf_span_exterior_kernel(const PfSpanSeq *seqs, const int *order, double *tabs, double *aux, int *exps, double kt, char *db, PfRec *rec)
{
    __shared__ double rm[PF_SPAN_RING];
    __shared__ int re[PF_SPAN_RING];
    const int s = order[blockIdx.x], lane = (int)threadIdx.x;
    const PfSpanSeq q = seqs[s];
    const int L = q.L, W = q.W;
    const PfTabBand tb = pf_span_view(q, tabs);
    const PfSpanAux a = pf_span_aux(q, aux, exps);
    const double inv = a.ps[1];
    pf_span_exterior_pass<true>(tb.tab(5), L, W, inv, rm, re, a.mF, a.eF, lane);
    const double mz = rm[L & (PF_SPAN_RING - 1)];
    const int ez = re[L & (PF_SPAN_RING - 1)];
    wave_sync();
    pf_span_exterior_pass<false>(tb.tab(3), L, W, inv, rm, re, a.mFr, a.eFr, lane);
    char *row = db + q.db_off;
    for (int x = lane; x < L; x += 64) row[x] = '.';
    if (lane == 0) {
        row[L] = 0;
        double energy = 0.0, share = 0.0;
        bool held = isfinite(mz) && mz > 0.0;
        if (held) {
            energy = -kt * (log(mz) + (double)ez * 0.693147180559945309417 + (double)L * q.ln_scale);
            share = exp((energy - (double)q.mfe_dcal / 100.0) / kt);
            held = share <= 1.0 + 1e-9;
        }
        rec[s].status = held ? 0 : RAFFT_ERR_CAPACITY;              // (n_pairs and bad stay 0 from the driver's memset)
        rec[s].energy = held ? energy : 0.0;
        rec[s].mfe_frequency = held ? share : 0.0;
    }
}

// the exterior sums as pf_out_cell reads them, divided by 2^e_Z: m_F[i] w m_Fr[j + 1] shifted by e_F[i] + e_Fr[j + 1] - e_Z
struct PfExtScaled {
    const double *mF;               // Fr's mantissas and exponents lie L + 1 behind F's
    const int *eF;
    int L, ez;
    __device__ __forceinline__ double operator()(int i, int j, double w) const { return ldexp(mF[i] * w * mF[L + j + 2], eF[i] + eF[L + j + 2] - ez); }
};

__global__ __launch_bounds__(PF_NT) void pf_span_out_diag_kernel(const EnergyTables *ET, const PfSpanSeq *seqs, const int *order, const uint8_t *codes, double *tabs,
                                                                 const double *aux, const int *exps, double beta, int d)
{
    __shared__ double wcl[PF_NCLOSE];
    const PfSpanSeq q = seqs[order[blockIdx.y]];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= q.W) return;
    const double *ps = aux + q.aux_off, *pb = ps + q.W + 2;
    const int *eF = exps + q.exp_off;
    const SmallT *T = &ET->s;
    pf_fill_wcl(wcl, T, beta, ps[2]);
    const PfTabBand tb = pf_span_view(q, tabs);
    const uint8_t *S = codes + q.code_off;
    const PfExtScaled ex{pb + q.W + 2, eF, L, eF[L]};
    for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) pf_out_cell(tb, MfeConNone(), T, &ET->b, S, L, ps, pb, ex, wcl, beta, i, i + d, lane);
}

// P(i, i + d) = C Co / m_Z into the Mo table as [i][d], which then has the shape of the caller's banded buffer (0 below d = 4 and
// beyond the sequence); the centroid row, every pair with P > 0.5; and unpaired[i] = 1 - sum_j P(i,j) - sum_h P(h,i), clamped to
// [0, 1].  One wavefront per position and round.  The pairs (h,i) lie in other rows, which other wavefronts fill: P goes into Mo and
// not over Co so that they can be formed again here from C and Co, the same bits.  Either sum is taken lane by lane over d = 4 +
// lane + 64 r ascending, then by pf_wave_sum: an order that L and W fix.
__global__ __launch_bounds__(PF_NT) void pf_span_prob_kernel(const PfSpanSeq *seqs, const int *order, double *tabs, double *aux, int *exps, char *db, PfRec *rec)
{
    const int s = order[blockIdx.y];
    const PfSpanSeq q = seqs[s];
    const int L = q.L, W = q.W, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PfTabBand tb = pf_span_view(q, tabs);
    const PfSpanAux a = pf_span_aux(q, aux, exps);
    const bool ok = rec[s].status == 0;
    const double mz = a.mF[L];
    char *row = db + q.db_off;
    for (int i = blockIdx.x * (PF_NT / 64) + wave; i < L; i += gridDim.x * (PF_NT / 64)) {
        double right = 0.0, left = 0.0;
        for (int d = lane; d < W; d += 64) {
            const int j = i + d;
            double p = 0.0;
            if (ok && d >= 4 && j < L) {
                p = tb.c(i, j) * tb.co(i, j) / mz;
                if (!isfinite(p)) { p = 0.0; atomicMax(&rec[s].bad, 1); }
                if (p > 0.5) { row[i] = '('; row[j] = ')'; atomicAdd(&rec[s].n_pairs, 1); }
            }
            tb.tab(4)[(size_t)i * W + d] = p;
            right += p;
        }
        if (ok)
            for (int d = 4 + lane; d < W && d <= i; d += 64) {
                const double p = tb.c(i - d, i) * tb.co(i - d, i) / mz;
                if (isfinite(p)) left += p;
            }
        const double u = 1.0 - pf_wave_sum(right) - pf_wave_sum(left);
        if (lane == 0) a.unp[i] = ok ? fmin(1.0, fmax(0.0, u)) : 0.0;
    }
}
