// rafft_pf.hip - partition function and base-pair probabilities of a batch (gfx950): McCaskill's sums in scaled fp64 over the
// ensemble rafft_mfe.hip minimises over, with the loop energies of rafft_device.h through the helpers the MFE kernels call
// (mfe_stem_ml, mfe_stem_ext, mfe_ml_close, the mfe_il candidate table): the energy model is not stated again.
// DESIGN.md section 10.  Included by rafft_api.hip, after rafft_mfe.hip.
//
// With w(e) = exp(-e / (100 kT)) and b = w(ml_base):
//   C[i][j]   (i,j) pair: w(hairpin) + sum over inner pairs (p,q), n1 + n2 <= 30, of w(interior) C[p][q]
//             + w(ml_closing + stem(closing pair, read from inside)) sum_k M[i+1][k-1] M1[k][j-1]
//   M1[i][j]  exactly one stem, starting at i, ending at or before j: C[i][j] w(stem(i,j)) + M1[i][j-1] b
//   M[i][j]   at least one stem in i..j: sum_{k=i..j} (b^(k-i) + M[i][k-1]) M1[k][j] - the LAST stem starts at k; before it
//             nothing but unpaired bases, or at least one stem
//   F[j]      exterior loop of 0..j: F[j-1] + sum_i F[i-1] C[i][j] w(stem_ext(i,j)), F[-1] = 1, Z = F[L-1]; Fr the same from the 3' end
// This grammar derives every structure exactly once.  The MFE's M (rafft_mfe.hip) reaches "i unpaired, two stems" both through
// M[i+1][j] + ml_base and through the split - harmless under min, a double count under + - so its M[i+1][j] term is deliberately
// absent here.
// Outside, descending over j - i, one variable per inside one; within a cell Mo, then M1o (reads Mo of the cell), then Co (reads M1o):
//   Mo[i][j]  = sum_{q>j+1} Co[i-1][q] w(close(i-1,q)) M1[j+1][q-1] + sum_{q>j} Mo[i][q] M1[j+1][q]
//   M1o[k][j] = b M1o[k][j+1] + sum_{i<k} Co[i][j+1] w(close(i,j+1)) M[i+1][k-1] + sum_{i<=k} Mo[i][j] (b^(k-i) + M[i][k-1])
//   Co[i][j]  = F[i-1] w(stem_ext(i,j)) Fr[j+1] + sum over enclosing pairs (p,q), n1 + n2 <= 30, of Co[p][q] w(interior)
//               + w(stem(i,j)) M1o[i][j]
//   P(i,j)    = C[i][j] Co[i][j] / Z
// (b M1o[k][j+1] carries "the stem ends at j, the bases up to j' are unpaired" one step at a time instead of a sum over j'.)
// Scaling: an inside cell holds its value divided by scale^(j-i+1), an outside cell by scale^(L-(j-i+1)), F[j] by scale^(j+1), Fr[i]
// by scale^(L-i): every term is multiplied by scale^-(positions it covers itself), read from the per-sequence powers ps[n] =
// scale^-n and pb[n] = (b / scale)^n.  In P the scales cancel.
// One size class: full L x L fp64 tables in device memory, one launch per anti-diagonal (stream order is the synchronisation),
// one wavefront per cell, candidates over the 64 lanes, summed by a butterfly of fixed order.
// pf_cell and pf_out_cell are templates over a table view, so that rafft_pf_span.hip runs them over L x W tables (DESIGN.md
// section 19); the kernels of this file use the full view PfTab.
// They, and the exterior sums, also take a constraint policy of rafft_mfe.hip beside the view: MfeConNone
// compiles away - every new factor stands under `if constexpr (Con::on)`, so the plain kernels keep the parent's code -, MfeConPack
// removes candidates and puts the soft terms into the loop energies before pf_w.  The pf_con_* kernels are the three passes again
// with a pack per sequence in device memory, for rafft_pf_constrained_batch.
#pragma once

#include "rafft_batch_layout.h"     // PfSeq, PfRec

#define PF_NT 256
#define PF_NCLOSE 175               // (pair type, base before the 3' end, base after the 5' end) of a closing pair

// C, M and their outside twins by rows, M1 and M1o by columns (as MfeTabHbm).  pf_cell and pf_out_cell are templates over such a
// view; besides the six cell accessors a view says which cells it has: hi(i), one past the largest q of a cell (i,q); lo(j), the
// smallest h of a cell (h,j); has(p,q).  This one, the full view, has every cell of the sequence (PfTabBand of rafft_pf_span.hip:
// the cells with q - p < W).  The outside sums run over hi / lo / has and read no cell the view does not have; the inside sums of a
// cell (i,j) stay within (i,j) and need no bound.
struct PfTab {
    double *C, *M, *M1T, *Co, *Mo, *M1oT;
    int L;
    __device__ __forceinline__ int hi(int) const { return L; }
    __device__ __forceinline__ int lo(int) const { return 0; }
    __device__ __forceinline__ bool has(int, int) const { return true; }
    __device__ __forceinline__ double &c(int i, int j) const { return C[(size_t)i * L + j]; }
    __device__ __forceinline__ double &m(int i, int j) const { return M[(size_t)i * L + j]; }
    __device__ __forceinline__ double &m1(int i, int j) const { return M1T[(size_t)j * L + i]; }
    __device__ __forceinline__ double &co(int i, int j) const { return Co[(size_t)i * L + j]; }
    __device__ __forceinline__ double &mo(int i, int j) const { return Mo[(size_t)i * L + j]; }
    __device__ __forceinline__ double &m1o(int i, int j) const { return M1oT[(size_t)j * L + i]; }
};
__device__ __forceinline__ PfTab pf_tab(double *t0, int L)
{
    const size_t LL = (size_t)L * L;
    return PfTab{t0, t0 + LL, t0 + 2 * LL, t0 + 3 * LL, t0 + 4 * LL, t0 + 5 * LL, L};
}

// sum over the 64 lanes of a wavefront (all of them active), the same bits in every lane: a butterfly, partner distance 32 .. 1
__device__ __forceinline__ double pf_wave_sum(double x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ double pf_w(int e, double beta) { return exp(-(double)e * beta); }

// ps[n] = scale^-n and pb[n] = (b / scale)^n, n = 0..L, by repeated multiplication
__global__ __launch_bounds__(64) void pf_powers_kernel(const EnergyTables *ET, const PfSeq *seqs, int n_seq, double *aux, double beta)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seq) return;
    const PfSeq q = seqs[s];
    if (q.L == 0) return;
    double *ps = aux + q.aux_off, *pb = ps + q.L + 1;
    const double inv = 1.0 / q.scale, binv = pf_w(ET->s.ml_base, beta) * inv;
    ps[0] = pb[0] = 1.0;
    for (int n = 1; n <= q.L; n++) { ps[n] = ps[n - 1] * inv; pb[n] = pb[n - 1] * binv; }
}

// the weight of leaving k, and of leaving a..b, unpaired, beside the factor `w` those positions have without constraints (pb[1],
// pb[n], 1 / scale): 0 where the constraints forbid it, else w times the weight of the soft terms - w itself, to the bit, when
// these are 0.  Only under a policy that is on; MfeConNone keeps the plain factor
template <class Con>
__device__ __forceinline__ double pf_up_w(const Con &cn, int k, double w, double beta)
{
    if constexpr (!Con::on) return w;
    else return cn.up(k) ? w * pf_w(cn.u(k), beta) : 0.0;
}
template <class Con>
__device__ __forceinline__ double pf_free_w(const Con &cn, int a, int b, double w, double beta)
{
    if constexpr (!Con::on) return w;
    else return cn.free(a, b) ? w * pf_w(cn.U(a, b), beta) : 0.0;
}

// MfeConNone for a sequence without a pack in the pf_con_* kernels: a type of its own, so that the instantiations the plain kernels
// inline keep their one caller, and with it their code to the instruction
struct PfConAbsent : MfeConNone {};

// one wavefront fills cell (i,j) of the three inside tables; every cell of a smaller j - i is there.  cn: the constraint policy of
// rafft_mfe.hip; a candidate it removes adds 0.0 and its lane stays in the butterfly
template <class TB, class Con>
__device__ inline void pf_cell(const TB &tb, const Con &cn, const SmallT *T, const BigT *B, const uint8_t *S, int L, const double *ps, const double *pb,
                               double beta, int i, int j, int lane)
{
    const int d = j - i;
    double c = 0.0, m1 = 0.0, m = 0.0;
    if (d >= 4) {
        int t = pair_type(S[i], S[j]);
        if constexpr (Con::on) { if (!cn.ok(i, j)) t = 0; }
        if (t) {
            double acc = 0.0;
            if constexpr (Con::on) { if (lane == 0 && cn.free(i + 1, j - 1)) acc = pf_w(e_hairpin(T, B, d - 1, t, S, i, j) + cn.U(i + 1, j - 1), beta) * ps[d + 1]; }
            else if (lane == 0) acc = pf_w(e_hairpin(T, B, d - 1, t, S, i, j), beta) * ps[d + 1];
            for (int x = lane; x < MFE_NIL; x += 64) {
                const int n12 = mfe_il.v[x], n1 = n12 >> 8, n2 = n12 & 255, p = i + 1 + n1, q = j - 1 - n2;
                if (q - p < 4) continue;
                const int t2 = pair_type(S[p], S[q]);
                if (!t2) continue;
                const double cc = tb.c(p, q);
                if (cc == 0.0) continue;
                int g = 0;
                if constexpr (Con::on) {
                    if (!cn.free(i + 1, p - 1) || !cn.free(q + 1, j - 1)) continue;
                    acc += pf_w(e_intloop(T, B, n1, n2, t, rtype(t2), S[i + 1], S[j - 1], S[p - 1], S[q + 1], g) + mfe_interior_soft(cn, i, j, p, q), beta) * ps[n1 + n2 + 2] * cc;
                } else
                    acc += pf_w(e_intloop(T, B, n1, n2, t, rtype(t2), S[i + 1], S[j - 1], S[p - 1], S[q + 1], g), beta) * ps[n1 + n2 + 2] * cc;
            }
            double ml = 0.0;                        // a stem takes five positions: k - 1 >= i + 5, k <= j - 5
            for (int k = i + 6 + lane; k <= j - 5; k += 64) ml += tb.m(i + 1, k - 1) * tb.m1(k, j - 1);
            acc += ml * (pf_w(mfe_ml_close(T, S, i, j, t), beta) * ps[2]);
            c = pf_wave_sum(acc);
            m1 = c * pf_w(mfe_stem_ml(T, S, L, i, j), beta);
        }
        m1 += tb.m1(i, j - 1) * pf_up_w(cn, j, pb[1], beta);
        double sp = 0.0;                            // the last stem starts at k > i (k = i is m1 itself)
        for (int k = i + 1 + lane; k <= j - 4; k += 64) {
            double left = pf_free_w(cn, i, k - 1, pb[k - i], beta);
            if (k - 1 - i >= 4) left += tb.m(i, k - 1);
            sp += left * tb.m1(k, j);
        }
        m = m1 + pf_wave_sum(sp);
    }
    if (lane == 0) { tb.c(i, j) = c; tb.m1(i, j) = m1; tb.m(i, j) = m; }
}

// anti-diagonal d of the sequences order[0 .. gridDim.y), four cells per workgroup and round
__global__ __launch_bounds__(PF_NT) void pf_diag_kernel(const EnergyTables *ET, const PfSeq *seqs, const int *order, const uint8_t *codes, double *tabs,
                                                        const double *aux, double beta, int d)
{
    const PfSeq q = seqs[order[blockIdx.y]];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= L) return;
    const PfTab tb = pf_tab(tabs + q.tab_off, L);
    const uint8_t *S = codes + q.code_off;
    const double *ps = aux + q.aux_off, *pb = ps + L + 1;
    for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) pf_cell(tb, MfeConNone(), &ET->s, &ET->b, S, L, ps, pb, beta, i, i + d, lane);
}
// the same under constraints: con_off[s] is where the sequence's pack lies in `packs`; MFE_CON_NONE: it has
// none and takes the code of pf_diag_kernel - a branch that is uniform for the workgroup
__global__ __launch_bounds__(PF_NT) void pf_con_diag_kernel(const EnergyTables *ET, const PfSeq *seqs, const int *order, const uint8_t *codes,
                                                            const unsigned long long *con_off, const int *packs, double *tabs, const double *aux, double beta, int d)
{
    const int s = order[blockIdx.y];
    const PfSeq q = seqs[s];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= L) return;
    const PfTab tb = pf_tab(tabs + q.tab_off, L);
    const uint8_t *S = codes + q.code_off;
    const double *ps = aux + q.aux_off, *pb = ps + L + 1;
    const unsigned long long co = con_off[s];
    if (co != MFE_CON_NONE) {
        const MfeConPack cn(packs + co, L);
        for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) pf_cell(tb, cn, &ET->s, &ET->b, S, L, ps, pb, beta, i, i + d, lane);
    } else {
        for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) pf_cell(tb, PfConAbsent(), &ET->s, &ET->b, S, L, ps, pb, beta, i, i + d, lane);
    }
}

// One wavefront per sequence: the exterior sums from both ends (F[j + 1]: positions 0..j; Fr[i]: positions i..L-1), the ensemble
// free energy, the share of the MFE structure, the range check, and the all-dot row the centroid is written into
template <class Con>
__device__ inline void pf_exterior(const Con &cn, const EnergyTables *ET, const PfSeq &q, int s, const uint8_t *codes, double *tabs, double *aux, double beta,
                                   double kt, char *db, PfRec *rec, double *F)
{
    const int lane = (int)threadIdx.x;
    const int L = q.L;
    const PfTab tb = pf_tab(tabs + q.tab_off, L);
    const SmallT *T = &ET->s;
    const uint8_t *S = codes + q.code_off;
    double *ps = aux + q.aux_off, *gF = ps + 2 * (L + 1), *gFr = gF + L + 1;
    const double inv = ps[1];
    if (lane == 0) F[0] = 1.0;
    wave_sync();
    for (int j = 0; j < L; j++) {
        double acc = 0.0;
        for (int i = lane; i <= j - 4; i += 64) {
            const double c = tb.c(i, j);
            if (c != 0.0) acc += F[i] * c * pf_w(mfe_stem_ext(T, S, L, i, j), beta);
        }
        acc = pf_wave_sum(acc);
        if constexpr (Con::on) { if (lane == 0) F[j + 1] = F[j] * pf_up_w(cn, j, inv, beta) + acc; }
        else if (lane == 0) F[j + 1] = F[j] * inv + acc;
        wave_sync();
    }
    const double z = F[L];
    for (int x = lane; x <= L; x += 64) gF[x] = F[x];
    wave_sync();
    if (lane == 0) F[L] = 1.0;
    wave_sync();
    for (int i = L - 1; i >= 0; i--) {
        double acc = 0.0;
        for (int j = i + 4 + lane; j < L; j += 64) {
            const double c = tb.c(i, j);
            if (c != 0.0) acc += c * pf_w(mfe_stem_ext(T, S, L, i, j), beta) * F[j + 1];
        }
        acc = pf_wave_sum(acc);
        if constexpr (Con::on) { if (lane == 0) F[i] = F[i + 1] * pf_up_w(cn, i, inv, beta) + acc; }
        else if (lane == 0) F[i] = F[i + 1] * inv + acc;
        wave_sync();
    }
    for (int x = lane; x <= L; x += 64) gFr[x] = F[x];
    char *row = db + q.db_off;
    for (int x = lane; x < L; x += 64) row[x] = '.';
    if (lane == 0) {
        row[L] = 0;
        PfRec r{};
        if (isfinite(z) && z > 0.0) {
            r.energy = -kt * (log(z) + (double)L * q.ln_scale);
            r.mfe_frequency = exp((r.energy - (double)q.mfe_dcal / 100.0) / kt);
        } else {
            r.status = RAFFT_ERR_CAPACITY;
        }
        rec[s] = r;
    }
}
__global__ __launch_bounds__(64) void pf_exterior_kernel(const EnergyTables *ET, const PfSeq *seqs, const int *order, const uint8_t *codes, double *tabs,
                                                         double *aux, double beta, double kt, char *db, PfRec *rec)
{
    __shared__ double F[RAFFT_MFE_MAX_LEN + 2];
    const int s = order[blockIdx.x];
    const PfSeq q = seqs[s];
    pf_exterior(MfeConNone(), ET, q, s, codes, tabs, aux, beta, kt, db, rec, F);
}
// the same under constraints, as pf_con_diag_kernel
__global__ __launch_bounds__(64) void pf_con_exterior_kernel(const EnergyTables *ET, const PfSeq *seqs, const int *order, const uint8_t *codes,
                                                             const unsigned long long *con_off, const int *packs, double *tabs, double *aux, double beta, double kt,
                                                             char *db, PfRec *rec)
{
    __shared__ double F[RAFFT_MFE_MAX_LEN + 2];
    const int s = order[blockIdx.x];
    const PfSeq q = seqs[s];
    const unsigned long long co = con_off[s];
    if (co != MFE_CON_NONE) pf_exterior(MfeConPack(packs + co, q.L), ET, q, s, codes, tabs, aux, beta, kt, db, rec, F);
    else pf_exterior(PfConAbsent(), ET, q, s, codes, tabs, aux, beta, kt, db, rec, F);
}

// the exterior sums as pf_out_cell reads them: F[i] w Fr[j + 1], the weight of the exterior loop around a stem (i,j) of weight w
struct PfExtPlain {
    const double *gF, *gFr;
    __device__ __forceinline__ double operator()(int i, int j, double w) const { return gF[i] * w * gFr[j + 1]; }
};

// w(close) scale^-2 by (type of the closing pair, the base before its 3' end, the base after its 5' end), by a workgroup of PF_NT
__device__ inline void pf_fill_wcl(double *wcl, const SmallT *T, double beta, double ps2)
{
    for (int x = threadIdx.x; x < PF_NCLOSE; x += PF_NT) {
        const int t = x / 25;
        wcl[x] = t ? pf_w(T->ml_closing + e_stem(T, rtype(t), (x / 5) % 5, x % 5, false), beta) * ps2 : 0.0;
    }
    __syncthreads();
}

// one wavefront fills cell (i,j) of the three outside tables; every cell of a larger j - i that the view has is there.  wcl: the
// table of pf_fill_wcl; ex: the exterior sums; cn: as pf_cell.  Co of a pair the constraints remove is 0: a weight there would
// leak into the pairs inside it
template <class TB, class EX, class Con>
__device__ inline void pf_out_cell(const TB &tb, const Con &cn, const SmallT *T, const BigT *B, const uint8_t *S, int L, const double *ps, const double *pb,
                                   const EX &ex, const double *wcl, double beta, int i, int j, int lane)
{
    double a = 0.0;
    if (i >= 1)
        for (int q = j + 6 + lane, qe = tb.hi(i - 1); q < qe; q += 64) {
            const double x = tb.co(i - 1, q);
            if (x != 0.0) a += x * wcl[(pair_type(S[i - 1], S[q]) * 5 + S[q - 1]) * 5 + S[i]] * tb.m1(j + 1, q - 1);
        }
    for (int q = j + 5 + lane, qe = tb.hi(i); q < qe; q += 64) a += tb.mo(i, q) * tb.m1(j + 1, q);
    const double mo = pf_wave_sum(a);
    a = 0.0;
    for (int h = tb.lo(j) + lane; h < i; h += 64) {
        const double x = tb.mo(h, j);
        if (x == 0.0) continue;
        double left = pb[i - h];
        if constexpr (Con::on) left = pf_free_w(cn, h, i - 1, left, beta);
        if (i - 1 - h >= 4) left += tb.m(h, i - 1);
        a += x * left;
    }
    if (j + 1 < L)
        for (int h = tb.lo(j + 1) + lane; h <= i - 6; h += 64) {
            const double x = tb.co(h, j + 1);
            if (x != 0.0) a += x * wcl[(pair_type(S[h], S[j + 1]) * 5 + S[j]) * 5 + S[h + 1]] * tb.m(h + 1, i - 1);
        }
    double m1o = mo + pf_wave_sum(a);
    if (j + 1 < L && tb.has(i, j + 1)) {
        if constexpr (Con::on) m1o += pf_up_w(cn, j + 1, pb[1], beta) * tb.m1o(i, j + 1);
        else m1o += pb[1] * tb.m1o(i, j + 1);
    }
    double co = 0.0;
    int t = pair_type(S[i], S[j]);
    if constexpr (Con::on) { if (!cn.ok(i, j)) t = 0; }
    if (t) {
        a = 0.0;
        if (lane == 0) a = ex(i, j, pf_w(mfe_stem_ext(T, S, L, i, j), beta)) + pf_w(mfe_stem_ml(T, S, L, i, j), beta) * m1o;
        for (int x = lane; x < MFE_NIL; x += 64) {
            const int n12 = mfe_il.v[x], n1 = n12 >> 8, n2 = n12 & 255, p = i - 1 - n1, q = j + 1 + n2;
            if (p < 0 || q >= L || !tb.has(p, q)) continue;
            const int t2 = pair_type(S[p], S[q]);
            if (!t2) continue;
            const double cc = tb.co(p, q);
            if (cc == 0.0) continue;
            int g = 0;
            if constexpr (Con::on) {
                if (!cn.free(p + 1, i - 1) || !cn.free(j + 1, q - 1)) continue;
                a += cc * pf_w(e_intloop(T, B, n1, n2, t2, rtype(t), S[p + 1], S[q - 1], S[i - 1], S[j + 1], g) + mfe_interior_soft(cn, p, q, i, j), beta) * ps[n1 + n2 + 2];
            } else
                a += cc * pf_w(e_intloop(T, B, n1, n2, t2, rtype(t), S[p + 1], S[q - 1], S[i - 1], S[j + 1], g), beta) * ps[n1 + n2 + 2];
        }
        co = pf_wave_sum(a);
    }
    if (lane == 0) { tb.mo(i, j) = mo; tb.m1o(i, j) = m1o; tb.co(i, j) = co; }
}

__global__ __launch_bounds__(PF_NT) void pf_out_diag_kernel(const EnergyTables *ET, const PfSeq *seqs, const int *order, const uint8_t *codes, double *tabs,
                                                            const double *aux, double beta, int d)
{
    __shared__ double wcl[PF_NCLOSE];
    const PfSeq q = seqs[order[blockIdx.y]];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= L) return;
    const double *ps = aux + q.aux_off, *pb = ps + L + 1, *gF = pb + L + 1, *gFr = gF + L + 1;
    const SmallT *T = &ET->s;
    pf_fill_wcl(wcl, T, beta, ps[2]);
    const PfTab tb = pf_tab(tabs + q.tab_off, L);
    const uint8_t *S = codes + q.code_off;
    const PfExtPlain ex{gF, gFr};
    for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) pf_out_cell(tb, MfeConNone(), T, &ET->b, S, L, ps, pb, ex, wcl, beta, i, i + d, lane);
}
// the same under constraints, as pf_con_diag_kernel
__global__ __launch_bounds__(PF_NT) void pf_con_out_diag_kernel(const EnergyTables *ET, const PfSeq *seqs, const int *order, const uint8_t *codes,
                                                                const unsigned long long *con_off, const int *packs, double *tabs, const double *aux, double beta, int d)
{
    __shared__ double wcl[PF_NCLOSE];
    const int s = order[blockIdx.y];
    const PfSeq q = seqs[s];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d >= L) return;
    const double *ps = aux + q.aux_off, *pb = ps + L + 1, *gF = pb + L + 1, *gFr = gF + L + 1;
    const SmallT *T = &ET->s;
    pf_fill_wcl(wcl, T, beta, ps[2]);
    const PfTab tb = pf_tab(tabs + q.tab_off, L);
    const uint8_t *S = codes + q.code_off;
    const PfExtPlain ex{gF, gFr};
    const unsigned long long co = con_off[s];
    if (co != MFE_CON_NONE) {
        const MfeConPack cn(packs + co, L);
        for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) pf_out_cell(tb, cn, T, &ET->b, S, L, ps, pb, ex, wcl, beta, i, i + d, lane);
    } else {
        for (int i = blockIdx.x * (PF_NT / 64) + wave; i + d < L; i += gridDim.x * (PF_NT / 64)) pf_out_cell(tb, PfConAbsent(), T, &ET->b, S, L, ps, pb, ex, wcl, beta, i, i + d, lane);
    }
}

// P(i,j) into the Co table, which then has the shape of the caller's buffer (0 below j - i = 4 and below the diagonal), and the
// centroid row: every pair with P > 0.5 - such pairs cannot cross or share a base.  One wavefront per row and round
__global__ __launch_bounds__(PF_NT) void pf_prob_kernel(const PfSeq *seqs, const int *order, double *tabs, const double *aux, char *db, PfRec *rec)
{
    const int s = order[blockIdx.y];
    const PfSeq q = seqs[s];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PfTab tb = pf_tab(tabs + q.tab_off, L);
    const bool ok = rec[s].status == 0;
    const double z = (aux + q.aux_off)[2 * (L + 1) + L];        // F[L]
    char *row = db + q.db_off;
    for (int i = blockIdx.x * (PF_NT / 64) + wave; i < L; i += gridDim.x * (PF_NT / 64))
        for (int j = lane; j < L; j += 64) {
            double p = 0.0;
            if (ok && j - i >= 4) {
                p = tb.c(i, j) * tb.co(i, j) / z;
                if (!isfinite(p)) { p = 0.0; atomicMax(&rec[s].bad, 1); }
                if (p > 0.5) { row[i] = '('; row[j] = ')'; atomicAdd(&rec[s].n_pairs, 1); }
            }
            tb.co(i, j) = p;
        }
}

// Under constraints a pair that every structure holds - a forced pair - has P = 1 up to rounding, and what stands on P
// (rafft_mea_probs_batch) takes no value above 1: the P of a sequence with a pack are held to 1.0.  A sequence without one keeps
// the bits pf_prob_kernel wrote
__global__ __launch_bounds__(PF_NT) void pf_con_clamp_kernel(const PfSeq *seqs, const int *order, const unsigned long long *con_off, double *tabs)
{
    const int s = order[blockIdx.y];
    if (con_off[s] == MFE_CON_NONE) return;
    const PfSeq q = seqs[s];
    const size_t LL = (size_t)q.L * q.L;
    double *P = tabs + q.tab_off + 3 * LL;
    for (size_t x = (size_t)blockIdx.x * PF_NT + threadIdx.x; x < LL; x += (size_t)gridDim.x * PF_NT)
        if (P[x] > 1.0) P[x] = 1.0;
}

// unpaired[k] = 1 - sum_j P(k,j) - sum_i P(i,k) from the P table pf_prob_kernel left, into the first L doubles of the sequence's
// aux block (ps is dead by then).  One wavefront per position and round; the sum of a position is taken in an order that L fixes
__global__ __launch_bounds__(PF_NT) void pf_unpaired_kernel(const PfSeq *seqs, const int *order, const double *tabs, double *aux)
{
    const PfSeq q = seqs[order[blockIdx.y]];
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *P = tabs + q.tab_off + 3 * (size_t)L * L;
    double *up = aux + q.aux_off;
    for (int k = blockIdx.x * (PF_NT / 64) + wave; k < L; k += gridDim.x * (PF_NT / 64)) {
        double a = 0.0;
        for (int x = lane; x < L; x += 64) a += P[(size_t)k * L + x] + P[(size_t)x * L + k];
        a = pf_wave_sum(a);
        if (lane == 0) up[k] = 1.0 - a;
    }
}
