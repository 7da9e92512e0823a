// rafft_sample.hip - structures drawn from the Boltzmann ensemble of a batch (gfx950): a stochastic traceback through the inside
// tables C, M, M1 and the exterior sums F that rafft_pf.hip builds, with the terms of pf_cell / pf_exterior_kernel re-formed through
// the same device functions (e_hairpin, e_intloop over the mfe_il table, mfe_ml_close, mfe_stem_ml, mfe_stem_ext, ps, pb): the
// energy model and the grammar are not stated again.  DESIGN.md section 11.  Included by rafft_api.hip, after rafft_pf.hip.
//
// One wavefront draws one structure.  A pending segment is the exterior loop of 0..j or a cell of C, M1 or M; a CHOICE picks one
// term of the segment's sum with probability term / stored value:
//   u       one uniform per choice: draw t of sample k under the sequence's seed (rafft_rng.h), t counting the sample's choices
//   target  u * (stored value of the cell)
//   rounds  of 64 candidates in ascending candidate index, an inclusive scan over the lanes in a fixed order on top of the running
//           total of the rounds before; the FIRST candidate of non-zero weight whose cumulative weight reaches the target is taken
//   order   F[j+1]:   j unpaired; stems (i,j), i ascending
//           C[i][j]:  hairpin; interior loops in the order of mfe_il (p ascending, then q descending); multiloop splits, k ascending
//           M1[i][j]: j unpaired; the stem (i,j)
//           M[i][j]:  the last stem starts at k, k ascending from i - for each k first "unpaired bases alone before k", then "M[i][k-1]
//                     before k" (one lane holds both; a round covers 64 values of k)
//   cheap candidates first: "j unpaired" of F and of M1 is tested before anything is scanned, so a run of unpaired bases costs one
//           choice of O(1) per base
//   fallback: the re-formed terms add up to the stored value but for the last bits (another summation order), so for u close to 1
//           no candidate may reach the target: then the LAST candidate of non-zero weight is taken.  Either way the candidate taken
//           has a non-zero weight, hence non-zero factors: the traceback only enters cells that hold a structure, and a sample can
//           never leave the ensemble.
// After a multiloop split of C the M1 part (3' side) is traced before the M part; after a choice of M the stem at k is traced at
// once and M[i][k-1] is stacked.  The energy of the sample is the sum of the integer loop energies of the terms taken.
#pragma once

#include "rafft_rng.h"
#include "rafft_batch_layout.h"     // SampleSeq, SAMPLE_NT, RAFFT_SAMPLE_STACK, row_bytes16, seg_stack_words, sample_lds_bytes

static_assert(sample_lds_bytes(RAFFT_MFE_MAX_LEN) <= 64 << 10, "the sampling kernel's LDS fits the default limit");

// inclusive sum over the lanes of a wavefront (all of them active), partner distance 1 .. 32: lane l holds x[0] + ... + x[l], every
// partial sum formed in the same order whatever the data
__device__ __forceinline__ double sample_scan(double x, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// the state of one choice.  A candidate is (index c, half h): h = 1 only for the second term a lane of M holds
struct SamplePick {
    double target, run;             // u * stored value; the total of the rounds done
    int found, found_h;             // the candidate taken, -1 before
    int last, last_h;               // the last candidate of non-zero weight so far, -1 when there is none
};
__device__ __forceinline__ SamplePick sample_pick(double target) { return SamplePick{target, 0.0, -1, 0, -1, 0}; }

// one round: lane l holds candidate (c, 0) of weight wa and (c, 1) of weight wb (0 where there is none).  true: a candidate is taken
__device__ __forceinline__ bool sample_round(SamplePick &p, int c, double wa, double wb, int lane)
{
    const double incl = sample_scan(wa + wb, lane);
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.0;
    const double c1 = p.run + excl + wa, c2 = c1 + wb;
    const bool ha = wa > 0.0 && c1 >= p.target, hb = wb > 0.0 && c2 >= p.target;
    const unsigned long long nz = __ballot(wa > 0.0 || wb > 0.0), hit = __ballot(ha || hb);
    if (hit) {
        const int l = __ffsll((long long)hit) - 1;
        p.found = __shfl(c, l, 64);
        p.found_h = __shfl((int)!ha, l, 64);
        return true;
    }
    if (nz) {
        const int l = 63 - __clzll((long long)nz);
        p.last = __shfl(c, l, 64);
        p.last_h = __shfl((int)(wb > 0.0), l, 64);
    }
    p.run += __shfl(incl, 63, 64);
    return false;
}
// after the last round: the fallback.  false: no candidate has a weight (the cell should not have been entered)
__device__ __forceinline__ bool sample_settle(SamplePick &p)
{
    if (p.found < 0) { p.found = p.last; p.found_h = p.last_h; }
    return p.found >= 0;
}

// candidate c of C[i][j], (i,j) of type t: 0 the hairpin, 1 .. MFE_NIL the interior loops, above them the multiloop splits
// k = i + 6 + (c - MFE_NIL - 1).  Its weight as pf_cell forms it, its loop energy in e, and in (p, q) the inner pair or (k, -1)
__device__ __forceinline__ double sample_c_term(const PfTab &tb, const SmallT *T, const BigT *B, const uint8_t *S, const double *ps, double beta,
                                                int i, int j, int t, int c, int &e, int &p, int &q)
{
    e = 0; p = q = -1;
    if (c == 0) {
        e = e_hairpin(T, B, j - i - 1, t, S, i, j);
        return pf_w(e, beta) * ps[j - i + 1];
    }
    if (c <= MFE_NIL) {
        const int n12 = mfe_il.v[c - 1], n1 = n12 >> 8, n2 = n12 & 255;
        p = i + 1 + n1; q = j - 1 - n2;
        if (q - p < 4) return 0.0;
        const int t2 = pair_type(S[p], S[q]);
        if (!t2) return 0.0;
        const double cc = tb.c(p, q);
        if (cc == 0.0) return 0.0;
        int g = 0;
        e = e_intloop(T, B, n1, n2, t, rtype(t2), S[i + 1], S[j - 1], S[p - 1], S[q + 1], g);
        return pf_w(e, beta) * ps[n1 + n2 + 2] * cc;
    }
    p = i + 6 + (c - MFE_NIL - 1);
    if (p > j - 5) return 0.0;
    e = mfe_ml_close(T, S, i, j, t);
    return tb.m(i + 1, p - 1) * tb.m1(p, j - 1) * (pf_w(e, beta) * ps[2]);
}

enum { SAMPLE_BAD_STACK = 1, SAMPLE_BAD_CELL = 2 };

// Sample k = blockIdx.x * 4 + wave of sequence order[blockIdx.y].  A sequence whose exterior sum failed the range check (rec.status)
// is skipped.  LDS per wave: the row and the stack of pending segments, words (i | j << 12 | kind << 24).
// The stack cannot overflow: pending segments cover disjoint stretches of the sequence and each of them yields at least one pair
// with a hairpin of three, five positions of its own - at most L / 5 are pending, the stack holds L / 5 + 2 words, and a push
// beyond them is not carried out (bad = SAMPLE_BAD_STACK ends the sample; the driver reports an internal error).
__global__ __launch_bounds__(SAMPLE_NT) void sample_kernel(const EnergyTables *ET, const PfSeq *seqs, const int *order, const uint8_t *codes, double *tabs,
                                                           const double *aux, double beta, const PfRec *rec, const SampleSeq *smp, int n_samples,
                                                           int lds_len, char *rows, int *dcal, int *bad_out)
{
    extern __shared__ __align__(16) unsigned char sample_lds[];
    const int s = order[blockIdx.y], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * (SAMPLE_NT / 64) + wave;
    if (k >= n_samples || rec[s].status) return;                    // (no workgroup barrier below)
    const PfSeq q = seqs[s];
    const unsigned long long seed = smp[s].seed;
    const int L = q.L;
    if (L > lds_len) return;                                        // (the driver sizes the LDS for the longest sequence of the launch)
    const PfTab tb = pf_tab(tabs + q.tab_off, L);
    const SmallT *T = &ET->s;
    const BigT *B = &ET->b;
    const uint8_t *S = codes + q.code_off;
    const double *ps = aux + q.aux_off, *pb = ps + L + 1, *F = pb + L + 1;      // F[x]: exterior sum of 0..x-1
    unsigned char *row = sample_lds + (size_t)wave * (row_bytes16(lds_len) + 4 * seg_stack_words(lds_len));
    uint32_t *stack = (uint32_t *)(row + row_bytes16(lds_len));
    const int cap = RAFFT_SAMPLE_STACK(L), mlb = T->ml_base;
    for (int x = lane; x < L; x += 64) row[x] = '.';
    if (lane == 0) row[L] = 0;
    wave_sync();
    int sp = 0, bad = 0, energy = 0;
    uint32_t t_draw = 0;
    auto push = [&](int i, int j, int kind) {
        if (sp >= cap) { bad = SAMPLE_BAD_STACK; return; }
        if (lane == 0) stack[sp] = (uint32_t)i | (uint32_t)j << 12 | (uint32_t)kind << 24;
        sp++;
    };
    // the exterior loop, from the 3' end
    for (int j = L - 1; j >= 4 && !bad;) {
        const double target = rafft_uniform(seed, (uint32_t)k, t_draw++) * F[j + 1], w0 = F[j] * ps[1];
        if (w0 > 0.0 && w0 >= target) { j--; continue; }
        SamplePick pk = sample_pick(target);
        pk.run = w0;
        for (int i0 = 0; i0 <= j - 4; i0 += 64) {
            const int i = i0 + lane;
            double w = 0.0;
            if (i <= j - 4) {
                const double c = tb.c(i, j);
                if (c != 0.0) w = F[i] * c * pf_w(mfe_stem_ext(T, S, L, i, j), beta);
            }
            if (sample_round(pk, i, w, 0.0, lane)) break;
        }
        if (!sample_settle(pk)) {
            if (w0 > 0.0) { j--; continue; }                        // nothing but "j unpaired" has a weight
            bad = SAMPLE_BAD_CELL;
            break;
        }
        energy += mfe_stem_ext(T, S, L, pk.found, j);
        push(pk.found, j, MFE_K_C);
        j = pk.found - 1;
    }
    while (sp > 0 && !bad) {
        sp--;
        uint32_t w = 0;
        if (lane == 0) w = stack[sp];
        w = (uint32_t)__shfl((int)w, 0, 64);
        int i = (int)(w & 4095u), j = (int)((w >> 12) & 4095u), kind = (int)(w >> 24);
        if (kind == MFE_K_M) {
            SamplePick pk = sample_pick(rafft_uniform(seed, (uint32_t)k, t_draw++) * tb.m(i, j));
            for (int k0 = i; k0 <= j - 4; k0 += 64) {
                const int kk = k0 + lane;
                double wa = 0.0, wb = 0.0;
                if (kk <= j - 4) {
                    const double m1 = tb.m1(kk, j);
                    if (m1 != 0.0) {
                        wa = pb[kk - i] * m1;
                        if (kk - 1 - i >= 4) wb = tb.m(i, kk - 1) * m1;
                    }
                }
                if (sample_round(pk, kk, wa, wb, lane)) break;
            }
            if (!sample_settle(pk)) { bad = SAMPLE_BAD_CELL; break; }
            if (pk.found_h) push(i, pk.found - 1, MFE_K_M);
            else energy += (pk.found - i) * mlb;
            i = pk.found; kind = MFE_K_M1;
        }
        if (!bad && kind == MFE_K_M1) {
            for (;;) {
                const double target = rafft_uniform(seed, (uint32_t)k, t_draw++) * tb.m1(i, j);
                const double w0 = tb.m1(i, j - 1) * pb[1];
                if (w0 > 0.0 && w0 >= target) { j--; energy += mlb; continue; }
                const double c = tb.c(i, j);
                if (c != 0.0 && c * pf_w(mfe_stem_ml(T, S, L, i, j), beta) > 0.0) { energy += mfe_stem_ml(T, S, L, i, j); kind = MFE_K_C; break; }
                if (w0 > 0.0) { j--; energy += mlb; continue; }      // the stem has no weight: the fallback
                bad = SAMPLE_BAD_CELL;
                break;
            }
        }
        if (bad || kind != MFE_K_C) continue;
        const int t = pair_type(S[i], S[j]);
        if (!t) { bad = SAMPLE_BAD_CELL; continue; }
        if (lane == 0) { row[i] = '('; row[j] = ')'; }
        SamplePick pk = sample_pick(rafft_uniform(seed, (uint32_t)k, t_draw++) * tb.c(i, j));
        const int n_cand = 1 + MFE_NIL + max(0, j - i - 10);
        int e, p, qq;
        for (int c0 = 0; c0 < n_cand; c0 += 64) {
            const int c = c0 + lane;
            const double wc = c < n_cand ? sample_c_term(tb, T, B, S, ps, beta, i, j, t, c, e, p, qq) : 0.0;
            if (sample_round(pk, c, wc, 0.0, lane)) break;
        }
        if (!sample_settle(pk)) { bad = SAMPLE_BAD_CELL; continue; }
        sample_c_term(tb, T, B, S, ps, beta, i, j, t, pk.found, e, p, qq);       // every lane: the candidate taken
        energy += e;
        if (pk.found == 0) continue;
        if (pk.found <= MFE_NIL) { push(p, qq, MFE_K_C); continue; }
        push(i + 1, p - 1, MFE_K_M);
        push(p, j - 1, MFE_K_M1);
    }
    wave_sync();
    char *out = rows + smp[s].row_off + (size_t)k * (L + 1);
    for (int x = lane; x <= L; x += 64) out[x] = bad ? (x < L ? '.' : 0) : (char)row[x];
    if (lane == 0) {
        dcal[smp[s].dcal_off + k] = bad ? 0 : energy;
        if (bad) atomicMax(&bad_out[s], bad);
    }
}
