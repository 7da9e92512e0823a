// rafft_mfe.hip - minimum-free-energy folds of a batch (gfx950): Zuker's recurrences in integer dcal over the device functions of
// rafft_device.h (e_hairpin, e_intloop, e_stem - the energy model is stated there and nowhere else), and the traceback.
// DESIGN.md section 9.  Included by rafft_api.hip, after rafft_kernels.hip (wave_sync).
//
//   C[i][j]   (i,j) pair: hairpin | interior loop with inner pair (p,q), n1 + n2 <= 30 | multiloop closed by (i,j)
//   M1[i][j]  exactly one stem, starting at i, ending at or before j: min(C[i][j] + stem(i,j), M1[i][j-1] + ml_base)
//   M[i][j]   at least one stem in i..j: min(M1[i][j], M[i+1][j] + ml_base, min_k M[i][k-1] + M1[k][j])
//   F[j]      exterior loop of 0..j: min(F[j-1], min_i F[i-1] + C[i][j] + stem_ext(i,j))
// The value of a cell is the minimum over its candidates, whatever their order.  The traceback visits the candidates of a cell in ONE
// fixed order and takes the first that reproduces the stored value, so the structure is a function of the sequence and the tables:
//   C:  hairpin; interior loops, p ascending then q descending; multiloop splits, k ascending
//   M1: the stem (i,j); j unpaired
//   M:  M1[i][j]; i unpaired; splits, k ascending
//   F:  j unpaired; stems (i,j), i ascending
// Two size classes share mfe_cell and mfe_traceback through a table view: triangular tables in LDS (mfe_lds_kernel, one workgroup per
// sequence, a barrier per anti-diagonal) and full L x L tables in HBM (mfe_diag_kernel, one launch per anti-diagonal: stream order
// is the synchronisation; mfe_traceback_kernel).
// Constraints are a policy handed through mfe_interior, mfe_cell, mfe_exterior and mfe_traceback beside the
// table view: which pairs may close, which ranges may stay unpaired, and what the soft terms add.  MfeConNone allows everything,
// adds nothing and compiles away; MfeConPack reads a sequence's constraint pack (constraint_pack of rafft_hostpure.h).  The
// mfe_con_* kernels are the two size classes again with a pack per sequence, in LDS behind the bases or in device memory.
// A strand break is a second policy beside it: which backbone bonds exist, which cells span the nick and
// what the loop that holds it costs.  MfeCutNone has no nick and compiles away; MfeCut is what rafft_cofold.hip folds dimers under.
#pragma once

#include "rafft_batch_layout.h"     // MfeSeq, RAFFT_MFE_LDS_LEN, MFE_LDS_BYTES, mfe_lds_bytes

#define MFE_INF 1000000000          // "no structure"; two of them still add up inside an int
#define MFE_INFH 500000000          // every real energy lies below, every sum with an MFE_INF above
#define MFE_MAXLOOP 30              // unpaired positions of an interior loop (RNA.fold's default)
#define MFE_NIL 496                 // pairs (n1, n2) with n1 + n2 <= 30
#define MFE_LDS_NT 512
#define MFE_HBM_NT 256

// (n1 << 8 | n2) of interior-loop candidate x: n1 ascending, then n2 ascending - p ascending, then q descending
struct MfeIlTable {
    unsigned short v[MFE_NIL];
    constexpr MfeIlTable() : v()
    {
        int x = 0;
        for (int n1 = 0; n1 <= MFE_MAXLOOP; n1++)
            for (int n2 = 0; n1 + n2 <= MFE_MAXLOOP; n2++) v[x++] = (unsigned short)(n1 << 8 | n2);
    }
};
__constant__ MfeIlTable mfe_il = MfeIlTable();

// table views: c / m / m1 are cell (i, j), i <= j.  The split loops read M along a row (k - 1 varies) and M1 along a column
// (k varies), so M is stored by rows and M1 by columns: the 64 lanes of a split read 64 consecutive words of each.
struct MfeTabLds {
    int *C, *M, *M1;
    int L;
    __device__ __forceinline__ int row(int i, int j) const { return i * L - ((i * (i - 1)) >> 1) + (j - i); }
    __device__ __forceinline__ int col(int i, int j) const { return ((j * (j + 1)) >> 1) + i; }
    __device__ __forceinline__ int &c(int i, int j) const { return C[row(i, j)]; }
    __device__ __forceinline__ int &m(int i, int j) const { return M[row(i, j)]; }
    __device__ __forceinline__ int &m1(int i, int j) const { return M1[col(i, j)]; }
};
struct MfeTabHbm {
    int *C, *M, *M1T;
    int L;
    __device__ __forceinline__ int &c(int i, int j) const { return C[(size_t)i * L + j]; }
    __device__ __forceinline__ int &m(int i, int j) const { return M[(size_t)i * L + j]; }
    __device__ __forceinline__ int &m1(int i, int j) const { return M1T[(size_t)j * L + i]; }
};

// minimum over the 64 lanes of a wavefront (all of them active), the same in every lane: the DPP steps of wave_incl_scan with min
__device__ __forceinline__ int mfe_wave_min(int x)
{
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x111, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x112, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x114, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x118, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x142, 0xA, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x143, 0xC, 0xF, false));
    return __builtin_amdgcn_readlane(x, 63);
}

// a stem (i,j) as a branch of a multiloop.  Inside a multiloop both neighbours exist; cells on the sequence's border are filled
// too (nothing reads them) and must not read outside the sequence
__device__ __forceinline__ int mfe_stem_ml(const SmallT *T, const uint8_t *S, int L, int i, int j)
{
    return e_stem(T, pair_type(S[i], S[j]), i > 0 ? (int)S[i - 1] : -1, j < L - 1 ? (int)S[j + 1] : -1, false);
}
__device__ __forceinline__ int mfe_stem_ext(const SmallT *T, const uint8_t *S, int L, int i, int j)
{
    return e_stem(T, pair_type(S[i], S[j]), i > 0 ? (int)S[i - 1] : -1, j < L - 1 ? (int)S[j + 1] : -1, true);
}
// constraint policies.  ok(i,j): the pair may close (that it is canonical and spans a hairpin is the caller's test); up(k): k may
// stay unpaired; free(a,b): every position of a..b may (the empty range is free); u(k), U(a,b): what k, what a..b add when
// unpaired; stack(i,j,p,q): what the stack of (i,j) on (p,q) = (i+1,j-1) adds.  `on`: false for the policy that compiles away.
struct MfeConNone {
    static constexpr bool on = false;
    __device__ __forceinline__ bool ok(int, int) const { return true; }
    __device__ __forceinline__ bool up(int) const { return true; }
    __device__ __forceinline__ bool free(int, int) const { return true; }
    __device__ __forceinline__ int u(int) const { return 0; }
    __device__ __forceinline__ int U(int, int) const { return 0; }
    __device__ __forceinline__ int stack(int, int, int, int) const { return 0; }
};
// over a sequence's pack (mfe_con_pack_ints(L) ints, LDS or device memory): code[L] (the partner of a bracket, else MFE_CON_*),
// must[L + 1] (must[k]: positions before k that have to pair), usum[L + 1] (the sum of u before k), b[L]
struct MfeConPack {
    static constexpr bool on = true;
    const int *code, *must, *usum, *b;
    __device__ __forceinline__ MfeConPack(const int *pack, int L) : code(pack), must(pack + L), usum(pack + 2 * L + 1), b(pack + 3 * L + 2) {}
    __device__ __forceinline__ bool ok(int i, int j) const
    {
        const int ci = code[i], cj = code[j];
        return (ci == MFE_CON_ANY || ci == MFE_CON_PAIRED || ci == MFE_CON_DOWN || ci == j) && (cj == MFE_CON_ANY || cj == MFE_CON_PAIRED || cj == MFE_CON_UP || cj == i);
    }
    __device__ __forceinline__ bool up(int k) const { return must[k + 1] == must[k]; }
    __device__ __forceinline__ bool free(int a, int b_) const { return must[b_ + 1] == must[a]; }
    __device__ __forceinline__ int u(int k) const { return usum[k + 1] - usum[k]; }
    __device__ __forceinline__ int U(int a, int b_) const { return usum[b_ + 1] - usum[a]; }
    __device__ __forceinline__ int stack(int i, int j, int p, int q) const { return b[i] + b[j] + b[p] + b[q]; }
};

// cut policies.  x(i,j): the cell spans the nick (i < c <= j); bond(k): the backbone between k - 1 and k exists; branch(i,j): the
// stem (i,j) may be a branch of a multiloop (both bonds next to it exist); close(i,j): (i,j) may close one (both bonds inside it
// exist).  `on`: false for the policy that compiles away: every guard that names a cut stands under `if constexpr (Cut::on)` or
// folds to a constant.
struct MfeCutNone {
    static constexpr bool on = false;
    __device__ __forceinline__ bool x(int, int) const { return false; }
    __device__ __forceinline__ bool bond(int) const { return true; }
    __device__ __forceinline__ bool branch(int, int) const { return true; }
    __device__ __forceinline__ bool close(int, int) const { return true; }
};
// a dimer A B with B's first base at c (0 < c < L).  G: L + 1 ints, the exterior energies of the two strand ends: G[i] of
// i..c-1 for i < c (FA), G[j + 1] of c..j for j >= c (FB), G[c] = 0 serving both.  dinit: duplex_init, added to the exterior
// stem that spans the nick.  A neighbour across a strand end does not exist.
struct MfeCut {
    static constexpr bool on = true;
    int c, dinit;
    const int *G;
    __device__ __forceinline__ bool x(int i, int j) const { return i < c && c <= j; }
    __device__ __forceinline__ bool bond(int k) const { return k != c; }
    __device__ __forceinline__ bool branch(int i, int j) const { return i != c && j + 1 != c; }
    __device__ __forceinline__ bool close(int i, int j) const { return i + 1 != c && j != c; }
    __device__ __forceinline__ int stem_ext(const SmallT *T, const uint8_t *S, int L, int i, int j) const
    {
        return e_stem(T, pair_type(S[i], S[j]), i > 0 && i != c ? (int)S[i - 1] : -1, j < L - 1 && j + 1 != c ? (int)S[j + 1] : -1, true) + (x(i, j) ? dinit : 0);
    }
    // the loop that holds the nick, closed by the cross pair (i,j) of type t: an exterior loop read from inside
    __device__ __forceinline__ int nick(const SmallT *T, const uint8_t *S, int i, int j, int t) const
    {
        return e_stem(T, rtype(t), j != c ? (int)S[j - 1] : -1, i + 1 != c ? (int)S[i + 1] : -1, true) + G[i + 1] + G[j];
    }
};

// the soft part of the loop between (i,j) and (p,q): its unpaired positions, and the stack term when there are none
template <class Con>
__device__ __forceinline__ int mfe_interior_soft(const Con &cn, int i, int j, int p, int q)
{
    return cn.U(i + 1, p - 1) + cn.U(q + 1, j - 1) + (p == i + 1 && q == j - 1 ? cn.stack(i, j, p, q) : 0);
}
// interior-loop candidate x of the pair (i,j) of type t: its energy with C[p][q], MFE_INF when there is no such loop.  A lane
// whose candidate the constraints remove returns MFE_INF like any other that has none: it stays in the minimum and the ballots
template <class Tab, class Con, class Cut>
__device__ __forceinline__ int mfe_interior(const Tab &tb, const Con &cn, const Cut &ct, const SmallT *T, const BigT *B, const uint8_t *S, int i, int j, int t, int x, int &p, int &q)
{
    const int n12 = mfe_il.v[x], n1 = n12 >> 8, n2 = n12 & 255;
    p = i + 1 + n1; q = j - 1 - n2;
    if constexpr (Cut::on) {                // inside a cross pair only a cross pair leaves a real loop, and it may be as short as two positions
        if (ct.x(i, j) ? !ct.x(p, q) : q - p < 4) return MFE_INF;
    } else if (q - p < 4) return MFE_INF;
    const int t2 = pair_type(S[p], S[q]);
    if (!t2) return MFE_INF;
    const int cc = tb.c(p, q);
    if (cc >= MFE_INFH) return MFE_INF;
    if (!cn.free(i + 1, p - 1) || !cn.free(q + 1, j - 1)) return MFE_INF;
    int g = 0;
    return e_intloop(T, B, n1, n2, t, rtype(t2), S[i + 1], S[j - 1], S[p - 1], S[q + 1], g) + cc + mfe_interior_soft(cn, i, j, p, q);
}
// what closing a multiloop with (i,j) of type t adds to its inside M[i+1][k-1] + M1[k][j-1]
__device__ __forceinline__ int mfe_ml_close(const SmallT *T, const uint8_t *S, int i, int j, int t)
{
    return T->ml_closing + e_stem(T, rtype(t), S[j - 1], S[i + 1], false);
}

// one wavefront fills cell (i,j) of the three tables; every cell of a smaller j - i is there (under a cut: and G, for a cross
// cell).  A cross stem takes as little as two positions, so under a cut the split ranges cover the whole cell: the cells that
// hold no structure hold MFE_INF
template <class Tab, class Con, class Cut>
__device__ inline void mfe_cell(const Tab &tb, const Con &cn, const Cut &ct, const SmallT *T, const BigT *B, const uint8_t *S, int L, int i, int j, int lane)
{
    const int d = j - i;
    int c = MFE_INF, m1 = MFE_INF, m = MFE_INF;
    const bool cross = ct.x(i, j);
    if (d >= 4 || cross) {
        const int t = pair_type(S[i], S[j]);
        if (t && cn.ok(i, j)) {
            int best = MFE_INF;
            if (lane == 0 && !cross && cn.free(i + 1, j - 1)) best = e_hairpin(T, B, d - 1, t, S, i, j) + cn.U(i + 1, j - 1);
            if constexpr (Cut::on)
                if (lane == 0 && cross) best = ct.nick(T, S, i, j, t);
            for (int x = lane; x < MFE_NIL; x += 64) {
                int p, q;
                best = min(best, mfe_interior(tb, cn, ct, T, B, S, i, j, t, x, p, q));
            }
            int ml = MFE_INF;                       // a stem takes five positions: k - 1 >= i + 5, k <= j - 5
            for (int k = i + (Cut::on ? 2 : 6) + lane; k <= j - (Cut::on ? 1 : 5); k += 64) {
                const int a = tb.m(i + 1, k - 1), b = tb.m1(k, j - 1);
                if (a < MFE_INFH && b < MFE_INFH && ct.bond(k)) ml = min(ml, a + b);
            }
            if (ml < MFE_INFH && ct.close(i, j)) best = min(best, ml + mfe_ml_close(T, S, i, j, t));
            c = mfe_wave_min(best);
            if (c < MFE_INFH && ct.branch(i, j)) m1 = c + mfe_stem_ml(T, S, L, i, j);
        }
        const int mlb = T->ml_base;
        const int prev = tb.m1(i, j - 1);
        if (prev < MFE_INFH && cn.up(j) && ct.bond(j)) m1 = min(m1, prev + mlb + cn.u(j));
        m = m1;
        const int nx = tb.m(i + 1, j);
        if (nx < MFE_INFH && cn.up(i) && ct.bond(i + 1)) m = min(m, nx + mlb + cn.u(i));
        int sp = MFE_INF;
        for (int k = i + (Cut::on ? 1 : 5) + lane; k <= j - (Cut::on ? 0 : 4); k += 64) {
            const int a = tb.m(i, k - 1), b = tb.m1(k, j);
            if (a < MFE_INFH && b < MFE_INFH && ct.bond(k)) sp = min(sp, a + b);
        }
        m = min(m, mfe_wave_min(sp));
    }
    if (lane == 0) { tb.c(i, j) = c; tb.m1(i, j) = m1; tb.m(i, j) = m; }
}

// What the exterior loop and the traceback need to know of a layout besides its table view: how a stack word packs (i, j, table),
// where the exterior stems that end at j begin (i ascending from there), and the exterior candidate C[i][j] + stem (MFE_INF: none).
enum { MFE_K_C = 0, MFE_K_M = 1, MFE_K_M1 = 2, MFE_K_FA = 3, MFE_K_FB = 4 };     // FA (i, c-1), FB (c, j): the strand ends of a dimer
struct MfeWalkFull {
    __device__ __forceinline__ uint32_t pack(int i, int j, int kind) const { return (uint32_t)i | (uint32_t)j << 12 | (uint32_t)kind << 24; }
    __device__ __forceinline__ void unpack(uint32_t w, int &i, int &j, int &kind) const { i = (int)(w & 4095u); j = (int)((w >> 12) & 4095u); kind = (int)(w >> 24); }
    __device__ __forceinline__ int lo(int) const { return 0; }
    template <class Tab>
    __device__ __forceinline__ int ext(const Tab &tb, const SmallT *T, const uint8_t *S, int L, int i, int j) const
    {
        const int c = tb.c(i, j);
        return c < MFE_INFH ? c + mfe_stem_ext(T, S, L, i, j) : MFE_INF;
    }
};
// the same for a dimer: the exterior stems know the strand ends, and the one that spans the nick carries duplex_init
struct MfeWalkCut : MfeWalkFull {
    MfeCut ct;
    __device__ __forceinline__ MfeWalkCut(const MfeCut &ct_) : ct(ct_) {}
    template <class Tab>
    __device__ __forceinline__ int ext(const Tab &tb, const SmallT *T, const uint8_t *S, int L, int i, int j) const
    {
        const int c = tb.c(i, j);
        return c < MFE_INFH ? c + ct.stem_ext(T, S, L, i, j) : MFE_INF;
    }
};

// One wavefront: the exterior loop.  F: L + 1 ints of LDS, F[j + 1] = exterior energy of 0..j (under constraints MFE_INF where
// 0..j has no structure)
template <class Tab, class Walk, class Con, class Cut>
__device__ inline void mfe_exterior(const Tab &tb, const Walk &wk, const Con &cn, const Cut &, const SmallT *T, const uint8_t *S, int L, int *F, int lane)
{
    if (lane == 0) F[0] = 0;
    wave_sync();
    for (int j = 0; j < L; j++) {
        int best = MFE_INF;
        for (int i = wk.lo(j) + lane; i <= j - (Cut::on ? 1 : 4); i += 64) {
            const int e = wk.ext(tb, T, S, L, i, j);
            if (e < MFE_INFH && (!Con::on || F[i] < MFE_INFH)) best = min(best, F[i] + e);
        }
        best = mfe_wave_min(best);
        const int prev = F[j];
        if (lane == 0) F[j + 1] = !Con::on ? min(prev, best) : prev < MFE_INFH && cn.up(j) ? min(prev + cn.u(j), best) : best;
        wave_sync();
    }
}

// One wavefront: the traceback from the F of mfe_exterior, with an explicit stack of (i, j, table) words; F holds the pair table
// once the exterior loop is traced.  `stack`: `cap` words only lane 0 touches.
// rec = (dcal, pairs, 1 when no candidate reproduced a cell - an internal error, the soft part of dcal for the row: 0 without
// constraints).  Under constraints a sequence without a structure gets a row of dots and rec = (MFE_INF, 0, 0, 0).
// Under a cut the stack also holds the strand ends FA (i, c-1) and FB (c, j) the loop with the nick pushes, traced from ct.G -
// FA: i unpaired, then the stems (i,j), j ascending; FB as F - and rec.w counts the pairs that span the nick.
template <class Tab, class Walk, class Con, class Cut>
__device__ inline void mfe_traceback(const Tab &tb, const Walk &wk, const Con &cn, const Cut &ct, const SmallT *T, const BigT *B, const uint8_t *S, int L, int *F, uint32_t *stack,
                                     int cap, char *db, int4 *rec, int lane)
{
    const int mfe = F[L];
    if (Con::on && mfe >= MFE_INFH) {
        for (int x = lane; x < L; x += 64) db[x] = '.';
        if (lane == 0) { db[L] = 0; *rec = make_int4(MFE_INF, 0, 0, 0); }
        return;
    }
    int sp = 0, npairs = 0, bad = 0, soft = 0, ninter = 0;
    constexpr int MIN_D = Cut::on ? 1 : 4;              // the shortest exterior stem
    auto push = [&](int i, int j, int kind) {
        if (sp >= cap) { bad = 1; return; }
        if (lane == 0) stack[sp] = wk.pack(i, j, kind);
        sp++;
    };
    int rest = L - 1;                                   // the 3' end of what the exterior loop has not traced yet
    for (int j = rest; j >= MIN_D && !bad; rest = j) {
        const int v = F[j + 1];
        if (!Con::on ? v == F[j] : F[j] < MFE_INFH && cn.up(j) && v == F[j] + cn.u(j)) { soft += cn.u(j); j--; continue; }
        int found = -1;
        for (int i0 = wk.lo(j); i0 <= j - MIN_D && found < 0; i0 += 64) {
            const int i = i0 + lane;
            bool hit = false;
            if (i <= j - MIN_D) {
                const int e = wk.ext(tb, T, S, L, i, j);
                hit = e < MFE_INFH && (!Con::on || F[i] < MFE_INFH) && F[i] + e == v;
            }
            const unsigned long long bal = __ballot(hit);
            if (bal) found = i0 + __ffsll((long long)bal) - 1;
        }
        if (found < 0) { bad = 1; break; }
        push(found, j, MFE_K_C);
        j = found - 1;
    }
    if (Con::on && rest >= 0) soft += cn.U(0, rest);    // what is left of the 5' end holds no pair
    wave_sync();
    int *pt = F;
    for (int x = lane; x < L; x += 64) pt[x] = -1;
    wave_sync();
    const int mlb = T->ml_base;
    while (sp > 0 && !bad) {
        sp--;
        uint32_t w = 0;
        if (lane == 0) w = stack[sp];
        w = (uint32_t)__shfl((int)w, 0, 64);
        int i, j, kind;
        wk.unpack(w, i, j, kind);
        if constexpr (Cut::on) {
            if (kind == MFE_K_FA || kind == MFE_K_FB) {
                const int *G = ct.G;
                while (i <= j && !bad) {
                    const bool fa = kind == MFE_K_FA;
                    const int v = fa ? G[i] : G[j + 1];
                    if (v == (fa ? G[i + 1] : G[j])) { if (fa) i++; else j--; continue; }
                    int found = -1;             // the other end of the stem at i (FA) or at j (FB), ascending
                    for (int y0 = i + (fa ? 4 : 0); y0 <= j - (fa ? 0 : 4) && found < 0; y0 += 64) {
                        const int y = y0 + lane;
                        bool hit = false;
                        if (y <= j - (fa ? 0 : 4)) {
                            const int e = fa ? wk.ext(tb, T, S, L, i, y) : wk.ext(tb, T, S, L, y, j);
                            hit = e < MFE_INFH && e + (fa ? G[y + 1] : G[y]) == v;
                        }
                        const unsigned long long bal = __ballot(hit);
                        if (bal) found = y0 + __ffsll((long long)bal) - 1;
                    }
                    if (found < 0) { bad = 1; break; }
                    if (fa) { push(i, found, MFE_K_C); i = found + 1; }
                    else { push(found, j, MFE_K_C); j = found - 1; }
                }
                continue;
            }
        }
        if (kind == MFE_K_M) {
            for (;;) {
                const int v = tb.m(i, j);
                if (tb.m1(i, j) == v) { kind = MFE_K_M1; break; }
                if (j > i) {
                    const int nx = tb.m(i + 1, j);
                    if (nx < MFE_INFH && cn.up(i) && ct.bond(i + 1) && nx + mlb + cn.u(i) == v) { soft += cn.u(i); i++; continue; }
                }
                int found = -1;
                for (int k0 = i + (Cut::on ? 1 : 5); k0 <= j - (Cut::on ? 0 : 4) && found < 0; k0 += 64) {
                    const int k = k0 + lane;
                    bool hit = false;
                    if (k <= j - (Cut::on ? 0 : 4)) {
                        const int a = tb.m(i, k - 1), b = tb.m1(k, j);
                        hit = a < MFE_INFH && b < MFE_INFH && ct.bond(k) && a + b == v;
                    }
                    const unsigned long long bal = __ballot(hit);
                    if (bal) found = k0 + __ffsll((long long)bal) - 1;
                }
                if (found < 0) { bad = 1; break; }
                push(i, found - 1, MFE_K_M);
                i = found; kind = MFE_K_M1;
                break;
            }
        }
        if (!bad && kind == MFE_K_M1) {
            for (;;) {
                const int v = tb.m1(i, j), c = tb.c(i, j);
                if (c < MFE_INFH && ct.branch(i, j) && c + mfe_stem_ml(T, S, L, i, j) == v) { kind = MFE_K_C; break; }
                if (j > i) {
                    const int prev = tb.m1(i, j - 1);
                    if (prev < MFE_INFH && cn.up(j) && ct.bond(j) && prev + mlb + cn.u(j) == v) { soft += cn.u(j); j--; continue; }
                }
                bad = 1;
                break;
            }
        }
        if (bad || kind != MFE_K_C) continue;
        if (lane == 0) { pt[i] = j; pt[j] = i; }
        npairs++;
        const int v = tb.c(i, j), t = pair_type(S[i], S[j]);
        if (!t || v >= MFE_INFH) { bad = 1; continue; }
        const bool cross = ct.x(i, j);
        if constexpr (Cut::on) {
            ninter += cross;
            if (cross && ct.nick(T, S, i, j, t) == v) {
                if (i + 1 < ct.c) push(i + 1, ct.c - 1, MFE_K_FA);
                if (j > ct.c) push(ct.c, j - 1, MFE_K_FB);
                continue;
            }
        }
        if (!cross && cn.free(i + 1, j - 1) && e_hairpin(T, B, j - i - 1, t, S, i, j) + cn.U(i + 1, j - 1) == v) { soft += cn.U(i + 1, j - 1); continue; }
        int found = -1;
        for (int x0 = 0; x0 < MFE_NIL && found < 0; x0 += 64) {
            const int x = x0 + lane;
            int p, q;
            const bool hit = x < MFE_NIL && mfe_interior(tb, cn, ct, T, B, S, i, j, t, x, p, q) == v;
            const unsigned long long bal = __ballot(hit);
            if (bal) found = x0 + __ffsll((long long)bal) - 1;
        }
        if (found >= 0) {
            const int n12 = mfe_il.v[found], p = i + 1 + (n12 >> 8), q = j - 1 - (n12 & 255);
            soft += mfe_interior_soft(cn, i, j, p, q);
            push(p, q, MFE_K_C);
            continue;
        }
        const int close = mfe_ml_close(T, S, i, j, t);
        for (int k0 = i + (Cut::on ? 2 : 6); k0 <= j - (Cut::on ? 1 : 5) && found < 0 && ct.close(i, j); k0 += 64) {
            const int k = k0 + lane;
            bool hit = false;
            if (k <= j - (Cut::on ? 1 : 5)) {
                const int a = tb.m(i + 1, k - 1), b = tb.m1(k, j - 1);
                hit = a < MFE_INFH && b < MFE_INFH && ct.bond(k) && a + b + close == v;
            }
            const unsigned long long bal = __ballot(hit);
            if (bal) found = k0 + __ffsll((long long)bal) - 1;
        }
        if (found < 0) { bad = 1; continue; }
        push(i + 1, found - 1, MFE_K_M);
        push(found, j - 1, MFE_K_M1);
    }
    wave_sync();
    for (int x = lane; x < L; x += 64) { const int y = pt[x]; db[x] = y < 0 ? '.' : y > x ? '(' : ')'; }
    if (lane == 0) { db[L] = 0; *rec = make_int4(mfe, npairs, bad, Cut::on ? ninter : soft); }
}

// LDS class: a workgroup folds sequence s, its tables, F and bases (already there, a barrier behind them) in LDS
template <class Con>
__device__ __forceinline__ void mfe_lds_fold(const MfeTabLds &tb, const Con &cn, const EnergyTables *ET, const MfeSeq &q, int *F, const uint8_t *S, uint32_t *stacks,
                                             char *db, int4 *rec)
{
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SmallT *T = &ET->s;
    const BigT *B = &ET->b;
    for (int d = 0; d < L; d++) {
        for (int i = wave; i + d < L; i += MFE_LDS_NT / 64) mfe_cell(tb, cn, MfeCutNone(), T, B, S, L, i, i + d, lane);
        __syncthreads();
    }
    if (wave == 0) {
        mfe_exterior(tb, MfeWalkFull(), cn, MfeCutNone(), T, S, L, F, lane);
        mfe_traceback(tb, MfeWalkFull(), cn, MfeCutNone(), T, B, S, L, F, stacks + q.stack_off, L + 8, db + q.db_off, rec, lane);
    }
}
// workgroup b folds sequence order[b]
__global__ __launch_bounds__(MFE_LDS_NT) void mfe_lds_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes,
                                                            uint32_t *stacks, char *db, int4 *rec)
{
    extern __shared__ __align__(16) int mfe_lds[];
    const int s = order[blockIdx.x];
    const MfeSeq q = seqs[s];
    const int L = q.L, N = L * (L + 1) / 2, tid = threadIdx.x;
    const MfeTabLds tb{mfe_lds, mfe_lds + N, mfe_lds + 2 * N, L};
    int *F = mfe_lds + 3 * N;
    uint8_t *S = (uint8_t *)(F + L + 1);
    for (int x = tid; x < L; x += MFE_LDS_NT) S[x] = codes[q.code_off + x];
    __syncthreads();
    mfe_lds_fold(tb, MfeConNone(), ET, q, F, S, stacks, db, rec + s);
}
// the same under constraints: con_off[s] is where the sequence's pack lies in `packs` (MFE_CON_NONE: it has none and is folded
// as mfe_lds_kernel folds it); the pack goes to LDS behind the bases (mfe_con_lds_bytes)
__global__ __launch_bounds__(MFE_LDS_NT) void mfe_con_lds_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes,
                                                                const unsigned long long *con_off, const int *packs, uint32_t *stacks, char *db, int4 *rec)
{
    extern __shared__ __align__(16) int mfe_lds[];
    const int s = order[blockIdx.x];
    const MfeSeq q = seqs[s];
    const unsigned long long co = con_off[s];
    const int L = q.L, N = L * (L + 1) / 2, tid = threadIdx.x;
    const MfeTabLds tb{mfe_lds, mfe_lds + N, mfe_lds + 2 * N, L};
    int *F = mfe_lds + 3 * N;
    uint8_t *S = (uint8_t *)(F + L + 1);
    int *pack = mfe_lds + mfe_lds_bytes(L) / 4;
    for (int x = tid; x < L; x += MFE_LDS_NT) S[x] = codes[q.code_off + x];
    if (co != MFE_CON_NONE)
        for (int x = tid; x < mfe_con_pack_ints(L); x += MFE_LDS_NT) pack[x] = packs[co + x];
    __syncthreads();
    if (co != MFE_CON_NONE) mfe_lds_fold(tb, MfeConPack(pack, L), ET, q, F, S, stacks, db, rec + s);
    else mfe_lds_fold(tb, MfeConNone(), ET, q, F, S, stacks, db, rec + s);
}

// HBM class: anti-diagonal d of a sequence, four cells per workgroup and round
template <class Con>
__device__ __forceinline__ void mfe_diag_fill(const Con &cn, const EnergyTables *ET, const MfeSeq &q, const uint8_t *codes, int *tabs, int d)
{
    const int L = q.L, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int *t0 = tabs + q.tab_off;
    const size_t LL = (size_t)L * L;
    const MfeTabHbm tb{t0, t0 + LL, t0 + 2 * LL, L};
    const uint8_t *S = codes + q.code_off;
    for (int i = blockIdx.x * (MFE_HBM_NT / 64) + wave; i + d < L; i += gridDim.x * (MFE_HBM_NT / 64)) mfe_cell(tb, cn, MfeCutNone(), &ET->s, &ET->b, S, L, i, i + d, lane);
}
// of the sequences order[0 .. gridDim.y)
__global__ __launch_bounds__(MFE_HBM_NT) void mfe_diag_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes, int *tabs, int d)
{
    const MfeSeq q = seqs[order[blockIdx.y]];
    if (d >= q.L) return;
    mfe_diag_fill(MfeConNone(), ET, q, codes, tabs, d);
}
// the same under constraints, the packs read where they lie in device memory
__global__ __launch_bounds__(MFE_HBM_NT) void mfe_con_diag_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes,
                                                                 const unsigned long long *con_off, const int *packs, int *tabs, int d)
{
    const int s = order[blockIdx.y];
    const MfeSeq q = seqs[s];
    if (d >= q.L) return;
    const unsigned long long co = con_off[s];
    if (co != MFE_CON_NONE) mfe_diag_fill(MfeConPack(packs + co, q.L), ET, q, codes, tabs, d);
    else mfe_diag_fill(MfeConNone(), ET, q, codes, tabs, d);
}

// the exterior loop and the traceback of a sequence of the HBM class, one wavefront; F: L + 1 ints of LDS
template <class Con>
__device__ __forceinline__ void mfe_hbm_trace(const Con &cn, const EnergyTables *ET, const MfeSeq &q, const uint8_t *codes, int *tabs, int *F, uint32_t *stacks,
                                              char *db, int4 *rec)
{
    const int L = q.L;
    int *t0 = tabs + q.tab_off;
    const size_t LL = (size_t)L * L;
    const MfeTabHbm tb{t0, t0 + LL, t0 + 2 * LL, L};
    mfe_exterior(tb, MfeWalkFull(), cn, MfeCutNone(), &ET->s, codes + q.code_off, L, F, (int)threadIdx.x);
    mfe_traceback(tb, MfeWalkFull(), cn, MfeCutNone(), &ET->s, &ET->b, codes + q.code_off, L, F, stacks + q.stack_off, L + 8, db + q.db_off, rec, (int)threadIdx.x);
}
__global__ __launch_bounds__(64) void mfe_traceback_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes, int *tabs,
                                                          uint32_t *stacks, char *db, int4 *rec)
{
    __shared__ int F[RAFFT_MFE_MAX_LEN + 1];
    const int s = order[blockIdx.x];
    const MfeSeq q = seqs[s];
    mfe_hbm_trace(MfeConNone(), ET, q, codes, tabs, F, stacks, db, rec + s);
}
__global__ __launch_bounds__(64) void mfe_con_traceback_kernel(const EnergyTables *ET, const MfeSeq *seqs, const int *order, const uint8_t *codes,
                                                              const unsigned long long *con_off, const int *packs, int *tabs, uint32_t *stacks, char *db, int4 *rec)
{
    __shared__ int F[RAFFT_MFE_MAX_LEN + 1];
    const int s = order[blockIdx.x];
    const MfeSeq q = seqs[s];
    const unsigned long long co = con_off[s];
    if (co != MFE_CON_NONE) mfe_hbm_trace(MfeConPack(packs + co, q.L), ET, q, codes, tabs, F, stacks, db, rec + s);
    else mfe_hbm_trace(MfeConNone(), ET, q, codes, tabs, F, stacks, db, rec + s);
}
