// rafft_materialize.hip - materialize_kernel / materialize_team_kernel and dedupe_kernel: the child regions of the new beam
// members, created once (gfx950).  Included by rafft_kernels.hip.
#pragma once

// ------------------------------------------------------- materialize kernel

// One team of lanes per new beam member.  Child regions are spliced from the parent's
// regions: inner = positions/branches strictly inside the innermost stem pair, outer =
// the rest of the parent's loop with the whole stem as one new branch.
//
// One lane describes one productive region of the parent (chosen stem, the branch indices it cuts the
// loop at, sizes of the two child regions); the copies then run FLAT over all output elements of the
// tile (binary search element -> child region), so every load of the team is independent and in
// flight at once instead of one dependent round trip per region.
struct MatDesc {
    unsigned long long srcpos, srcbr, cidx;      // cidx: the candidate (its two child slots are cslot[2 cidx], cslot[2 cidx + 1])
    int pn, mi, mj, nb, n, nbr, ci, cj, lo0, hi0, loo, hio, a0, b0, ao, bo, flags, win;   // flags: which children exist (1 inner, 2 outer); win: which of them THIS structure creates
    uint32_t newbr;        // the stem as a branch of the outer child: outermost pair, in the arena's (packed) form
    int nnod, npos_in, npos_out, nbr_in, nbr_out;
};
// (`cidx` comes from the parent's productive-region list: the candidate record and the region header are independent loads)
__device__ inline MatDesc mat_describe(const Dev &d, int pn, unsigned long long cidx)
{
    MatDesc m;
    m.pn = pn;
    const Cand cd = d.cand[cidx];
    // (the header as three 16-byte loads issued together: as single fields the compiler loaded `nbr` where it is first used - after the
    //  loads of the four stem positions below, whose round trip it then waited for before the arena allocations could be issued)
    const uint4 *hp = (const uint4 *)&d.nd[pn];
    const uint4 hq0 = hp[0], hq1 = hp[1], hq2 = hp[2];      // seq pdcal n ci | cj nbr ncand L | pos br
    m.n = (int)hq0.z; m.ci = (int)hq0.w; m.cj = (int)hq1.x; m.nbr = (int)hq1.y;
    m.srcpos = (unsigned long long)hq2.x | ((unsigned long long)hq2.y << 32); m.srcbr = (unsigned long long)hq2.z | ((unsigned long long)hq2.w << 32);
    m.cidx = cidx;
    m.mi = cd.mi; m.mj = cd.mj; m.nb = cd.nb;
    const uint16_t *pp = d.pos + m.srcpos;
    const int pm = d.pos_packed ? 0x0FFF : 0xFFFF;
    const uint32_t rao = pp[m.mi - m.nb + 1], rbo = pp[m.mj + m.nb - 1];
    m.a0 = pp[m.mi] & pm; m.b0 = pp[m.mj] & pm; m.ao = (int)rao & pm; m.bo = (int)rbo & pm;
    m.newbr = rao | (rbo << 16);          // (with Dev::pos_packed the base codes ride in bits 12-15 and 28-31)
    cd.get_cuts(m.lo0, m.hi0, m.loo, m.hio);      // where the stem cuts the branch list (found by expand_kernel)
    // (no branches: every header field is used right here, so all of them are loaded together - see above)
    const bool has_in = m.mj - m.mi > 1, has_out = m.mi - (m.nb - 1) > 0 || m.mj + m.nb < m.n;
    m.win = 0;
    m.flags = (has_in ? 1 : 0) | (has_out ? 2 : 0); m.nnod = (has_in ? 1 : 0) + (has_out ? 1 : 0);
    m.npos_in = has_in ? m.mj - m.mi - 1 : 0; m.nbr_in = has_in ? m.hi0 - m.lo0 : 0;
    m.npos_out = has_out ? (m.mi - m.nb + 1) + (m.n - (m.mj + m.nb)) : 0; m.nbr_out = has_out ? m.loo + 1 + (m.nbr - m.hio) : 0;
    return m;
}

// The flat copies of one tile of the materialize kernels: unpaired positions and branch helices of the regions created, pairs of
// the stems.  (Round 5: U elements per lane are located and LOADED before the first of them is stored - with one element per
// iteration every load was waited for before its store and the next load issued after it: a dependent HBM round trip per 16 (64)
// elements, five or six per structure on the benchmark set, a dozen and more on long sequences.)
// `l`: my lane in the team, STR lanes; descriptor kk of the tile sits at index kb + kk of the k_* arrays.
template <int STR, int U>
__device__ __forceinline__ void mat_copy_tile(const Dev &d, int l, int kb, int kt, const int *ps, const int *bs, const int *ns,
                                              const unsigned long long *k_srcpos, const unsigned long long *k_srcbr, const int *k_mi, const int *k_mj,
                                              const int *k_nb, const int *k_lo0, const int *k_loo, const int *k_hio, const int *k_newbr,
                                              int tp, int tbr, int ts, unsigned long long pdst, unsigned long long bdst, unsigned long long sdst, int pmask)
{
    for (int f0 = l; f0 < tp; f0 += STR * U) {           // unpaired positions of the regions created here
        uint32_t v[U];          // (32-bit: two 16-bit values packed into one register are a wait after every load)
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int f = f0 + u * STR;
            v[u] = 0;
            if (f < tp) {
                int lo = 0, hi = 2 * kt - 1;             // last slot starting at or before f (empty slots share starts)
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ps[mid] <= f) lo = mid; else hi = mid - 1; }
                const int kk = kb + (lo >> 1), off = f - ps[lo];
                const uint16_t *pp = d.pos + k_srcpos[kk];
                int src;
                if (!(lo & 1)) src = k_mi[kk] + 1 + off;
                else { const int left = k_mi[kk] - k_nb[kk] + 1; src = off < left ? off : k_mj[kk] + k_nb[kk] + (off - left); }
                v[u] = pp[src];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { const int f = f0 + u * STR; if (f < tp) d.pos[pdst + f] = (uint16_t)v[u]; }
    }
    for (int f0 = l; f0 < tbr; f0 += STR * U) {          // their branch helices
        uint32_t v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int f = f0 + u * STR;
            v[u] = 0;
            if (f < tbr) {
                int lo = 0, hi = 2 * kt - 1;
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (bs[mid] <= f) lo = mid; else hi = mid - 1; }
                const int kk = kb + (lo >> 1), off = f - bs[lo];
                const uint32_t *bb = d.br + k_srcbr[kk];
                if (!(lo & 1)) v[u] = bb[k_lo0[kk] + off];
                else {
                    const int loo = k_loo[kk];
                    v[u] = off < loo ? bb[off] : off == loo ? (uint32_t)k_newbr[kk] : bb[k_hio[kk] + (off - loo - 1)];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { const int f = f0 + u * STR; if (f < tbr) d.br[bdst + f] = v[u]; }
    }
    // the pairs of the stems (rafft/rafft.py:97,127-128 marks them in the parent's dot-bracket row; here the row is implicit)
    for (int f0 = l; f0 < ts; f0 += STR * U) {
        uint32_t va[U], vb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int f = f0 + u * STR;
            va[u] = 0; vb[u] = 0;
            if (f < ts) {
                int lo = 0, hi = kt - 1;
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ns[mid] <= f) lo = mid; else hi = mid - 1; }
                const int t = f - ns[lo];
                const uint16_t *pp = d.pos + k_srcpos[kb + lo];
                va[u] = pp[k_mi[kb + lo] - t]; vb[u] = pp[k_mj[kb + lo] + t];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { const int f = f0 + u * STR; if (f < ts) d.sp[sdst + f] = (uint32_t)(va[u] & pmask) | ((uint32_t)(vb[u] & pmask) << 16); }
    }
}

#ifndef RAFFT_MAT_WAVES
#define RAFFT_MAT_WAVES 1
#endif
constexpr int MAT_NT = 64;              // materialize_kernel: one team of 64 lanes, the wavefront
constexpr int MAT4_TL = 16;             // materialize_team_kernel: teams of 16 lanes ...
constexpr int MAT4_TEAMS = 64 / MAT4_TL;
constexpr int MAT4_PROD = 64;           // ... with productive-region lists of this many entries in static LDS

// sums and inclusive scans over a team of TL lanes: DPP row scans for a team of 16 (one row), shuffles for the whole wavefront
template <int TL>
__device__ __forceinline__ int team_incl_scan(int x, int tl)
{
    if constexpr (TL == 16) return row16_incl_scan(x);
    else {
        static_assert(TL == 64, "a team is one DPP row or the whole wavefront");
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (tl >= o) x += y; }
        return x;
    }
}
template <int TL>
__device__ __forceinline__ int team_sum(int x)
{
    if constexpr (TL == 16) return __shfl(row16_incl_scan(x), TL - 1, TL);
    else {
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        return x;
    }
}

// One new beam member per team of TL lanes, 64 / TL of them per wavefront at a time (the reference's create_childs,
// rafft/rafft.py:112-153).  The workgroup is one wavefront.  `prod_off` .. `sel`: my team's productive-region lists, `cap`
// entries each.  A structure is stored as the pairs it adds to its parent's: no dot-bracket row is staged or written here.
// (`d` by value, as the kernels get it: through a reference the compiler must assume that the stores below may alias its fields,
//  and the team kernel came out with other code and SGPR spills)
template <int TL>
__device__ __forceinline__ void materialize_body(const Dev d, int n_mat, unsigned long long *prod_off, int *prod_node, int *prod_cnt,
                                                 int *sel, int cap)
{
    constexpr int TEAMS = 64 / TL;
    const int tid = threadIdx.x, team = tid / TL, tl = tid % TL;
    // per-tile descriptors (one lane per productive region; index = lane of the wavefront) and the flat-copy prefix sums of every
    // team (two slots per region)
    __shared__ unsigned long long k_srcpos[64], k_srcbr[64];
    __shared__ int k_mi[64], k_mj[64], k_nb[64], k_lo0[64], k_loo[64], k_hio[64], k_newbr[64];
    __shared__ int ps_[TEAMS][2 * TL + 1], bs_[TEAMS][2 * TL + 1], ns_[TEAMS][TL + 1];
    __shared__ unsigned long long sh64_[TEAMS][5];
    int *ps = ps_[team], *bs = bs_[team], *ns = ns_[team];
    const int tb = team * TL;                            // first lane of my team
    const unsigned long long tmask = (~0ULL >> (64 - TL)) << tb;
    if (d.c->overflow) return;                           // (see expand_kernel)
    for (int mat_i0 = blockIdx.x * TEAMS; mat_i0 < n_mat; mat_i0 += gridDim.x * TEAMS) {
    const int mat_i = mat_i0 + team;
    const bool live = mat_i < n_mat;
    MatRec rec;
    rec.sid = 0; rec.sq = 0; rec.L = 0; rec.dcal = 0; rec.nprod = 0; rec.combo = 0; rec.prod = 0; rec.soff = 0;
    if (live) rec = d.mat[mat_i];                        // written by the beam step: no chain of look-ups to get started
    const int sid = rec.sid, sq = rec.sq, L = rec.L, my_dcal = rec.dcal;
    const uint64_t soff = rec.soff;
    const int pmask = d.pos_packed ? 0x0FFF : 0xFFFF;
    int mprod = rec.nprod;
    if (mprod > cap) mprod = cap;
    {
        const ProdEnt *pl = d.prod + rec.prod;             // the parent's productive regions (beam_step prepass)
        for (int k = tl; k < mprod; k += TL) { const ProdEnt pe = pl[k]; prod_node[k] = pe.node; prod_cnt[k] = (int)pe.cnt; prod_off[k] = pe.off; sel[k] = 0; }
    }
    wave_sync();
    if (tl == 0) {       // digits of the combo, last region fastest; high digits of a small index stay 0
        unsigned long long idx = rec.combo;
        for (int k = mprod - 1; k >= 0 && idx; k--) {
            const unsigned int c = (unsigned int)prod_cnt[k];
            if (idx < (1ULL << 24)) {
                const unsigned int v = (unsigned int)idx;
                unsigned int q = (unsigned int)((float)v * __frcp_rn((float)c));       // off by one at most
                int r = (int)(v - q * c);
                if (r < 0) { q--; r += (int)c; } else if (r >= (int)c) { q++; r -= (int)c; }
                sel[k] = r; idx = q;
            } else { const unsigned long long q = idx / c; sel[k] = (int)(idx - q * c); idx = q; }
        }
    }
    wave_sync();

    // pass 1: sizes, and who creates what.  A child region is a function of (parent region, candidate, side) alone
    // (rafft/rafft.py:127-152, rafft/utils.py:141-152): the beam member whose compare-and-swap finds the slot empty creates it, everybody
    // else - the other members of this step that picked the same stem, and every later step - only notes the slot number in its node
    // list (the next beam step reads the region id out of the slot, once this kernel and dedupe_kernel are done: nobody reads a slot's
    // value in here).  Without memoization (min_nrj != 0: a region's filter depends on its parent's energy) every member creates its own.
    // (a single tile - the usual case - keeps its descriptors in registers for pass 2; with several the claims ride in sel[])
    const int TILE = d.mat_tile < TL ? d.mat_tile : TL;       // d.mat_tile is 64; smaller only in tests (several tiles per structure)
    const bool one_tile = mprod <= TILE;
    const bool memo = d.memo != 0;
    MatDesc md;
    md.flags = 0; md.win = 0; md.nnod = 0; md.npos_in = md.npos_out = md.nbr_in = md.nbr_out = 0; md.nb = 0; md.cidx = 0;
    int tot_nodes = 0, tot_new = 0, tot_pos = 0, tot_br = 0, tot_sp = 0;
    for (int base = 0; base < mprod; base += TILE) {
        const int k = base + tl;
        int nnod = 0, nnew = 0, npos = 0, nbrr = 0, nsp = 0;
        if (k < mprod && tl < TILE) {
            // the claim of both child slots of the chosen candidate: ONE returning atomic, issued before anything else is loaded (its
            // round trip runs beside those of the region header, the candidate and the positions).  A slot word is inner | outer << 32;
            // bit 31 of a half says "claimed", and whoever finds it clear has claimed that half.  (Claiming the half of a child that
            // does not exist - an empty inside, nothing left outside - is harmless: nobody ever looks at it.)
            const unsigned long long cidx = prod_off[k] + (unsigned long long)sel[k];
            unsigned long long old = 0;
            if (memo) old = atomicOr(&d.cslot[cidx], 0x8000000080000000ULL);
            md = mat_describe(d, prod_node[k], cidx);
            int win = md.flags;
            if (memo) win &= ((old >> 31) & 1ULL ? 0 : 1) | ((old >> 63) & 1ULL ? 0 : 2);
            md.win = win;
            if (!one_tile) sel[k] |= win << 28;
            nnod = md.nnod; nnew = (win & 1) + (win >> 1); nsp = md.nb;
            npos = ((win & 1) ? md.npos_in : 0) + ((win & 2) ? md.npos_out : 0);
            nbrr = ((win & 1) ? md.nbr_in : 0) + ((win & 2) ? md.nbr_out : 0);
        }
        nnod = team_sum<TL>(nnod); nnew = team_sum<TL>(nnew); npos = team_sum<TL>(npos); nbrr = team_sum<TL>(nbrr); nsp = team_sum<TL>(nsp);
        tot_nodes += nnod; tot_new += nnew; tot_pos += npos; tot_br += nbrr; tot_sp += nsp;
    }
    bool ok = live;
    if (tl < 5 && live) {
        // bump allocation from one of NSHARD sub-arenas (spreads the same-address atomics); one lane per arena
        const int shd = mat_i & (NSHARD - 1);
        unsigned long long *ctr = tl == 0 ? &d.c->node[shd].v : tl == 1 ? &d.c->pos[shd].v : tl == 2 ? &d.c->sp[shd].v : tl == 3 ? &d.c->br[shd].v : &d.c->nlist[shd].v;
        const unsigned long long want = tl == 0 ? (unsigned long long)tot_new : tl == 1 ? (unsigned long long)tot_pos
                                      : tl == 2 ? (unsigned long long)tot_sp : tl == 3 ? (unsigned long long)tot_br : (unsigned long long)tot_nodes;
        const unsigned long long cap = tl == 0 || tl == 4 ? d.nd_shard_cap : tl == 1 ? d.pos_shard_cap : tl == 2 ? d.sp_shard_cap : d.br_shard_cap;
        const unsigned long long b0 = want ? atomicAdd(ctr, want) : 0ULL;
        const bool bad = b0 + want > cap;
        if (bad) atomicOr(&d.c->overflow, tl == 0 || tl == 4 ? OVF_NODE : tl == 1 ? OVF_POS : tl == 2 ? OVF_SP : OVF_BR);
        const unsigned long long origin = tl == 0 || tl == 4 ? d.nd_base : tl == 1 ? d.pos_base : 0ULL;
        sh64_[team][tl] = origin + (unsigned long long)shd * cap + b0;
        ok = !bad;
    }
    // (every lane of the team learns whether all five allocations fit)
    ok = ((__ballot(!ok) & tmask) == 0ULL) && live;
    wave_sync();
    if (!ok) { if (tl == 0 && live) { d.st[sid].nnodes = 0; d.st[sid].node0 = 0; d.st[sid].sp = 0; d.st[sid].nsp = 0; } }
    const unsigned long long nbase = sh64_[team][0], pbase = sh64_[team][1], sbase = sh64_[team][2], bbase = sh64_[team][3], lbase = sh64_[team][4];

    // pass 2: per tile: descriptors -> LDS, prefix sums, node-list entries, records and flat copies of the regions created here
    int run_nodes = 0, run_new = 0, run_pos = 0, run_br = 0, run_sp = 0;
    const int mp2 = ok ? mprod : 0;
    for (int base = 0; base < mp2; base += TILE) {
        const int k = base + tl;
        const int kt = mp2 - base < TILE ? mp2 - base : TILE;
        if (!one_tile) {
            md.flags = 0; md.win = 0; md.nnod = 0; md.npos_in = md.npos_out = md.nbr_in = md.nbr_out = 0; md.nb = 0;
            if (k < mp2 && tl < TILE) { md = mat_describe(d, prod_node[k], prod_off[k] + (unsigned long long)(sel[k] & 0x0FFFFFFF)); md.win = (sel[k] >> 28) & 3; }
        }
        const bool act = k < mp2 && tl < TILE;
        const int cp_in = act && (md.win & 1) ? md.npos_in : 0, cp_out = act && (md.win & 2) ? md.npos_out : 0;
        const int cb_in = act && (md.win & 1) ? md.nbr_in : 0, cb_out = act && (md.win & 2) ? md.nbr_out : 0;
        // inclusive scans over the tile: node-list entries, regions created, their pos and branch elements, stem pairs
        int xn = act ? md.nnod : 0, xw = act ? (md.win & 1) + (md.win >> 1) : 0, xp = cp_in + cp_out, xb = cb_in + cb_out, xs = act ? md.nb : 0;
        const int vn = xn, vw = xw, vp = xp, vb = xb, vs = xs;
        xn = team_incl_scan<TL>(xn, tl); xw = team_incl_scan<TL>(xw, tl); xp = team_incl_scan<TL>(xp, tl); xb = team_incl_scan<TL>(xb, tl);
        xs = team_incl_scan<TL>(xs, tl);
        const int tn = __shfl(xn, TL - 1, TL), tw = __shfl(xw, TL - 1, TL), tp = __shfl(xp, TL - 1, TL), tbr = __shfl(xb, TL - 1, TL),
                  ts = __shfl(xs, TL - 1, TL);
        const int p0 = xp - vp, b0 = xb - vb;          // exclusive
        ps[2 * tl] = p0; ps[2 * tl + 1] = p0 + cp_in;
        bs[2 * tl] = b0; bs[2 * tl + 1] = b0 + cb_in;
        ns[tl] = xs - vs;
        if (tl == 0) { ps[2 * TL] = tp; bs[2 * TL] = tbr; ns[TL] = ts; }
        if (act) {
            k_srcpos[tid] = md.srcpos; k_srcbr[tid] = md.srcbr;
            k_mi[tid] = md.mi; k_mj[tid] = md.mj; k_nb[tid] = md.nb; k_lo0[tid] = md.lo0; k_loo[tid] = md.loo; k_hio[tid] = md.hio;
            k_newbr[tid] = (int)md.newbr;
            // region records (rafft/utils.py:141-152) of the children created here, and the node list (rafft/rafft.py:187-190): inner, then outer
            int nid = (int)(nbase + run_new + (xw - vw));
            unsigned long long le = lbase + run_nodes + (xn - vn);
            const unsigned long long poff = pbase + run_pos + p0, boff = bbase + run_br + b0;
            const int slot0 = (int)(2 * md.cidx);
            if (md.flags & 1) {
                if (md.win & 1) {
                    d.nd[nid].seq = sq; d.nd[nid].pdcal = my_dcal; d.nd[nid].pos = poff; d.nd[nid].n = md.npos_in;
                    d.nd[nid].L = L; d.nd[nid].soff = soff;
                    d.nd[nid].ci = md.a0; d.nd[nid].cj = md.b0; d.nd[nid].br = boff; d.nd[nid].nbr = md.nbr_in;
                    d.nd[nid].ncand = -1; d.nd[nid].cand = 0;
                    if (memo) { d.nd_slot[nid] = (uint32_t)slot0; ((uint32_t *)d.cslot)[slot0] = (uint32_t)(nid + 1) | 0x80000000u; }
                    d.nlist[le] = memo ? -(slot0 + 1) : nid;
                    nid++;
                } else d.nlist[le] = -(slot0 + 1);
                le++;
            }
            if (md.flags & 2) {
                if (md.win & 2) {
                    d.nd[nid].seq = sq; d.nd[nid].pdcal = my_dcal; d.nd[nid].pos = poff + cp_in; d.nd[nid].n = md.npos_out;
                    d.nd[nid].L = L; d.nd[nid].soff = soff;
                    d.nd[nid].ci = md.ci; d.nd[nid].cj = md.cj; d.nd[nid].br = boff + cb_in; d.nd[nid].nbr = md.nbr_out;
                    d.nd[nid].ncand = -1; d.nd[nid].cand = 0;
                    if (memo) { d.nd_slot[nid] = (uint32_t)(slot0 + 1); ((uint32_t *)d.cslot)[slot0 + 1] = (uint32_t)(nid + 1) | 0x80000000u; }
                    d.nlist[le] = memo ? -(slot0 + 2) : nid;
                } else d.nlist[le] = -(slot0 + 2);
            }
        }
        wave_sync();
        // (descriptor kk of my team sits at lane tb + kk)
        mat_copy_tile<TL, 4>(d, tl, tb, kt, ps, bs, ns, k_srcpos, k_srcbr, k_mi, k_mj, k_nb, k_lo0, k_loo, k_hio, k_newbr, tp, tbr, ts,
                             pbase + run_pos, bbase + run_br, sbase + run_sp, pmask);
        run_nodes += tn; run_new += tw; run_pos += tp; run_br += tbr; run_sp += ts;
        wave_sync();
    }
    if (ok && tl == 0) { d.st[sid].node0 = (int)lbase; d.st[sid].nnodes = tot_nodes; d.st[sid].sp = sbase; d.st[sid].nsp = tot_sp; }
    wave_sync();
    }
}

// One new beam member per wavefront, its lists in dynamic LDS (d.max_prod entries each, up to MAX_PROD_LONG).  Host: the long
// lists - sequences longer than LDS_SEQ, or a wave folded again after a structure had more productive regions than MAX_PROD.
__global__ __launch_bounds__(MAT_NT, RAFFT_MAT_WAVES) void materialize_kernel(Dev d, int n_mat)
{
    extern __shared__ __align__(16) uint8_t mat_dyn[];
    unsigned long long *prod_off = (unsigned long long *)mat_dyn;
    int *prod_node = (int *)(prod_off + d.max_prod);
    int *prod_cnt = prod_node + d.max_prod;
    int *sel = prod_cnt + d.max_prod;
    materialize_body<MAT_NT>(d, n_mat, prod_off, prod_node, prod_cnt, sel, d.max_prod);
}

// Four new beam members per wavefront, teams of 16 lanes (round 4: a lane stands for one productive region of the parent - three to
// five of them on the benchmark set - so a wavefront per structure keeps most lanes idle through its chain of dependent round trips,
// and what a CU holds of such wavefronts bounds the structures in flight).  Host: the short lists (d.max_prod <= MAT4_PROD).
// Identical results: the arenas are bump allocated, so only the PLACES of records and lists differ from the one-structure form.
__global__ __launch_bounds__(64, RAFFT_MAT_WAVES) void materialize_team_kernel(Dev d, int n_mat)
{
    __shared__ unsigned long long prod_off_[MAT4_TEAMS][MAT4_PROD];
    __shared__ int prod_node_[MAT4_TEAMS][MAT4_PROD], prod_cnt_[MAT4_TEAMS][MAT4_PROD], sel_[MAT4_TEAMS][MAT4_PROD];
    const int team = threadIdx.x / MAT4_TL;
    materialize_body<MAT4_TL>(d, n_mat, prod_off_[team], prod_node_[team], prod_cnt_[team], sel_[team], MAT4_PROD);
}

// ------------------------------------------------------------ dedupe kernel

// a region header as four 16-byte words, loaded together: seq pdcal n ci | cj nbr ncand L | pos br | cand soff
struct NodeWords { uint4 q0, q1, q2; };
__device__ __forceinline__ NodeWords load_node_words(const Dev &d, int nid)
{
    const uint4 *hp = (const uint4 *)&d.nd[nid];
    NodeWords w;
    w.q0 = hp[0]; w.q1 = hp[1]; w.q2 = hp[2];
    pin(w.q0); pin(w.q1); pin(w.q2);
    return w;
}
// (round 5: the other region's header in one round trip and the branch lists four entries at a time - field by field, each
//  comparison behind the one before, this was seven dependent round trips)
__device__ inline bool same_loop(const Dev &d, const NodeWords &a, int b)
{
    const NodeWords o = load_node_words(d, b);
    // seq, n, ci | cj, nbr
    if (a.q0.x != o.q0.x || a.q0.z != o.q0.z || a.q0.w != o.q0.w || a.q1.x != o.q1.x || a.q1.y != o.q1.y) return false;
    const uint32_t *x = d.br + ((unsigned long long)a.q2.z | ((unsigned long long)a.q2.w << 32));
    const uint32_t *y = d.br + ((unsigned long long)o.q2.z | ((unsigned long long)o.q2.w << 32));
    const int k = (int)a.q1.y;
    for (int i = 0; i < k; i += 4) {
        unsigned int xa[4], ya[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { xa[u] = i + u < k ? x[i + u] : 0u; ya[u] = i + u < k ? y[i + u] : 0u; }
#pragma unroll
        for (int u = 0; u < 4; u++) { pin(xa[u]); pin(ya[u]); }
        if (xa[0] != ya[0] || xa[1] != ya[1] || xa[2] != ya[2] || xa[3] != ya[3]) return false;
    }
    return true;
}

// One thread per region created in this step (the new node ids are the ranges the
// materialize kernel bumped in each allocation shard since the last snapshot).  The first
// region to claim a loop key becomes canonical and goes to the expand work list; later
// identical loops alias it.  Work-list appends are aggregated per wavefront.
#ifndef DEDUPE_NT
#define DEDUPE_NT 512         // (256 / 512 / 1024 measured with eight batches in flight: 282 / 285 / 279 k sequences/s)
#endif
__global__ __launch_bounds__(DEDUPE_NT) void dedupe_kernel(Dev d)
{
    __shared__ unsigned int pre[NSHARD + 1];
    __shared__ unsigned int prev[NSHARD];
    __shared__ unsigned int wcnt[DEDUPE_NT / 64][NCLS], wbase[DEDUPE_NT / 64][NCLS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // an arena overflowed while materializing: some region records of this step were never written.
    // Nothing may be read from them; the host sees the flag at its next read-back and regrows.
    if (d.c->overflow) return;
    if (tid < NSHARD) {
        prev[tid] = (unsigned int)d.c->node_prev[tid].v;
        pre[tid + 1] = (unsigned int)(d.c->node[tid].v - d.c->node_prev[tid].v);
    }
    if (tid == 0) pre[0] = 0;
    __syncthreads();
    if (tid == 0) for (int i = 1; i <= NSHARD; i++) pre[i] += pre[i - 1];
    __syncthreads();
    const unsigned int total = pre[NSHARD];
    unsigned long long aliases = 0;
    const unsigned int stride = gridDim.x * blockDim.x;
    for (unsigned int f0 = blockIdx.x * blockDim.x; f0 < total; f0 += stride) {
        const unsigned int f = f0 + tid;
        int cls = -1, nid = 0;
        if (f < total) {
            int lo = 0, hi = NSHARD;             // shard with pre[lo] <= f < pre[lo+1]
            while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (pre[mid] <= f) lo = mid; else hi = mid; }
            nid = (int)(d.nd_base + (unsigned long long)lo * d.nd_shard_cap + prev[lo] + (f - pre[lo]));
            int canon = nid;
            // the header once, in one round trip (round 5: as single fields it was loaded in three trips here and AGAIN field by field
            // after the table look-up - the compiler cannot keep a loaded value across the compare-and-swap and the stores between)
            const NodeWords hw = load_node_words(d, nid);
            const int h_seq = (int)hw.q0.x, h_n = (int)hw.q0.z, h_ci = (int)hw.q0.w, h_cj = (int)hw.q1.x, h_nbr = (int)hw.q1.y, h_L = (int)hw.q1.w;
            if (d.memo) {
                const uint32_t *bb = d.br + ((unsigned long long)hw.q2.z | ((unsigned long long)hw.q2.w << 32));
                const int nbr = h_nbr;
                uint64_t h = mix64(((uint64_t)(uint32_t)h_seq << 32) ^ ((uint64_t)(uint32_t)(h_ci + 1) << 16) ^ (uint32_t)h_cj);
                for (int t = 0; t < nbr; t += 4) {           // (four branch helices per round trip)
                    unsigned int bv[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) bv[u] = t + u < nbr ? bb[t + u] : 0u;
#pragma unroll
                    for (int u = 0; u < 4; u++) pin(bv[u]);
#pragma unroll
                    for (int u = 0; u < 4; u++) if (t + u < nbr) h += mix64((uint64_t)bv[u] ^ 0x5bd1e9955bd1e995ULL);
                }
                const unsigned long long tag = (h >> 32) | 0x80000000ULL;
                const uint64_t mask = d.looptab_cap - 1;
                uint64_t sl = h & mask;
                for (unsigned probe = 0;; probe++) {
                    unsigned long long old = atomicCAS(&d.looptab[sl], 0ULL, (tag << 32) | (unsigned long long)(nid + 1));
                    if (old == 0) break;
                    if ((old >> 32) == tag) {
                        int other = (int)(old & 0xffffffffULL) - 1;
                        if (same_loop(d, hw, other)) { canon = other; break; }
                    }
                    sl = (sl + 1) & mask;
                    if (probe > d.looptab_cap) { atomicOr(&d.c->overflow, OVF_LOOPTAB); break; }
                }
            }
            if (canon == nid) {
                // a stem needs two unpaired positions: a lone position (bulge remnant) has no candidates
                const int n = h_n;
                if (n < 2) d.nd[nid].ncand = 0;
                else {
                    // (sequences beyond 4096 nt keep out of the one-wavefront class whatever the span: see expand_kernel's Sl)
                    const int Ls = h_L, span = (h_ci < 0 || Ls > LDS_SEQ) ? Ls : h_cj + 1 - h_ci;
                    cls = node_class(n, span, h_nbr, d.merge_cls, d.cls1_P, d.cls1_br, d.K, d.sm_n4, d.sm_n5);
                }
            }
            else { ((uint32_t *)d.cslot)[d.nd_slot[nid]] = (uint32_t)(canon + 1) | 0x80000000u; aliases++; }      // (the loop is known - reached along another path: the slot points at it)
        }
        // work-list appends, aggregated over the WORKGROUP: one atomic per class and pass (per wavefront they were
        // 4096 x 4-6 returning atomics on one cache line per pass - the kernel's whole duration)
        unsigned long long mybal = 0;
        for (int c = 0; c < NCLS; c++) {
            const unsigned long long bal = __ballot(cls == c);
            if (cls == c) mybal = bal;
            if (lane == 0) wcnt[wv][c] = (unsigned int)__popcll(bal);
        }
        __syncthreads();
        if (tid < NCLS) {
            unsigned int tot = 0;
            for (int w = 0; w < DEDUPE_NT / 64; w++) tot += wcnt[w][tid];
            unsigned int b = tot ? atomicAdd(&d.c->n_work[tid].v, tot) : 0u;
            for (int w = 0; w < DEDUPE_NT / 64; w++) { wbase[w][tid] = b; b += wcnt[w][tid]; }
        }
        __syncthreads();
        if (cls >= 0) {
            const unsigned int w = wbase[wv][cls] + (unsigned int)__popcll(mybal & ((1ULL << lane) - 1));
            if (w < d.work_cap) d.work[cls][w] = nid; else atomicOr(&d.c->overflow, OVF_WORK);
        }
    }
    for (int o = 32; o > 0; o >>= 1) aliases += __shfl_xor(aliases, o, 64);
    if (lane == 0 && aliases) atomicAdd(&d.c->xstat[0][blockIdx.x & (NSHARD - 1)].alias, aliases);
}
