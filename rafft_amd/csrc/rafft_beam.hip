// rafft_beam.hip - beam_step_kernel and its `seen` hash table (gfx950).  Included by rafft_kernels.hip.
#pragma once

// --------------------------------------------------------- beam step kernel

// (round 5: four slots per round trip.  A wavefront waits for the longest probe chain among its 64 lanes - at half load that was four or
//  five dependent trips for a lookup whose expected length is 1.5; the four 16-byte loads are independent and mostly one 64-byte line.
//  `free_sl`: the empty slot that ended the search - where seen_insert_at starts, every slot before it holds another key for good)
__device__ inline bool seen_lookup(const uint64_t *tab, uint32_t cap, uint64_t h1, uint64_t h2, uint32_t &free_sl)
{
    const uint32_t mask = cap - 1;
    uint32_t sl = (uint32_t)h1 & mask;
    const ulonglong2 *t2 = (const ulonglong2 *)tab;
    for (;;) {
        const uint32_t s1 = (sl + 1) & mask, s2 = (sl + 2) & mask, s3 = (sl + 3) & mask;
        ulonglong2 e0 = t2[sl], e1 = t2[s1], e2 = t2[s2], e3 = t2[s3];
        pin(e0); pin(e1); pin(e2); pin(e3);           // (all four in flight: without this the compiler loads a slot when the one before did not decide)
        if (e0.x == 0) { free_sl = sl; return false; }
        if (e0.x == h1 && e0.y == h2) return true;
        if (e1.x == 0) { free_sl = s1; return false; }
        if (e1.x == h1 && e1.y == h2) return true;
        if (e2.x == 0) { free_sl = s2; return false; }
        if (e2.x == h1 && e2.y == h2) return true;
        if (e3.x == 0) { free_sl = s3; return false; }
        if (e3.x == h1 && e3.y == h2) return true;
        sl = (sl + 4) & mask;
    }
}
// insert a key that seen_lookup did not find, starting at the empty slot it stopped at (other threads of the pass may have taken it since)
__device__ inline void seen_insert_at(uint64_t *tab, uint32_t cap, uint64_t h1, uint64_t h2, uint32_t sl)
{
    const uint32_t mask = cap - 1;
    for (;;) {
        unsigned long long old = atomicCAS((unsigned long long *)&tab[2 * (uint64_t)sl], 0ULL, (unsigned long long)h1);
        if (old == 0) { tab[2 * (uint64_t)sl + 1] = h2; return; }
        if (old == h1 && tab[2 * (uint64_t)sl + 1] == h2) return;
        sl = (sl + 1) & mask;
    }
}
// insert unless present; true if it was new.  Keys inserted concurrently by other threads are always
// different structures (distinct combos of one parent), so a half-written entry can only be someone else's.
__device__ inline bool seen_insert_new(uint64_t *tab, uint32_t cap, uint64_t h1, uint64_t h2)
{
    uint32_t mask = cap - 1, sl = (uint32_t)h1 & mask;
    for (;;) {
        unsigned long long old = atomicCAS((unsigned long long *)&tab[2 * (uint64_t)sl], 0ULL, (unsigned long long)h1);
        if (old == 0) { tab[2 * (uint64_t)sl + 1] = h2; return true; }
        if (old == h1 && tab[2 * (uint64_t)sl + 1] == h2) return false;
        sl = (sl + 1) & mask;
    }
}
__device__ inline void seen_insert(uint64_t *tab, uint32_t cap, uint64_t h1, uint64_t h2)
{
    uint32_t mask = cap - 1, sl = (uint32_t)h1 & mask;
    for (;;) {
        unsigned long long old = atomicCAS((unsigned long long *)&tab[2 * (uint64_t)sl], 0ULL, (unsigned long long)h1);
        if (old == 0) { tab[2 * (uint64_t)sl + 1] = h2; return; }
        if (old == h1 && tab[2 * (uint64_t)sl + 1] == h2) return;
        sl = (sl + 1) & mask;
    }
}


// ---- the same set with its occupancy kept in LDS: bit s of `bm` set <=> slot s of the table holds a key.
// A sequence's table is only ever touched by that sequence's workgroup, one beam step at a time, so which slots are taken need not be
// asked of HBM: the workgroup loads the table's bitmap (cap / 8 bytes) when it starts and stores it when its inserts are done.  A
// lookup whose home slot is free - the usual answer, the tables are at most half full - makes no HBM access at all, an insert claims
// its slot with an LDS atomic and writes the entry with one plain 16-byte store, and a table need not be zeroed: a slot is read only
// where its bit is set.
__device__ __forceinline__ bool bm_test(const uint32_t *bm, uint32_t s) { return (bm[s >> 5] >> (s & 31)) & 1u; }
// (the slots of a run of set bits are loaded together, as in seen_lookup; the run's end is known before anything is loaded)
__device__ inline bool seen_lookup_bm(const uint64_t *tab, const uint32_t *bm, uint32_t cap, uint64_t h1, uint64_t h2, uint32_t &free_sl)
{
    const uint32_t mask = cap - 1;
    uint32_t sl = (uint32_t)h1 & mask;
    const ulonglong2 *t2 = (const ulonglong2 *)tab;
    for (;;) {
        if (!bm_test(bm, sl)) { free_sl = sl; return false; }
        const uint32_t s1 = (sl + 1) & mask, s2 = (sl + 2) & mask, s3 = (sl + 3) & mask;
        const bool b1 = bm_test(bm, s1), b2 = b1 && bm_test(bm, s2), b3 = b2 && bm_test(bm, s3);
        ulonglong2 e0 = t2[sl], e1 = make_ulonglong2(0ULL, 0ULL), e2 = e1, e3 = e1;
        if (b1) e1 = t2[s1];
        if (b2) e2 = t2[s2];
        if (b3) e3 = t2[s3];
        pin(e0); pin(e1); pin(e2); pin(e3);
        if (e0.x == h1 && e0.y == h2) return true;
        if (!b1) { free_sl = s1; return false; }
        if (e1.x == h1 && e1.y == h2) return true;
        if (!b2) { free_sl = s2; return false; }
        if (e2.x == h1 && e2.y == h2) return true;
        if (!b3) { free_sl = s3; return false; }
        if (e3.x == h1 && e3.y == h2) return true;
        sl = (sl + 4) & mask;
    }
}
// insert a key that is not in the set, starting at a slot at or before its first free one (seen_lookup_bm's free_sl, or its home slot in
// a table being filled by a rehash).  A slot found taken is never compared: the keys inserted side by side are distinct (wk_tab, the
// keys of a table), and the slot of a concurrent insert may not be written yet - the table is not zeroed, what it holds until then is
// whatever the arena held before, possibly this very key from an earlier wave.
__device__ inline void seen_insert_at_bm(uint64_t *tab, uint32_t *bm, uint32_t cap, uint64_t h1, uint64_t h2, uint32_t sl)
{
    const uint32_t mask = cap - 1;
    for (;;) {
        const uint32_t bit = 1u << (sl & 31);
        if (!(atomicOr(&bm[sl >> 5], bit) & bit)) { ((ulonglong2 *)tab)[sl] = make_ulonglong2((unsigned long long)h1, (unsigned long long)h2); return; }
        sl = (sl + 1) & mask;
    }
}

// move every key of a sequence's `seen` set into a bigger table.  (round 5: four slots per thread read together and their
// compare-and-swaps issued together - one slot at a time was a chain of two or three dependent round trips per slot, 32 slots per
// thread for the first growth: ~60 us of a workgroup's ~250)
// `sbm`: the old table's bitmap - it is read only where a bit is set (null: an empty slot holds zero); `nbm`: the new table's bitmap,
// zeroed by the caller and filled here (null: the new table itself was zeroed, slots are claimed by compare-and-swap)
template <int NT>
__device__ inline void seen_rehash(const uint64_t *stab, uint32_t scap, const uint32_t *sbm, uint64_t *ntab, uint32_t ncap, uint32_t *nbm, int tid)
{
    const ulonglong2 *src = (const ulonglong2 *)stab;
    const uint32_t mask = ncap - 1;
    for (uint32_t base = 0; base < scap; base += NT * 4) {
        ulonglong2 e[4];
        unsigned long long old[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = base + (uint32_t)u * NT + (uint32_t)tid;
            e[u] = i < scap && (!sbm || bm_test(sbm, i)) ? src[i] : make_ulonglong2(0ULL, 0ULL);
        }
        if (nbm) {
#pragma unroll
            for (int u = 0; u < 4; u++) if (e[u].x) seen_insert_at_bm(ntab, nbm, ncap, e[u].x, e[u].y, (uint32_t)e[u].x & mask);
            continue;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { old[u] = 1; if (e[u].x) old[u] = atomicCAS((unsigned long long *)&ntab[2 * (uint64_t)((uint32_t)e[u].x & mask)], 0ULL, (unsigned long long)e[u].x); }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (e[u].x) {
                if (old[u] == 0) ntab[2 * (uint64_t)((uint32_t)e[u].x & mask) + 1] = e[u].y;
                else seen_insert(ntab, ncap, e[u].x, e[u].y);        // home slot taken: the probing insert
            }
    }
}

// The set of sequence `sq` moves into a table of `ncap` slots from the arena (workgroup-uniform call).  The new table is in bitmap
// mode when its bitmap fits the launch's budget `bm_max` (bytes): then it is not zeroed, its bitmap is built in `bm` - the old one,
// if there was one, is parked in `obm` (ncap / 16 bytes at the most) meanwhile.  Otherwise the table is zeroed here (the arena is
// not) and keeps the compare-and-swap protocol from now on.  False: the arena is full (OVF_SEEN is set).
template <int NT>
__device__ inline bool seen_grow(const Dev &d, int sq, uint32_t ncap, uint64_t *&stab, uint32_t &scap, bool &bmode, uint32_t *bm, uint32_t *obm,
                                 uint32_t bm_max, int *sh, int tid)
{
    if (tid == 0) {
        unsigned long long o = atomicAdd(&d.c->seen_top, (unsigned long long)ncap);
        // (a table's bitmap starts at bit `o` of the bitmap arena: whole words, since every table is a power of two >= 2048 slots)
        if (o + ncap > d.seen_cap_total || (o & 31)) { atomicOr(&d.c->overflow, OVF_SEEN); *(unsigned long long *)&sh[8] = ~0ULL; }
        else *(unsigned long long *)&sh[8] = o;
    }
    __syncthreads();
    const unsigned long long o = *(unsigned long long *)&sh[8];
    __syncthreads();
    if (o == ~0ULL) return false;
    uint64_t *ntab = d.seen + 2 * o;
    // (a rare path inside the product walk's loop: the per-thread addresses of the bitmap loops below are formed here, from a copy of
    //  the thread id that the compiler cannot see through - hoisted in front of the walk's loop they would take registers of the walk,
    //  and the 256-thread kernel has none to spare)
    uint32_t t = (uint32_t)tid;
    asm volatile("" : "+v"(t));
    const bool nmode = ncap / 8 <= bm_max;
    const uint32_t *sbm = bmode ? bm : nullptr;
    if (bmode && nmode) {
        for (uint32_t i = t; i < scap / 32; i += NT) obm[i] = bm[i];
        sbm = obm;
        __syncthreads();
    }
    if (nmode) for (uint32_t i = t; i < ncap / 32; i += NT) bm[i] = 0;
    else for (uint32_t i = tid; i < ncap; i += NT) ((ulonglong2 *)ntab)[i] = make_ulonglong2(0ULL, 0ULL);
    __syncthreads();
    seen_rehash<NT>(stab, scap, sbm, ntab, ncap, nmode ? bm : nullptr, tid);
    __syncthreads();
    // (stored at once: the step may accept nothing more, and nobody else stores a bitmap that no insert of the walk changed)
    if (nmode) { uint32_t *gbm = d.seen_bm + o / 32; for (uint32_t i = t; i < ncap / 32; i += NT) gbm[i] = bm[i]; }
    stab = ntab; scap = ncap; bmode = nmode;
    if (tid == 0) { d.seen_off[sq] = o; d.seen_cap[sq] = ncap; d.seen_mode[sq] = nmode ? 1u : 0u; }
    return true;
}

struct ParentInfo {         // filled by the parallel prepass, one entry per beam member
    unsigned long long total, cur;        // product size, cursor
    unsigned long long h1, h2;            // pair-set hash of combo 0 (absolute)
    int dcal0, flag;        // energy of combo 0; flag: 0 live, 1 nothing to produce, 2 cursor already moved
    int sid, nprod;         // structure id; productive regions
    unsigned long long prod;              // productive-region list (global)
    int rl0, nrl;           // this member's regions with >= 2 candidates in the LDS list (rl0 < 0: not resident)
};
static_assert(sizeof(ParentInfo) == 64, "ParentInfo layout");

__device__ __forceinline__ unsigned long long sat_mul(unsigned long long a, unsigned long long b)
{
    const unsigned long long lim = 1ULL << 62;
    if (a == 0 || b == 0) return 0;
    return (a > lim / b) ? lim : a * b;
}

// LDS: sort keys (dynamic) + product description + per-parent prepass records.  `bm_max`: bytes of LDS for the bitmap of the sequence's
// `seen` table, the launch's budget - a table whose bitmap does not fit keeps the compare-and-swap protocol on a zeroed table.
template <int BS_NT>
__global__ __launch_bounds__(BS_NT, BS_NT == 256 ? 5 : 1) void beam_step_kernel(Dev d, int sort_cap, int bm_max)
{
    extern __shared__ __align__(16) unsigned char lds[];
    // region 0 is time-shared: scratch of the product walk (per-thread keys + dedupe table) and behind it the bitmap of the `seen` table
    // (stored back when the walk is over), then the sort keys
    const size_t r0 = max((size_t)8 * (size_t)sort_cap, (size_t)24 * BS_NT + (size_t)bm_max);
    unsigned long long *skey = (unsigned long long *)lds;                       // [sort_cap]
    unsigned long long *wk_h1 = (unsigned long long *)lds;                      // [BS_NT] keys of this chunk's combos
    unsigned long long *wk_h2 = wk_h1 + BS_NT;                                  // [BS_NT]
    unsigned int *wk_tab = (unsigned int *)(wk_h2 + BS_NT);                     // [2 BS_NT] first claimant of a key
    unsigned long long *rl_off = (unsigned long long *)(lds + r0);              // [RL_CAP] candidate offset of a region
    int *rl_cnt = (int *)(rl_off + RL_CAP);                                     // [RL_CAP] its candidate count (>= 2)
    ParentInfo *pinfo = (ParentInfo *)(rl_cnt + RL_CAP);                        // [B]
    unsigned long long *ppre = (unsigned long long *)(pinfo + d.B);             // [B + 1] flat positions of the products
    int *oldbeam = (int *)(ppre + d.B + 1);                                     // [B]
    int *sh = oldbeam + ((d.B + 3) & ~3);                                       // scratch [32], then the prepass's pnode0 [B]
    // (at a fixed address: the bitmap's per-thread addresses cost the product walk's loop no register)
    uint32_t *bm = (uint32_t *)(lds + 24 * BS_NT);                              // [bm_max / 4] occupancy of the `seen` table
    uint32_t *obm = (uint32_t *)lds;                                            // ... of the old table while a set grows (in wk_h1 / wk_h2)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int sq = blockIdx.x;
    // snapshot of the region allocators: whatever materialize adds after this kernel is "new"
    if (sq == 0 && tid < NSHARD) d.c->node_prev[tid].v = d.c->node[tid].v;
    // the expand kernels of this step are done with their work lists: reset them for dedupe_kernel / the next step
    if (sq == 0 && tid < NCLS) d.c->n_work[tid].v = 0;
    if (sq == 0) for (int i = tid; i < NCLS * NSHARD; i += BS_NT) d.c->wcur[i / NSHARD][i % NSHARD].v = 0;
    if (sq == 0 && tid < NCLS) d.c->wdone[tid] = 0;
    if (d.done[sq]) return;
    // an arena overflowed while the last step's structures were materialized: some child slots were claimed and never filled, some
    // node lists point at them.  Nothing of that step may be read; the host sees the flag in this step's read-back and regrows.
    // (one thread looks: other workgroups of this launch may set the flag while this one starts)
    if (tid == 0) sh[27] = d.c->overflow != 0 ? 1 : 0;
    __syncthreads();
    if (sh[27]) return;
    const int nbeam = d.beam_n[sq];
    const int step_no = d.nsteps[sq];          // (read by everyone before the barrier below; thread 0 counts the step after it)
    int *beam = d.beam + (size_t)sq * d.B;
    for (int i = tid; i < nbeam; i += BS_NT) oldbeam[i] = beam[i];
    __syncthreads();

    // glob_traj += [glob_tree]   (rafft/rafft.py:161)
    if (d.traj) {
        if (tid == 0) {
            unsigned long long r = atomicAdd(&d.c->trec_n, 1ULL);
            unsigned long long o = atomicAdd(&d.c->tsid_top, (unsigned long long)nbeam);
            if (r >= d.trec_cap || o + nbeam > d.tsid_cap) { atomicOr(&d.c->overflow, OVF_TRAJ); sh[0] = -1; }
            else { d.trec[r] = make_int4(sq, d.nsteps[sq], nbeam, (int)o); sh[0] = (int)o; }
        }
        __syncthreads();
        int o = sh[0];
        if (o >= 0) for (int i = tid; i < nbeam; i += BS_NT) d.tsid[o + i] = oldbeam[i];
        __syncthreads();
    }
    if (tid == 0) d.nsteps[sq] += 1;

    // ---- prepass: product size and combo 0 of every parent, its productive regions as a compact list in HBM (written on the first
    // visit, read back by later product walks and by materialize_kernel) and its regions with a real choice (>= 2 candidates) as a
    // (count, offset) list in LDS.
    // Round 5: FLAT over (beam member, region) items.  Every member costs a chain of dependent loads - structure row -> node list ->
    // child slot -> region header -> first candidate - and the kernel lives on how many of those chains are in flight at once: a group
    // of 8 / 16 / 64 lanes per member walked the 50 members of a beam in two to thirteen passes of nine dependent round trips each (the
    // row's fields, the list allocation and the header's two words were trips of their own).  Now one thread per member reads its whole
    // row (one trip), a prefix sum over the region counts numbers the items, and one thread per item runs the remaining four trips -
    // 200 items of a short sequence's beam in ONE pass of a 256-thread workgroup; sums go to the member's record with LDS atomics, the
    // lists are placed by a workgroup-wide prefix sum (member-major, node order: rafft/rafft.py:166-171).
    {
        unsigned long long *istart = ppre;                 // [B + 1] first item of a member (ppre proper is written after the prepass)
        int *pnode0 = sh + 32;                             // [B] first node-list entry of a member on its first visit
        unsigned int irun = 0;
        if (tid == 0) sh[28] = 0;                          // regions of this step's first visits
        __syncthreads();
        for (int b0 = 0; b0 < nbeam; b0 += BS_NT) {
            const int b = b0 + tid;
            int ic = 0;
            if (b < nbeam) {
                const int sid = oldbeam[b];
                // the whole row, one round trip (seven 16-byte loads pinned: as a struct copy the compiler split it into the fields each
                // branch below uses and loaded them there - two or three dependent trips)
                StRec r;
                {
                    const uint4 *rp = (const uint4 *)&d.st[sid];
                    uint4 q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3], q4 = rp[4], q5 = rp[5], q6 = rp[6];
                    pin(q0); pin(q1); pin(q2); pin(q3); pin(q4); pin(q5); pin(q6);
                    auto u64 = [](unsigned int lo, unsigned int hi) { return (unsigned long long)lo | ((unsigned long long)hi << 32); };
                    r.dcal = (int)q0.y; r.node0 = (int)q0.z; r.nnodes = (int)q0.w; r.nprod = (int)q1.y; r.c0d = (int)q1.z;
                    r.h1 = u64(q2.x, q2.y); r.h2 = u64(q2.z, q2.w); r.cursor = u64(q3.z, q3.w); r.total = u64(q4.z, q4.w);
                    r.prod = u64(q5.x, q5.y); r.c0h1 = u64(q5.z, q5.w); r.c0h2 = u64(q6.x, q6.y);
                }
                ParentInfo pi;
                pi.sid = sid; pi.rl0 = 0; pi.nrl = 0; pi.prod = 0; pi.nprod = 0; pi.total = 0; pi.cur = 0; pi.h1 = 0; pi.h2 = 0; pi.dcal0 = 0;
                if (r.total && r.cursor >= r.total) pi.flag = 1;                       // product exhausted
                else if (r.total && r.cursor > 0) {      // expanded in an earlier step: cursor, total and combo 0 are on record
                    pi.flag = 2; pi.total = r.total; pi.cur = r.cursor; pi.h1 = r.c0h1; pi.h2 = r.c0h2; pi.dcal0 = r.c0d;
                    pi.prod = r.prod; pi.nprod = r.nprod; ic = r.nprod;
                } else {                                  // first visit: combo 0 = the first candidate of every region that has one
                    pi.flag = 0; pi.total = 1; pi.h1 = r.h1; pi.h2 = r.h2; pi.dcal0 = r.dcal;
                    pnode0[b] = r.node0; ic = r.nnodes;
                    if (ic) atomicAdd(&sh[28], ic);
                }
                pinfo[b] = pi;
            }
            int tot, ex = block_exscan<BS_NT>(ic, sh, &tot);
            if (b < nbeam) istart[b] = irun + (unsigned int)ex;
            irun += (unsigned int)tot;
            __syncthreads();
        }
        const int nitems = (int)irun;
        // ONE allocation for the productive-region lists of all first visits of the step (at most one entry per region): a returning
        // atomic per member was 50 per sequence and step on the 64 sub-arena counters - same-address atomics are served one after the
        // other (1.20 -> 1.29 ms per batch).  The sub-arena rotates with the step, so that a lone sequence spreads over all of them.
        // The answer is needed when the lists are written, i.e. after the item loads below are under way: kept in a register till then.
        const int nfirst = sh[28], pshard = (sq + step_no) & (NSHARD - 1);
        unsigned long long pb_raw = 0, pball = 0;
        if (tid == BS_NT - 1 && nfirst) pb_raw = atomicAdd(&d.c->prod[pshard].v, (unsigned long long)nfirst);
        unsigned int run1 = 0, run2 = 0;
        for (int t0 = 0; t0 < nitems; t0 += BS_NT) {
            const int t = t0 + tid;
            int b = -1, i = 0, cnt = 0, cn = -1, first = 0;
            unsigned long long coff = 0;
            if (t < nitems) {
                int lo = 0, hi = nbeam - 1;              // the last member whose items start at or before t
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (istart[mid] <= (unsigned long long)t) lo = mid; else hi = mid - 1; }
                b = lo; i = t - (int)istart[b];
                first = pinfo[b].flag == 0 ? 1 : 0;
                if (first) {
                    cn = d.nlist[pnode0[b] + i];
                    // (written by materialize_kernel as -(slot + 1): the region that hangs in that child slot - created there by
                    //  whichever beam member asked first, or the known loop dedupe_kernel found for it)
                    if (cn < 0) cn = (int)(((const uint32_t *)d.cslot)[-cn - 1] & 0x7FFFFFFFu) - 1;
                    if (cn >= 0) { cnt = d.nd[cn].ncand; coff = d.nd[cn].cand; }
                    if (cnt > 0) {
                        const Cand *cp = &d.cand[coff];
                        const int dd = cp->ddcal;
                        const ulonglong2 hh = *(const ulonglong2 *)&cp->h1;
                        atomicAdd(&pinfo[b].dcal0, dd);
                        atomicAdd(&pinfo[b].h1, hh.x); atomicAdd(&pinfo[b].h2, hh.y);
                        if (cnt >= 2) {                  // product size: a saturating product commutes (every factor >= 1)
                            unsigned long long old = pinfo[b].total, seen_;
                            do { seen_ = old; old = atomicCAS(&pinfo[b].total, seen_, sat_mul(seen_, (unsigned long long)cnt)); } while (old != seen_);
                        }
                    }
                } else {
                    const ProdEnt pe = d.prod[pinfo[b].prod + i];
                    cnt = (int)pe.cnt; coff = pe.off; cn = pe.node;
                }
            }
            if (t0 == 0 && tid == BS_NT - 1) {
                unsigned long long v = pb_raw;
                if (v + (unsigned long long)nfirst > d.prod_shard_cap) { atomicOr(&d.c->overflow, OVF_PRODLIST); v = ~0ULL; }
                else v += (unsigned long long)pshard * d.prod_shard_cap;
                *(unsigned long long *)&sh[30] = v;
            }
            const int f1 = (first && cnt > 0) ? 1 : 0, f2 = cnt >= 2 ? 1 : 0;
            int tot12, ex12 = block_exscan<BS_NT>(f1 | (f2 << 16), sh, &tot12);      // (barriers inside: sh[30] is there for everyone)
            if (t0 == 0) pball = *(const unsigned long long *)&sh[30];
            const unsigned int pos1 = run1 + (unsigned int)(ex12 & 0xFFFF), pos2 = run2 + (unsigned int)(ex12 >> 16);
            if (b >= 0) {
                if (i == 0) { pinfo[b].rl0 = (int)pos2; if (first) pinfo[b].prod = pball == ~0ULL ? ~0ULL : pball + pos1; }
                if (f1) {
                    atomicAdd(&pinfo[b].nprod, 1);
                    if (pball != ~0ULL) { ProdEnt pe; pe.cnt = (uint32_t)cnt; pe.node = cn; pe.off = coff; d.prod[pball + pos1] = pe; }
                }
                if (f2) {
                    atomicAdd(&pinfo[b].nrl, 1);
                    if ((int)pos2 < d.rl_cap) { rl_cnt[pos2] = cnt; rl_off[pos2] = coff; }
                }
            }
            run1 += (unsigned int)(tot12 & 0xFFFF); run2 += (unsigned int)(tot12 >> 16);
            __syncthreads();
        }
        for (int b = tid; b < nbeam; b += BS_NT) {
            ParentInfo pi = pinfo[b];
            if (pi.flag == 1) continue;
            if (pi.nrl == 0) pi.rl0 = 0;
            else if (pi.rl0 + pi.nrl > d.rl_cap) pi.rl0 = -1;      // a list that does not fit whole is read from HBM by the walk
            if (pi.flag == 0) {
                if (pi.prod == ~0ULL) { pi.prod = 0; pi.nprod = 0; pi.nrl = 0; pi.rl0 = 0; pi.total = 1; }
                const int np = pi.nprod;
                if (np > d.max_prod) atomicOr(&d.c->overflow, OVF_PROD);     // materialize_kernel's limit
                if (np > 64) atomicMax(&d.c->max_nprod, (unsigned int)np);
                StRec *sr = &d.st[pi.sid];
                sr->prod = pi.prod; sr->nprod = np; sr->c0h1 = pi.h1; sr->c0h2 = pi.h2; sr->c0d = pi.dcal0;
                if (np == 0) { pi.flag = 1; sr->total = 1; sr->cursor = 1; }
            }
            pinfo[b] = pi;
        }
    }
    __syncthreads();

    // ---- the product walk (rafft/rafft.py:173-204), flat over all parents: position p of the walk is combo
    // cur_b + (p - ppre[b]) of the parent b whose range holds p, in beam order and itertools.product order.
    // One chunk of BS_NT consecutive positions per pass - usually several whole parents at once.
    if (wv == 0) {
        unsigned long long carry = 0;
        const unsigned long long LIM = 1ULL << 63;
        for (int base = 0; base < nbeam; base += 64) {
            const int b = base + lane;
            unsigned long long rem = 0;
            if (b < nbeam && !(pinfo[b].flag & 1)) rem = pinfo[b].total - pinfo[b].cur;
            unsigned long long x = rem;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long y = __shfl_up(x, o, 64);
                if (lane >= o) x = (x > LIM - y) ? LIM : x + y;
            }
            unsigned long long incl = (x > LIM - carry) ? LIM : x + carry;
            if (b < nbeam) ppre[b + 1] = incl;
            carry = __shfl(incl, 63, 64);
        }
        if (lane == 0) ppre[0] = 0;
    }
    // the `seen` table of this sequence: in bitmap mode its occupancy bitmap comes into LDS (a table in compare-and-swap mode was
    // zeroed by the host, or by seen_grow when it was handed out)
    uint64_t *stab = d.seen + 2 * d.seen_off[sq];
    uint32_t scap = d.seen_cap[sq], scnt = d.seen_cnt[sq];
    bool bmode = d.seen_mode[sq] != 0;
    if (bmode && scap / 8 > (uint32_t)bm_max) {       // (never: the host hands a launch no table in bitmap mode beyond its budget)
        if (tid == 0) atomicOr(&d.c->overflow, OVF_SEEN);
        d.done[sq] = 1;
        return;
    }
    if (bmode) {
        const uint32_t *gbm = d.seen_bm + (size_t)(stab - d.seen) / 64;
#pragma unroll 1
        for (uint32_t i = tid; i < scap / 32; i += BS_NT) bm[i] = gbm[i];
    }
    bool seen_full = false;        // the arena had no bigger table left (OVF_SEEN): the walk stops, the sequence leaves once the bitmap is stored
    for (int i = tid; i < 2 * BS_NT; i += BS_NT) wk_tab[i] = 0;
    __syncthreads();
    const size_t chb = (size_t)sq * d.ch_cap;
    int nb_branch = 0, nchild = 0;
    int single_from = nbeam;
    // once nb_branch >= max_branch every later parent only replays its combo 0
    // (rafft/rafft.py:202-203): those are handled together, in parallel, after this loop
    if (d.max_branch <= 0) single_from = 0;
    const unsigned long long Ptot = ppre[nbeam];
    unsigned long long W = 0;
    while (single_from == nbeam && W < Ptot) {
        const unsigned long long left = Ptot - W;
        const int chunk = left < (unsigned long long)BS_NT ? (int)left : BS_NT;
        if ((unsigned long long)(scnt + chunk) * 2 > scap) {   // grow the seen set (rehash into a bigger table)
            uint32_t ncap = scap;
            while ((unsigned long long)(scnt + BS_NT) * 2 > ncap) ncap <<= 1;
            if (!seen_grow<BS_NT>(d, sq, ncap, stab, scap, bmode, bm, obm, (uint32_t)bm_max, sh, tid)) { seen_full = true; break; }
        }
        const int need = d.max_branch - nb_branch;      // > 0
        int b = 0, sidb = 0, cd = 0, slot = -1;
        uint32_t free_sl = 0;
        bool cand_new = false, last_combo = false;
        unsigned long long idx = 0, totb = 0, h1 = 0, h2 = 0;
        const unsigned long long pos = W + (unsigned long long)tid;
        if (tid < chunk) {
            int lo = 0, hi = nbeam - 1;                  // the last member whose range starts at or before pos
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ppre[mid] <= pos) lo = mid; else hi = mid - 1; }
            b = lo;
            const ParentInfo pi = pinfo[b];
            sidb = pi.sid; totb = pi.total;
            idx = pi.cur + (pos - ppre[b]);
            last_combo = idx == totb - 1;
            // combo idx = combo 0 with the digits of idx (mixed radix over the regions with a choice, last
            // region fastest) swapped in
            unsigned long long a1 = pi.h1, a2 = pi.h2, rest = idx;
            int ad = pi.dcal0;
            auto divmod = [&](unsigned int c, unsigned int &r) {
                if (rest < (1ULL << 24)) {
                    const unsigned int v = (unsigned int)rest;
                    unsigned int q = (unsigned int)((float)v * __frcp_rn((float)c));       // off by one at most
                    int rr = (int)(v - q * c);
                    if (rr < 0) { q--; rr += (int)c; } else if (rr >= (int)c) { q++; rr -= (int)c; }
                    r = (unsigned int)rr; rest = q;
                } else { const unsigned long long q = rest / c; r = (unsigned int)(rest - q * c); rest = q; }
            };
            if (pi.rl0 >= 0) {
                int j = pi.nrl - 1;
                // up to four changed digits are located first and their candidates loaded together
                // (round 5: digits that did not change point both at the arena's first record - the eight records are loaded unconditionally,
                //  i.e. together, one round trip; loads behind `if (changed)` were one dependent trip per changed digit)
                const Cand *const same = d.cand;
                const Cand *pn0 = same, *pn1 = same, *pn2 = same, *pn3 = same, *po0 = same, *po1 = same, *po2 = same, *po3 = same;
                auto next = [&](const Cand *&pn, const Cand *&po) {
                    while (j >= 0 && rest) {
                        unsigned int r;
                        divmod((unsigned int)rl_cnt[pi.rl0 + j], r);
                        j--;
                        if (r) { po = &d.cand[rl_off[pi.rl0 + j + 1]]; pn = po + r; return; }
                    }
                };
                next(pn0, po0); next(pn1, po1); next(pn2, po2); next(pn3, po3);
                {
                    const int dn0 = pn0->ddcal, dn1 = pn1->ddcal, dn2 = pn2->ddcal, dn3 = pn3->ddcal, do0 = po0->ddcal, do1 = po1->ddcal, do2 = po2->ddcal, do3 = po3->ddcal;
                    const ulonglong2 hn0 = *(const ulonglong2 *)&pn0->h1, hn1 = *(const ulonglong2 *)&pn1->h1, hn2 = *(const ulonglong2 *)&pn2->h1, hn3 = *(const ulonglong2 *)&pn3->h1;
                    const ulonglong2 ho0 = *(const ulonglong2 *)&po0->h1, ho1 = *(const ulonglong2 *)&po1->h1, ho2 = *(const ulonglong2 *)&po2->h1, ho3 = *(const ulonglong2 *)&po3->h1;
                    ad += (dn0 - do0) + (dn1 - do1) + (dn2 - do2) + (dn3 - do3);
                    a1 += (hn0.x - ho0.x) + (hn1.x - ho1.x) + (hn2.x - ho2.x) + (hn3.x - ho3.x);
                    a2 += (hn0.y - ho0.y) + (hn1.y - ho1.y) + (hn2.y - ho2.y) + (hn3.y - ho3.y);
                }
                while (j >= 0 && rest) {
                    const Cand *pn = same, *po = same;
                    next(pn, po);
                    ad += pn->ddcal - po->ddcal; a1 += pn->h1 - po->h1; a2 += pn->h2 - po->h2;
                }
            } else {
                // region list not resident in LDS (more than RL_CAP regions with a choice in this beam)
                for (int j = pi.nprod - 1; j >= 0 && rest; j--) {
                    const ProdEnt pe = d.prod[pi.prod + j];
                    if (pe.cnt < 2) continue;
                    unsigned int r;
                    divmod(pe.cnt, r);
                    if (r) { const Cand *po = &d.cand[pe.off], *pn = po + r; ad += pn->ddcal - po->ddcal; a1 += pn->h1 - po->h1; a2 += pn->h2 - po->h2; }
                }
            }
            h1 = a1 ? a1 : 1; h2 = a2 ? a2 : 1; cd = ad;
            wk_h1[tid] = h1; wk_h2[tid] = h2;
            cand_new = bmode ? !seen_lookup_bm(stab, bm, scap, h1, h2, free_sl) : !seen_lookup(stab, scap, h1, h2, free_sl);
        }
        // the same structure can come from several parents of this chunk: its first position wins (`seen` order)
        if (cand_new) {
            unsigned int sl = (unsigned int)(h1 ^ (h1 >> 32)) & (2 * BS_NT - 1);
            for (;;) {
                const unsigned int old = atomicCAS(&wk_tab[sl], 0u, (unsigned int)tid + 1u);
                if (old == 0) break;
                if (wk_h1[old - 1] == h1 && wk_h2[old - 1] == h2) { atomicMin(&wk_tab[sl], (unsigned int)tid + 1u); break; }
                sl = (sl + 1) & (2 * BS_NT - 1);
            }
            slot = (int)sl;
        }
        __syncthreads();
        const bool isnew = cand_new && wk_tab[slot < 0 ? 0 : slot] == (unsigned int)tid + 1u;
        const unsigned long long bal = __ballot(isnew);
        if (lane == 0) sh[wv] = __popcll(bal);
        __syncthreads();
        int ex = __popcll(bal & ((1ULL << lane) - 1)), tot = 0;
        for (int w = 0; w < BS_NT / 64; w++) { const int t = sh[w]; if (w < wv) ex += t; tot += t; }
        const bool hit = tot >= need;
        const bool accepted = isnew && ex < need;
        if (accepted) {
            const int ci2 = nchild + ex;
            if (ci2 < d.ch_cap) {
                d.ch_parent[chb + ci2] = (uint16_t)b;
                d.ch_combo[chb + ci2] = idx;
                d.ch_dcal[chb + ci2] = cd;
                d.ch_h[2 * (chb + ci2)] = h1;
                d.ch_h[2 * (chb + ci2) + 1] = h2;
            } else atomicOr(&d.c->overflow, OVF_SORT);
            if (bmode) seen_insert_at_bm(stab, bm, scap, h1, h2, free_sl);
            else seen_insert_at(stab, scap, h1, h2, free_sl);
        }
        if (hit) {
            // the reference stops walking after the combo that brings nb_branch to max_branch
            if (accepted && ex == need - 1) {
                sh[21] = b; *(unsigned long long *)&sh[22] = pos;
                d.st[sidb].cursor = idx + 1; d.st[sidb].total = totb;
            }
            __syncthreads();
            const unsigned long long hpos = *(unsigned long long *)&sh[22];
            if (tid < chunk && last_combo && pos < hpos) { d.st[sidb].cursor = totb; d.st[sidb].total = totb; }
            nchild += need; nb_branch += need; scnt += need;
            single_from = sh[21] + 1;
            __syncthreads();
            break;
        }
        if (tid < chunk && last_combo) { d.st[sidb].cursor = totb; d.st[sidb].total = totb; }   // product exhausted
        nchild += tot; nb_branch += tot; scnt += tot;
        W += (unsigned long long)chunk;
        for (int i = tid; i < 2 * BS_NT; i += BS_NT) wk_tab[i] = 0;
        __syncthreads();
    }
    if (single_from < nbeam && !seen_full) {
        // ---- parents in "one combo then break" mode: combo 0 of each (from the prepass), accepted in
        // beam order if its structure is new; a parent whose cursor already moved replays a known combo
        const int nrest = nbeam - single_from;
        if ((unsigned long long)(scnt + nrest) * 2 > scap) {
            uint32_t ncap = scap;
            while ((unsigned long long)(scnt + nrest + BS_NT) * 2 > ncap) ncap <<= 1;
            if (!seen_grow<BS_NT>(d, sq, ncap, stab, scap, bmode, bm, obm, (uint32_t)bm_max, sh, tid)) seen_full = true;
        }
        for (int base = single_from; base < nbeam && !seen_full; base += BS_NT) {
            const int b = base + tid;
            int isnew = 0;
            uint32_t free_sl = 0;
            uint64_t h1 = 0, h2 = 0;
            if (b < nbeam && pinfo[b].flag == 0) {       // live and cursor == 0
                h1 = pinfo[b].h1; h2 = pinfo[b].h2;
                if (h1 == 0) h1 = 1;
                if (h2 == 0) h2 = 1;
                isnew = (bmode ? seen_lookup_bm(stab, bm, scap, h1, h2, free_sl) : seen_lookup(stab, scap, h1, h2, free_sl)) ? 0 : 1;
                // an earlier parent of this phase producing the same structure wins (`seen` order)
                for (int e = single_from; isnew && e < b; e++)
                    if (pinfo[e].flag == 0) {
                        uint64_t g1 = pinfo[e].h1, g2 = pinfo[e].h2;
                        if (g1 == 0) g1 = 1;
                        if (g2 == 0) g2 = 1;
                        if (g1 == h1 && g2 == h2) isnew = 0;
                    }
            }
            int tot, ex = block_exscan_flag<BS_NT>(isnew, sh, &tot);
            if (isnew) {
                const int ci2 = nchild + ex;
                if (ci2 < d.ch_cap) {
                    d.ch_parent[chb + ci2] = (uint16_t)b;
                    d.ch_combo[chb + ci2] = 0;
                    d.ch_dcal[chb + ci2] = pinfo[b].dcal0;
                    d.ch_h[2 * (chb + ci2)] = h1;
                    d.ch_h[2 * (chb + ci2) + 1] = h2;
                } else atomicOr(&d.c->overflow, OVF_SORT);
                if (bmode) seen_insert_at_bm(stab, bm, scap, h1, h2, free_sl);
                else seen_insert_at(stab, scap, h1, h2, free_sl);
            }
            if (b < nbeam && pinfo[b].flag == 0) { d.st[oldbeam[b]].cursor = 1; d.st[oldbeam[b]].total = pinfo[b].total; }
            nchild += tot; nb_branch += tot; scnt += tot;
            __syncthreads();
        }
    }
    // (every insert of this step lies before a barrier: the pass's own, or the one that ends a round of the loop above)
    // The bitmap goes back to HBM, before the sort keys take its place - and before any return: the step's entries are in the table,
    // their bits must not be lost.  (A table that seen_grow filled is stored there.)
    if (bmode) {
        if (nchild > 0) {
            uint32_t *gbm = d.seen_bm + (size_t)(stab - d.seen) / 64;
#pragma unroll 1
            for (uint32_t i = tid; i < scap / 32; i += BS_NT) gbm[i] = bm[i];
        }
        __syncthreads();           // (the sort keys below overwrite the bitmap's LDS)
    }
    if (seen_full) { d.done[sq] = 1; return; }
    if (tid == 0) { d.seen_cnt[sq] = scnt; atomicAdd(&d.c->xstat[1][sq & (NSHARD - 1)].children, (unsigned long long)nchild); }
    if (nchild > d.ch_cap) nchild = d.ch_cap;

    // ---- new = children + beam, stable sort by energy, cut (rafft/rafft.py:206-210)
    const int N = nchild + nbeam;
    if (N > sort_cap) { if (tid == 0) atomicOr(&d.c->overflow, OVF_SORT); d.done[sq] = 1; return; }
    for (int i = tid; i < N; i += BS_NT) {
        unsigned long long key;
        if (i < nchild) key = ((unsigned long long)(uint32_t)(d.ch_dcal[chb + i] + 0x40000000) << 32) | (uint32_t)i;
        else key = ((unsigned long long)(uint32_t)(d.st[oldbeam[i - nchild]].dcal + 0x40000000) << 32) | (uint32_t)i;
        skey[i] = key;
    }
    __syncthreads();
    {
        // only the max_stack best survive: select them exactly (radix select), then sort just those
        const int K = N < d.B ? N : d.B;
        select_smallest_inplace<BS_NT>(skey, N, K, rl_cnt, sh);
        if (K <= RL_CAP) {
            // order the selected keys by counting (round 4): the rank of a key is the number of smaller ones among the K (they are
            // distinct), and it goes straight to its place - two barriers where the bitonic sort of 64 keys takes 21
            unsigned long long *outk = rl_off;              // (the region list of the product walk is dead by now; RL_CAP entries)
            for (int i = tid; i < K; i += BS_NT) {
                const unsigned long long ki = skey[i];
                int r = 0;
                for (int j = 0; j < K; j++) r += skey[j] < ki ? 1 : 0;
                outk[r] = ki;
            }
            __syncthreads();
            for (int i = tid; i < K; i += BS_NT) skey[i] = outk[i];
            __syncthreads();
        } else {
        int M = 2; while (M < K) M <<= 1;
        for (int i = K + tid; i < M; i += BS_NT) skey[i] = ~0ULL;
        __syncthreads();
        for (int k2 = 2; k2 <= M; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < M; i += BS_NT) {
                    int ixj = i ^ j;
                    if (ixj > i) {
                        unsigned long long a = skey[i], bb = skey[ixj];
                        bool up = (i & k2) == 0;
                        if (up ? a > bb : a < bb) { skey[i] = bb; skey[ixj] = a; }
                    }
                }
                __syncthreads();
            }
        }
    }
    const int nnew = N < d.B ? N : d.B;
    // children among the survivors
    int nsurv_child = 0;
    for (int base = 0; base < nnew; base += BS_NT) {
        int i = base + tid, f = 0;
        if (i < nnew) f = ((uint32_t)skey[i] < (uint32_t)nchild) ? 1 : 0;
        int tot, ex = block_exscan_flag<BS_NT>(f, sh, &tot);
        (void)ex;
        nsurv_child += tot;
        __syncthreads();
    }
    if (nsurv_child == 0) {   // same structures as before: fixed point (rafft/rafft.py:213-214)
        if (tid == 0) {
            d.done[sq] = 1;
            atomicAdd(&d.c->n_done, 1u);
            if (!d.traj) {
                unsigned long long r = atomicAdd(&d.c->trec_n, 1ULL);
                unsigned long long o = atomicAdd(&d.c->tsid_top, (unsigned long long)nbeam);
                if (r >= d.trec_cap || o + nbeam > d.tsid_cap) atomicOr(&d.c->overflow, OVF_TRAJ);
                else {
                    d.trec[r] = make_int4(sq, 0, nbeam, (int)o);
                    for (int i = 0; i < nbeam; i++) d.tsid[o + i] = oldbeam[i];
                }
            }
        }
        return;
    }
    if (tid == 0) {
        unsigned long long sb = atomicAdd(&d.c->n_struct, (unsigned long long)nsurv_child);
        unsigned int mb = atomicAdd(&d.c->n_mat, (unsigned int)nsurv_child);
        atomicAdd(&d.c->xstat[1][sq & (NSHARD - 1)].struct_len, (unsigned long long)nsurv_child * (unsigned long long)d.seq_len[sq]);
        if (sb + nsurv_child > d.st_cap || mb + nsurv_child > d.mat_cap) { atomicOr(&d.c->overflow, OVF_STRUCT); sh[24] = -1; }
        else { sh[24] = (int)sb; sh[25] = (int)mb; }
    }
    __syncthreads();
    const int sbase = sh[24], mbase = sh[25];
    __syncthreads();
    if (sbase < 0) { d.done[sq] = 1; return; }
    int run = 0;
    const int Lsq = d.seq_len[sq];
    const unsigned long long soff_sq = (unsigned long long)d.seq_off[sq];
    for (int base = 0; base < nnew; base += BS_NT) {
        int i = base + tid, f = 0;
        uint32_t ord = 0;
        if (i < nnew) { ord = (uint32_t)skey[i]; f = (ord < (uint32_t)nchild) ? 1 : 0; }
        // the child's record: five loads issued together, under way while the ranks below are counted (interleaved with the stores they
        // feed they were three or four dependent round trips)
        int c_dcal = 0;
        unsigned int c_par = 0;
        unsigned long long c_combo = 0;
        ulonglong2 c_h = make_ulonglong2(0ULL, 0ULL);
        if (f) {
            const size_t c = chb + ord;
            c_dcal = d.ch_dcal[c]; c_par = d.ch_parent[c]; c_combo = d.ch_combo[c]; c_h = *(const ulonglong2 *)&d.ch_h[2 * c];
        }
        int tot, ex = block_exscan_flag<BS_NT>(f, sh, &tot);
        if (i < nnew) {
            if (f) {
                pin(c_dcal); pin(c_par); pin(c_combo); pin(c_h);
                const int sid = sbase + run + ex;
                const ParentInfo &pp_ = pinfo[c_par];
                StRec *sr = &d.st[sid];
                sr->seq = sq; sr->dcal = c_dcal; sr->h1 = c_h.x; sr->h2 = c_h.y; sr->parent = oldbeam[c_par]; sr->combo = c_combo;
                sr->cursor = 0; sr->total = 0; sr->nnodes = 0;
                MatRec mr;
                mr.sid = sid; mr.sq = sq; mr.L = Lsq; mr.dcal = c_dcal; mr.nprod = pp_.nprod; mr.pad = 0;
                mr.combo = c_combo; mr.prod = pp_.prod; mr.soff = soff_sq;
                d.mat[mbase + run + ex] = mr;
                beam[i] = sid;
            } else
                beam[i] = oldbeam[ord - nchild];
        }
        run += tot;
        __syncthreads();
    }
    if (tid == 0) d.beam_n[sq] = nnew;
}
