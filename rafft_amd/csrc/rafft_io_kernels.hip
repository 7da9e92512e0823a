// rafft_io_kernels.hip - stage_in_kernel, init_roots_kernel, output_kernel, eval_kernel: what goes into a wave and what
// comes out of it (gfx950).  Included by rafft_kernels.hip.
#pragma once

// ------------------------------------------------------------- init kernel

// The inputs of a wave, from its pinned staging chunk into the device buffers: up to eight segments copied by one kernel that reads
// the host memory itself (hipHostMalloc memory is mapped into the device's address space).  Round 5: as hipMemcpyAsync calls the first
// of these uploads now and then kept the scheduler thread - i.e. every wave in flight - for 12-19 ms (six bench runs in ten on one
// box, the runtime's copy path waiting for something of its own); a kernel launch never waits.
struct StageIn { const uint32_t *src[8]; uint32_t *dst[8]; unsigned long long words[8]; int n; };
__global__ __launch_bounds__(256) void stage_in_kernel(StageIn si)
{
    for (int k = 0; k < si.n; k++) {
        const uint32_t *src = si.src[k];
        uint32_t *dst = si.dst[k];
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < si.words[k]; i += (unsigned long long)gridDim.x * 256) dst[i] = src[i];
    }
}

__global__ void init_roots_kernel(Dev d)
{
    const int sq = blockIdx.x, tid = threadIdx.x;
    const int L = d.seq_len[sq];
    // structure sq / node sq are the unfolded structure and its single region (rafft.py:224-231)
    const unsigned long long off = (unsigned long long)d.seq_off[sq];
    for (int x = tid; x < L; x += blockDim.x) d.pos[off + x] = (uint16_t)(d.pos_packed ? x | (d.codes[off + x] << 12) : x);

    if (tid == 0) {
        d.st[sq].seq = sq; d.st[sq].dcal = 0; d.st[sq].h1 = 0; d.st[sq].h2 = 0;
        d.st[sq].sp = 0; d.st[sq].nsp = 0; d.st[sq].node0 = sq; d.st[sq].nnodes = L > 0 ? 1 : 0; d.st[sq].cursor = 0; d.st[sq].total = 0;
        d.st[sq].parent = -1; d.st[sq].combo = 0;
        d.nd[sq].seq = sq; d.nd[sq].pdcal = 0; d.nd[sq].pos = off; d.nd[sq].n = L; d.nd[sq].ci = -1; d.nd[sq].cj = L;
        d.nd[sq].L = L; d.nd[sq].soff = off;
        d.nd[sq].br = 0; d.nd[sq].nbr = 0; d.nlist[sq] = sq;
        d.nd[sq].ncand = -1; d.nd[sq].cand = 0;
        d.beam[(size_t)sq * d.B] = sq; d.beam_n[sq] = 1; d.nsteps[sq] = 0;
        d.done[sq] = L > 0 ? 0 : 1;
        d.seen_cnt[sq] = 0;       // (seen_off / seen_cap: uploaded by the host - tables sized from the lengths)
        // bitmap mode (the host zeroed the bitmap) or, beyond the first launch's bitmap budget, a table that the host zeroed
        d.seen_mode[sq] = d.seen_cap[sq] / 8 <= d.seen_bm0 ? 1u : 0u;
        if (L > 0) {
            int cls = node_class(L, L, 0, 0, d.cls1_P, d.cls1_br);
            unsigned int w = atomicAdd(&d.c->n_work[cls].v, 1u);
            d.work[cls][w] = sq;
        }
    }
}

// ----------------------------------------------------------- output kernel

// One record = the beam of one sequence at one step (all of them with traj, the last one otherwise); its rows
// go out back to back, `off` bytes into the result buffer, row numbers from `row0`.
struct OutRec { long long off; int row0, w, cnt, L; };
// The dot-bracket rows are made HERE: a structure is stored as the pairs it added to its parent's (materialize kernels), so a row is
// the unfolded one (rafft.py:224-231) with the stems of the whole lineage marked (rafft/rafft.py:97,127-128) - built in LDS (dynamic,
// the longest sequence of the wave) and written out once.
__global__ void output_kernel(Dev d, int nrows, int nrec, const OutRec *recs, char *out_db, int *out_dcal)
{
    extern __shared__ __align__(16) uint8_t out_row[];
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        int lo = 0, hi = nrec - 1;                      // record holding row r
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (recs[mid].row0 <= r) lo = mid; else hi = mid - 1; }
        const OutRec rc = recs[lo];
        const int k = r - rc.row0;
        const int sid = d.tsid[rc.w + k];
        const int L = rc.L;
        for (int x = threadIdx.x; x < L; x += blockDim.x) out_row[x] = '.';
        __syncthreads();
        // the lineage, child to root (the unfolded structure has parent -1 and no pairs).  The next ancestor's row is asked for before
        // this one's pairs are read: one dependent round trip per generation instead of two (a row of the benchmark set has 5-25)
        int s = sid, par = -1, np = 0;
        unsigned long long spo = 0;
        if (s >= 0) { par = d.st[s].parent; np = d.st[s].nsp; spo = d.st[s].sp; }
        while (s >= 0) {
            const int s2 = par;
            int par2 = -1, np2 = 0;
            unsigned long long spo2 = 0;
            if (s2 >= 0) { par2 = d.st[s2].parent; np2 = d.st[s2].nsp; spo2 = d.st[s2].sp; }
            const uint32_t *pl = d.sp + spo;
            for (int x = threadIdx.x; x < np; x += blockDim.x) { const uint32_t u = pl[x]; out_row[u & 0xFFFFu] = '('; out_row[u >> 16] = ')'; }
            s = s2; par = par2; np = np2; spo = spo2;
        }
        __syncthreads();
        char *o = out_db + rc.off + (long long)k * (L + 1);
        for (int x = threadIdx.x; x < L; x += blockDim.x) o[x] = (char)out_row[x];
        if (threadIdx.x == 0) { o[L] = 0; out_dcal[r] = d.st[sid].dcal; }
        __syncthreads();
    }
}

// ------------------------------------------------------------- eval kernel

// one wavefront per structure: sum of loop energies (rafft/utils.py:135-138)
__global__ __launch_bounds__(64) void eval_kernel(const EnergyTables *ET, int n, const uint8_t *codes, const int16_t *pts,
                                                  const long long *off, const int *len, int *out, int *status, int *guessed)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= n) return;
    const int L = len[s];
    const uint8_t *S = codes + off[s];
    PlainView pv{pts + off[s]};
    const SmallT *T = &ET->s;
    const BigT *B = &ET->b;
    int e = 0, bad = 0;
    if (lane == 0) e += loop_energy(T, B, S, L, pv, -1, L, &bad);
    for (int i = lane; i < L; i += 64) {
        int j = pv(i);
        if (j > i) e += loop_energy(T, B, S, L, pv, i, j, &bad);
    }
    for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o, 64); bad |= __shfl_xor(bad, o, 64); }
    if (lane == 0) { out[s] = e; status[s] = (bad & 1) ? 8 : 0; if (guessed) guessed[s] = (bad >> 1) & 1; }
}
