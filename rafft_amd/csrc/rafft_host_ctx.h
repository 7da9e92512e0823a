// rafft_host_ctx.h - the process-wide state of the host library: error reporting, the workspaces and their device buffers, the
// global context, the device and pinned memory pools, and the initialisation of the device, a workspace and the energy tables.
// Part of the single translation unit of rafft_api.hip (included there, after the kernels).
#pragma once

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIPCHK(x)                                                                                      \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess)                                                                          \
            return fail(RAFFT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                 \
    } while (0)

struct Buf {
    void *p = nullptr;
    size_t cap = 0;
};
struct PinBuf { void *p = nullptr; size_t cap = 0; };

#define MAX_PIPES 4
// Every named device buffer of a workspace (grow-only), listed ONCE as X(name, matched).  matched = 0: Workspace::match() leaves
// the buffer alone - `dbg` and `big` are sized by the call that needs them (a seam's debug output, the lag scratch of the widest
// classes), not from the wave's plan.
#define WS_BUFFERS(X)                                                                                                           \
    X(codes, 1) X(seq_off, 1) X(seq_len, 1) X(beam, 1) X(beam_n, 1) X(done, 1) X(nsteps, 1) X(ch_parent, 1) X(ch_combo, 1)      \
    X(ch_dcal, 1) X(ch_h, 1) X(seen, 1) X(seen_off, 1) X(seen_cap, 1) X(seen_cnt, 1) X(seen_bm, 1) X(seen_mode, 1) X(st, 1) X(prod, 1) X(nd, 1) X(nlist, 1)   \
    X(nd_slot, 1) X(cslot, 1) X(pos, 1) X(br, 1) X(sp, 1) X(cand, 1) X(looptab, 1) X(trec, 1) X(tsid, 1) X(work0, 1)            \
    X(work1, 1) X(work2, 1) X(work3, 1) X(work4, 1) X(work5, 1) X(mat, 1) X(counters, 1) X(row_off, 1) X(out_db, 1)             \
    X(out_dcal, 1) X(row_off2, 1) X(out_db2, 1) X(out_dcal2, 1) X(dbg, 0) X(big, 0)
// One workspace = one folding pipeline: own stream set, grow-only device buffers and a pinned slot for the
// per-step read-back.  Even workspaces serve the long-tail lane of a batch, odd ones the bulk lane.
struct Workspace {
    bool ready = false;
    hipStream_t stream = nullptr;
    hipStream_t cls_stream[NCLS] = {};
    hipStream_t copy_stream = nullptr;   // result rows of sequences that finish early leave while the others still fold
    hipEvent_t ev_fork = nullptr, ev_join[NCLS] = {}, ev_hot = nullptr, ev_copy = nullptr;
    void *hot = nullptr;                 // pinned, 1 KiB: the read-back slot of the running step
    // named device buffers (grow-only)
#define X(name, matched) Buf name;
    WS_BUFFERS(X)
#undef X
    template <class F> static void for_each_buf(F f)      // f(pointer to the member, matched)
    {
#define X(name, matched) f(&Workspace::name, matched != 0);
        WS_BUFFERS(X)
#undef X
    }
    // every buffer of this workspace at least as big as its counterpart in `o` (defined after ensure())
    int match(const Workspace &o);
    void release_buffers()
    {
        for_each_buf([&](Buf Workspace::*m, bool) {
            Buf &b = this->*m;
            if (b.p) { hipError_t e_ = hipFree(b.p); (void)e_; b.p = nullptr; b.cap = 0; }
        });
    }
    size_t bytes() const
    {
        size_t t = 0;
        for_each_buf([&](Buf Workspace::*m, bool) { t += (this->*m).cap; });
        return t;
    }
};

struct Ctx {
    bool ready = false;
    int device = -1;
    int n_cu = 256;
    EnergyTables *T = nullptr;
    double T_temp = -1e300;            // temperature the device tables were scaled for
    bool T_dirty = true;               // the parameter set changed since the last upload
    rafft_par::ParamSet *P = nullptr;  // current parameter set (built-in until rafft_load_params)
    float2 *tw = nullptr;
    size_t hbm_total = 0;
    Workspace ws[MAX_PIPES];
    std::vector<PinBuf> pin_free;
    std::mutex pin_mu;                 // the pinned-chunk pool is used by the scheduler thread and by rafft_free_result
    std::vector<hipEvent_t> ev_free;   // timing events (scheduler thread only)
    std::vector<void *> garbage;       // device buffers replaced by bigger ones: freed when no wave is running (hipFree waits
    std::mutex gc_mu;                  //   for the whole device - tens of ms per regrown workspace while kernels are in flight)
    std::mutex ws_mu;                  // held by the seam calls that borrow workspace 0 on the caller's thread (vs idle trimming)
    rafft_stats stats{};               // of the batch that was waited for last
    std::mutex mu;                     // serialises the C-ABI entry points
    // ---- scheduler: one thread drives every wave of every batch in flight (rafft_sched.h)
    std::mutex qmu;
    std::condition_variable qcv_sched, qcv_done;
    std::deque<std::shared_ptr<struct Batch>> submitted;
    int n_inflight = 0;                // under qmu: batches submitted and not yet finished
    bool last_submit_async = false;    // under qmu: the last batch came through rafft_fold_submit (its caller may be about to queue more)
    std::chrono::steady_clock::time_point t_last_submit{};   // under qmu: when the last batch was queued (the scheduler lingers on a stream of them)
    Config proc_cfg;                   // read at rafft_init: the process-wide switches (rafft_config.h)
    Config sched_cfg;                  // read when the scheduler thread starts: its own settings
    bool sched_started = false;
    bool stop = false;                 // under qmu: the process is exiting (rafft_shutdown): the scheduler thread returns
    std::thread sched_thread;
};
// Never destroyed: the scheduler thread sleeps on its condition variable for as long as the process lives, and a
// condition variable must not be destroyed under a waiter (glibc's pthread_cond_destroy would block process exit).
Ctx &g = *new Ctx();

// allocations made so far: device buffers (calls, bytes, slowest call in ms) and pinned chunks (calls, bytes) - rafft_alloc_counters()
std::atomic<unsigned long long> g_dev_allocs{0}, g_dev_bytes{0}, g_dev_worst_us{0}, g_pin_allocs{0}, g_pin_bytes{0};

int ensure(Buf &b, size_t bytes, bool exact = false)
{
    if (bytes <= b.cap) return 0;
    const auto t0_ = std::chrono::steady_clock::now();
    const size_t old_cap = b.cap;
    if (b.p) { std::lock_guard<std::mutex> lk(g.gc_mu); g.garbage.push_back(b.p); b.p = nullptr; b.cap = 0; }
    // a buffer that had to grow once will grow again: leave room (at most 256 MB of it)
    size_t want = exact ? bytes : bytes + std::min<size_t>(bytes / (old_cap ? 2 : 8), (size_t)256 << 20) + 256;
    want = (want + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);      // whole 2 MiB fragments
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        // out of memory with replaced buffers still waiting for an idle moment to be freed: free them now (hipFree waits for the
        // device - a stall, not a failure) and ask again, for what is needed without the head-room
        (void)hipGetLastError();
        std::vector<void *> junk;
        { std::lock_guard<std::mutex> lk(g.gc_mu); junk.swap(g.garbage); }
        for (void *q : junk) { hipError_t e2 = hipFree(q); (void)e2; }
        want = (bytes + 256 + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        e = hipMalloc(&b.p, want);
    }
    {
        const unsigned long long us = (unsigned long long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0_).count();
        g_dev_allocs++; g_dev_bytes += want;
        unsigned long long w = g_dev_worst_us.load();
        while (us > w && !g_dev_worst_us.compare_exchange_weak(w, us)) { }
    }
    if (g.proc_cfg.trace_alloc) fprintf(stderr, "[rafft] ptr %p (mod 2MiB %zu KiB) ", b.p, ((size_t)(uintptr_t)b.p & (((size_t)2 << 20) - 1)) >> 10);
    if (g.proc_cfg.trace_alloc) fprintf(stderr, "[rafft] t=%.3f device buffer -> %.1f MB in %.3f ms\n", std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(), (double)want / 1e6, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count());
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(RAFFT_ERR_HIP, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
    }
    b.cap = want;
    return 0;
}

int Workspace::match(const Workspace &o)
{
    int rc = 0;
    for_each_buf([&](Buf Workspace::*m, bool matched) { if (matched && !rc) rc = ensure(this->*m, (o.*m).cap, true); });
    return rc;
}

rafft_par::ParamSet &param_set()
{
    if (!g.P) { g.P = new rafft_par::ParamSet(); rafft_par::builtin(*g.P); }
    return *g.P;
}

// Device energy tables for `temp`: the current parameter set rescaled as ViennaRNA does for md.temperature
// (rafft/utils.py:17-21).  Submission is asynchronous: the caller (submit_locked) drains the batches in flight first, so
// the device is idle when the tables are replaced.
int ensure_tables(double temp)
{
    if (!g.T_dirty && g.T_temp == temp) return 0;
    std::unique_ptr<EnergyTables> h(new EnergyTables());
    std::string err;
    if (!rafft_par::scaled_tables(param_set(), temp, h.get(), err)) return fail(RAFFT_ERR_TEMP, err);
    HIPCHK(hipMemcpy(g.T, h.get(), sizeof(EnergyTables), hipMemcpyHostToDevice));
    g.T_temp = temp; g.T_dirty = false;
    return 0;
}

int init_ws(Workspace &w)
{
    if (w.ready) return 0;
    // Stream priorities: streams of another priority have HW queues of their own, so the kernels of one wave do not
    // queue behind those of another.  The long-tail lane keeps workspace 0 and the bulk lane takes 1-3 (Scheduler::pick_workspace):
    // workspace 1 runs at high priority, 3 at low, 0 and 2 at normal.  (Measured with two waves: bulk high or low 13.4 ms,
    // no priorities 17.3 ms, the long tail high 15.4 ms.)
    int plo = 0, phi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&plo, &phi));
    const int idx = (int)(&w - g.ws);
    const int prio = idx == 1 ? phi : idx == 3 ? plo : 0;
    HIPCHK(hipStreamCreateWithPriority(&w.stream, hipStreamNonBlocking, prio));
    for (int c = 0; c < NCLS; c++) {
        HIPCHK(hipStreamCreateWithPriority(&w.cls_stream[c], hipStreamNonBlocking, prio));
        HIPCHK(hipEventCreateWithFlags(&w.ev_join[c], hipEventDisableTiming));
    }
    HIPCHK(hipStreamCreateWithFlags(&w.copy_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&w.ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&w.ev_copy, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&w.ev_hot, hipEventDisableTiming | hipEventBlockingSync));   // (the scheduler sleeps on it when it has spun long enough)
    static_assert(offsetof(Counters, node) <= 1024, "hot counters must fit the pinned read-back slot");
    HIPCHK(hipHostMalloc(&w.hot, 1024, hipHostMallocDefault));
    w.ready = true;
    return 0;
}

int init_ctx(int device)
{
    if (g.ready && (device < 0 || device == g.device)) {
        HIPCHK(hipSetDevice(g.device));    // HIP's current device is per host thread: bind it on every entry
        return 0;
    }
    g.proc_cfg = read_config();
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(RAFFT_ERR_NO_DEVICE, "no HIP device: libraffthip.so has no CPU fallback");
    if (device < 0) device = 0;
    if (device >= ndev) return fail(RAFFT_ERR_NO_DEVICE, "device ordinal out of range");
    if (g.ready) return fail(RAFFT_ERR_PARAM, "library already initialised on another device in this process");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    g.hbm_total = prop.totalGlobalMem;
    g.n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIPCHK(hipMalloc((void **)&g.T, sizeof(EnergyTables)));
    g.T_dirty = true;
    std::vector<float2> tw(MAX_P / 2);
    for (int m = 0; m < MAX_P / 2; m++) {
        double a = -2.0 * M_PI * (double)m / (double)MAX_P;
        tw[m] = make_float2((float)cos(a), (float)sin(a));
    }
    HIPCHK(hipMalloc((void **)&g.tw, sizeof(float2) * tw.size()));
    HIPCHK(hipMemcpy(g.tw, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice));
    g.device = device;
    g.ready = true;
    return init_ws(g.ws[0]);
}

static void free_garbage()
{
    std::vector<void *> junk;
    { std::lock_guard<std::mutex> lk(g.gc_mu); junk.swap(g.garbage); }
    for (void *p : junk) { hipError_t e_ = hipFree(p); (void)e_; }
}

// Pool of pinned host buffers, recycled across calls: hipHostMalloc / hipHostFree cost milliseconds for a result chunk
// of tens of MB and stall the queues while they run (measured: a steady stream of them turned 10 ms batches into
// 45-70 ms ones).  Sizes are rounded up to powers of two so that chunks of merged waves of different sizes reuse each
// other's buffers; the pool gives memory back only above 4 GB.
PinBuf pin_acquire(size_t bytes)
{
    std::lock_guard<std::mutex> lk(g.pin_mu);
    size_t want = 256 * 1024;
    while (want < bytes) want <<= 1;
    int best = -1;
    for (size_t i = 0; i < g.pin_free.size(); i++)
        if (g.pin_free[i].cap >= bytes && g.pin_free[i].cap <= 4 * want && (best < 0 || g.pin_free[i].cap < g.pin_free[best].cap)) best = (int)i;
    if (best >= 0) { PinBuf b = g.pin_free[best]; g.pin_free.erase(g.pin_free.begin() + best); return b; }
    PinBuf b;
    const auto t0_ = std::chrono::steady_clock::now();
    if (hipHostMalloc(&b.p, want, hipHostMallocDefault) != hipSuccess) { b.p = nullptr; return b; }
    g_pin_allocs++; g_pin_bytes += want;
    if (g.proc_cfg.trace_alloc) fprintf(stderr, "[rafft] t=%.3f pinned chunk %.1f MB in %.3f ms (pool %zu)\n", std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(), (double)want / 1e6, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count(), g.pin_free.size());
    b.cap = want;
    return b;
}
void pin_release(PinBuf b)
{
    if (!b.p) return;
    std::lock_guard<std::mutex> lk(g.pin_mu);
    size_t held = 0;
    for (auto &x : g.pin_free) held += x.cap;
    if (g.pin_free.size() < 64 && held + b.cap <= ((size_t)4 << 30)) g.pin_free.push_back(b);
    else {
        const auto t0_ = std::chrono::steady_clock::now();
        hipError_t e = hipHostFree(b.p); (void)e;
        if (g.proc_cfg.trace_alloc) fprintf(stderr, "[rafft] pinned chunk freed in %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count());
    }
}

// a pinned result chunk, returned to the pool when the last result that points into it is freed
struct PinChunk {
    PinBuf b;
    explicit PinChunk(PinBuf x) : b(x) {}
    ~PinChunk() { pin_release(b); }
    PinChunk(const PinChunk &) = delete;
    PinChunk &operator=(const PinChunk &) = delete;
};

} // namespace
