// assign_driver.h — the host driver of the exact assignment solver.  Included at the end of assign.hip (one
// translation unit: it launches that file's kernels); host code only.
// The kernels take only workspace-derived arguments, so the launch programs are captured once per
// host thread / workspace into hipGraphs and replayed (a solve is ~200 launches; with several
// couplings in flight on different streams the host launch rate would be the limit).  Falls back
// to plain launches when the stream cannot be captured (the legacy default stream) or CFM_ASG_GRAPH=0.
//   PRG_BULK   `bulk` x asg_step, or the whole solve in 9 / 11 launches (unpolled head of a solve)
//   PRG_CHUNK  `chunk` x asg_step, asg_build, asg_solve, 2 x asg_step   (polled; progresses from any state)
// Both are written once, in AsgLaunch::program.  asg_run is the solve: check, size, upload, programs, drive.
#pragma once

enum { PRG_CHUNK = 0, PRG_BULK = 1, PRG_COUNT = 2 };
struct AsgProblem { const float* M; int* perm; int* certified; double* total_cost; int* stats; };
#define ASG_BATCH_MAX 16
// The host polls the first 64 bytes of every problem's AsgState (asg_collect gathers 16 ints): these three words of it.
#define ASG_POLL_BYTES 64
#define ASG_POLL_INTS 16
enum { ASG_POLL_MODE = offsetof(AsgState, mode) / sizeof(int), ASG_POLL_ERROR = offsetof(AsgState, error) / sizeof(int),
       ASG_POLL_CERT = offsetof(AsgState, certified) / sizeof(int) };
static_assert(offsetof(AsgState, certified) + sizeof(int) <= ASG_POLL_BYTES, "the polled words lie in the polled block");
// pinned host memory: two slots (the chunk waited for, the look-ahead chunk) of ASG_BATCH_MAX polled blocks
#define ASG_PINNED_SLOT_INTS (ASG_BATCH_MAX * ASG_POLL_INTS)
// nb polled blocks -> cert_out[b] / err_out[b] (1 / 0 for a problem that is still open); returns the open problems
static int asg_read_polled(const int* hs, int nb, int* cert_out, int* err_out) {
    int open_ = 0;
    for (int b = 0; b < nb; ++b, hs += ASG_POLL_INTS) {
        cert_out[b] = 1; err_out[b] = 0;
        if (hs[ASG_POLL_ERROR]) err_out[b] = hs[ASG_POLL_ERROR];        // this problem stopped (its launches are no-ops now)
        else if (hs[ASG_POLL_MODE] == MODE_DONE) cert_out[b] = hs[ASG_POLL_CERT];
        else ++open_;
    }
    return open_;
}
// A batch workspace is nb carvings `stride` bytes apart, then the staging area asg_collect gathers the polled blocks
// into (two slots of nb blocks; room for the largest batch), then 256 spare bytes.
static inline size_t asg_batch_stride(int n) { return cfm_align_up(asg_ws_bytes(n), 256); }
static inline size_t asg_stage_offset(int nb, size_t stride) { return (size_t)nb * stride; }
#define ASG_STAGE_BYTES (2 * ASG_POLL_BYTES * (size_t)ASG_BATCH_MAX)
static inline int* asg_stage_slot(void* ws, int nb, size_t stride, int slot) {
    return reinterpret_cast<int*>((char*)ws + asg_stage_offset(nb, stride)) + ASG_POLL_INTS * nb * slot;
}
extern "C" size_t cfm_assign_batch_ws_bytes_internal(int n, int nb) {
    if (nb > ASG_BATCH_MAX) nb = ASG_BATCH_MAX;       // longer lists go through in groups of ASG_BATCH_MAX
    return asg_stage_offset(nb, asg_batch_stride(n)) + ASG_STAGE_BYTES + 256;
}
// What identifies a captured pair of programs: where it runs and every quantity its launches were captured with.
struct AsgProgramId {
    void* ws = nullptr; int n = 0, nb = 0; hipStream_t stream = nullptr;
    int chunk = 0, bulk = 0, blocks = 0, blocks_auction = 0, sparse = 0, async_auction = 0, sweep = 0;
    bool same_place(const AsgProgramId& o) const { return ws == o.ws && n == o.n && nb == o.nb && stream == o.stream; }
    bool operator==(const AsgProgramId& o) const {
        return same_place(o) && chunk == o.chunk && bulk == o.bulk && blocks == o.blocks && blocks_auction == o.blocks_auction && sparse == o.sparse && async_auction == o.async_auction && sweep == o.sweep;
    }
};
struct AsgGraph {
    AsgProgramId id;
    hipGraphExec_t exec[PRG_COUNT] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int ev_blocking = -1;          // how ev[] were created (this thread's blocking_sync at the time)
    unsigned use = 0;              // the thread's graph_clock when the slot was last taken
};
// A host thread keeps the programs of its last few (workspace, size, batch, stream) combinations: a training loop
// alternates between a few of them (groups of couplings and a shorter last group, single solves), and capturing +
// instantiating the two programs costs milliseconds.
#define ASG_GRAPH_SLOTS 4
static thread_local struct AsgThread {
    AsgGraph graphs[ASG_GRAPH_SLOTS];
    unsigned graph_clock = 0;
    int graph_off = 0;             // this thread's streams cannot be captured: plain launches from now on
    hipStream_t cap_stream = nullptr;       // the programs are captured here (asg_programs)
    // poll buffer (pinned host memory): one per host thread, concurrent solves on different streams must not share it
    int* pinned = nullptr;
    // The host wait of a solve (ONE per solve since round 5): with HIP's default an event wait SPINS on a host core; a
    // coupling worker of a training loop (cfm_amd.prefetch: 3 per rank, 8 ranks per node) burns a core each for the whole
    // solve.  cfm_set_blocking_sync(1) makes this THREAD's solver waits yield: its events carry hipEventBlockingSync AND the
    // wait itself is a poll (hipEventQuery) with a 20 us sleep in between — on this stack (ROCm 7, torch 2.10) a
    // "blocking" event wait was measured to spin exactly like the default (tools/probe/blocking_sync_probe.py: thread CPU
    // time == wall time for torch.cuda.Event(blocking=True) and for hipEventBlockingSync alike), so the flag alone buys
    // nothing.  The poll notices completion up to one sleep (~60 us with the kernel's timer slack) late — once per job of
    // several couplings, not per step.  Thread-local: a latency-critical lone solve on the caller's own thread keeps the spin.
    int blocking_sync = 0;
    int small_last[16] = {0};      // status block of this thread's last one-workgroup solve (phase times)
    struct { hipStream_t s; int dev, n; } cu_cache[4] = {};      // asg_stream_cus: the last few streams
    unsigned cu_clock = 0;
    int last_run[8] = {0};         // launch record of this thread's last chip-wide solve (cfm_assign_debug_sweep, mode -1)
} g_thr;
extern "C" void cfm_set_blocking_sync(int on) { g_thr.blocking_sync = on ? 1 : 0; }
static hipError_t asg_wait(hipEvent_t ev) {
    if (!g_thr.blocking_sync) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        (void)hipGetLastError();                  // (hipErrorNotReady is sticky in hipGetLastError otherwise)
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
    }
}
static hipError_t asg_events(AsgGraph& G) {
    if (G.ev_blocking != g_thr.blocking_sync) {
        for (int q = 0; q < 2; ++q) if (G.ev[q]) { (void)hipEventDestroy(G.ev[q]); G.ev[q] = nullptr; }
        G.ev_blocking = g_thr.blocking_sync;
    }
    const unsigned flags = hipEventDisableTiming | (g_thr.blocking_sync ? hipEventBlockingSync : 0u);
    for (int q = 0; q < 2; ++q)
        if (!G.ev[q]) { hipError_t e = hipEventCreateWithFlags(&G.ev[q], flags); if (e != hipSuccess) return e; }
    return hipSuccess;
}
// the slot that holds programs for this place, else the least recently used one
static AsgGraph& asg_graph_slot(const AsgProgramId& id) {
    AsgGraph* G = &g_thr.graphs[0];
    for (AsgGraph& Q : g_thr.graphs) {
        if (Q.exec[0] && Q.id.same_place(id)) { G = &Q; break; }
        if (Q.use < G->use) G = &Q;
    }
    G->use = ++g_thr.graph_clock;
    return *G;
}
static void asg_graph_drop(AsgGraph& G) {
    for (int q = 0; q < PRG_COUNT; ++q) if (G.exec[q]) { (void)hipGraphExecDestroy(G.exec[q]); G.exec[q] = nullptr; }
}
static int asg_pinned() {
    return g_thr.pinned ? 0 : cfm_hip(hipHostMalloc((void**)&g_thr.pinned, 2 * ASG_PINNED_SLOT_INTS * sizeof(int), hipHostMallocDefault));
}
// tuning aid: solves of this PROCESS that the dense state machine had to redo, and the last device error code — process-wide
// since round 6: the couplings of a training loop run on prefetch worker threads, and the bench line reports the count
static std::atomic<int> g_fallback_count{0}, g_fallback_error{0};
static void asg_fallback_error(int err) { g_fallback_error.store(err, std::memory_order_relaxed); }
extern "C" void cfm_assign_debug_fallback(int* out2) { out2[0] = g_fallback_count.load(); out2[1] = g_fallback_error.load(); }
extern "C" void cfm_assign_debug_small(int* out16) { for (int q = 0; q < 16; ++q) out16[q] = g_thr.small_last[q]; }
// Test hook: the candidate lists of the last solve on `ws` that built any (n <= SP_NMAX; problem b of a batch workspace,
// b = 0 for a single solve) — cl_out: n x SP_K {column, fp32 cost bits}, cT_out: n bounds, p_out: the n prices the build
// read.  Host buffers; blocking.  The caller tells a solve that never reached the build by clearing the workspace first.
extern "C" int cfm_assign_debug_lists(const void* ws, int n, int b, void* cl_out, double* cT_out, double* p_out) {
    if (!ws || n < 2 || n > SP_NMAX || b < 0 || b >= ASG_BATCH_MAX || !cl_out || !cT_out || !p_out) return CFM_EINVAL;
    const AsgWs w = asg_carve((char*)const_cast<void*>(ws) + (size_t)b * asg_batch_stride(n), n);
    int rc = cfm_hip(hipMemcpy(cl_out, w.cl, (size_t)n * SP_K * sizeof(uint2), hipMemcpyDeviceToHost));
    if (!rc) rc = cfm_hip(hipMemcpy(cT_out, w.cT, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (!rc) rc = cfm_hip(hipMemcpy(p_out, w.pb, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return rc;
}
// dynamic LDS above the 64 KiB default needs the attribute.  Bit 0: asg_step / asg_auction, bit 1: the list build + solver.
static int asg_raise_lds() {
    return cfm_once_per_device([] {
        hipError_t e1 = hipFuncSetAttribute((const void*)asg_step, hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024);
        if (e1 == hipSuccess) e1 = hipFuncSetAttribute((const void*)asg_auction, hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024);
        hipError_t e2 = hipFuncSetAttribute((const void*)asg_build, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
        hipError_t e3 = hipFuncSetAttribute((const void*)asg_solve, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        return (e1 == hipSuccess ? 1 : 0) | (e2 == hipSuccess && e3 == hipSuccess ? 2 : 0);
    });
}
// CUs the stream may use: the device's count, or the population of its CU mask (hipExtStreamCreateWithCUMask streams).
// Cached per host thread for its last few streams (the query is a host-side lookup, but it sits on every solve's path).
static int asg_stream_cus(hipStream_t s) {
    const int c = cfm_device_cus();
    if (!s) return c;
    const int di = cfm_device_index();
    for (auto& e : g_thr.cu_cache) if (e.s == s && e.dev == di && e.n > 0) return e.n;
    uint32_t mask[16] = {0}; int n = c;
    if (hipExtStreamGetCUMask(s, 16, mask) == hipSuccess) {
        int pop = 0;
        for (int q = 0; q < 16; ++q) pop += __builtin_popcount(mask[q]);
        if (pop > 0 && pop < n) n = pop;
    } else (void)hipGetLastError();
    auto& e = g_thr.cu_cache[g_thr.cu_clock++ & 3];
    e.s = s; e.dev = di; e.n = n;
    return n;
}

// The launch programs and everything they are sized by.
struct AsgLaunch {
    AsgWs w; int n, blocks, blocks_build, nb; size_t stride; size_t lds_step, lds_build, lds_solve; int sparse; hipStream_t s;
    int async_auction = 0, blocks_auction = 0;
    int chunk = 0, bulk = 0;       // asg_step launches of a polled chunk / of the unpolled head in the asg_step form (both even)
    int sweep = 0;                 // 1: the lean form of the head (asg_sweep)
    // the head holds the whole solve (see program)
    bool head_is_whole() const { return async_auction >= 2 && sparse && bulk > 0; }
    AsgProgramId id(void* ws) const { return {ws, n, nb, s, chunk, bulk, blocks, blocks_auction, sparse, async_auction, sweep}; }
    // asg_step launches of the head: the polled chunks go on from their parity
    int head_steps() const {
        if (bulk <= 0) return 0;
        if (!sweep) return head_is_whole() ? 8 : bulk;
        return head_is_whole() ? 1 : bulk - 2;
    }
    // Issues program `prg` on stream `s` (dry: issues nothing) and returns the number of its launches (kinds: of them
    // asg_step [0] and asg_sweep [1] launches).
    // The parity argument (which control record a bid round reads, see AucCtl) counts the asg_step launches of a solve:
    // launch k of them gets k & 1.  In the asg_step form every program holds an even number of them, so k is the position
    // inside the program; the lean head holds ONE (its CONVERT step), so the chunks behind it start on parity 1 — a chunk
    // holds an even number, every later chunk starts there too.  An asg_sweep launch takes no part in the count and gets
    // the parity of the asg_step launch in FRONT of it: the control step of INITRED leaves the first record of the bid
    // rounds in ctl[par ^ 1], where the next asg_step launch looks.
    // grid.y = the problems of a batch (one carving each, `stride` bytes apart)
    int program(int prg, bool dry = false, int* kinds = nullptr) const {
        int k = (prg == PRG_CHUNK) ? (head_steps() & 1) : 0, issued = 0, n_step = 0, n_sweep = 0;
        auto steps = [&](int cnt) {
            for (int c = 0; c < cnt; ++c, ++k, ++issued, ++n_step)
                if (!dry) hipLaunchKernelGGL(asg_step, dim3(blocks, nb), dim3(WT), lds_step, s, w, n, k & 1, stride);
        };
        // the plain matrix sweeps, when the program knows that the state is at one: the lean kernel on four times the
        // workgroups (the same number of waves); a no-op in any other mode
        auto sweeps = [&](int cnt) {
            for (int c = 0; c < cnt; ++c, ++issued, ++n_sweep)
                if (!dry) hipLaunchKernelGGL(asg_sweep, dim3(4 * blocks, nb), dim3(ASG_SWEEP_T), 0, s, w, n, (k & 1) ^ 1, stride);
        };
        // CONVERT (and whatever the state holds instead: any mode is served) is the work of ONE workgroup: nothing reads
        // the grid of that launch but the strides of the mode it runs and the arrival's group count, both from gridDim
        auto narrow_step = [&]() {
            if (!dry) hipLaunchKernelGGL(asg_step, dim3(1, nb), dim3(WT), lds_step, s, w, n, k & 1, stride);
            ++k; ++issued; ++n_step;
        };
        // asynchronous phase A: ONE launch behind the two init steps (a no-op in any other state, like every kernel here)
        auto auction = [&]() {
            if (async_auction && !dry) hipLaunchKernelGGL(asg_auction, dim3(blocks_auction, nb), dim3(WT), lds_step, s, w, n, stride);
            issued += async_auction ? 1 : 0;
        };
        auto list_pair = [&]() {
            if (!dry) hipLaunchKernelGGL(asg_build, dim3(blocks_build, nb), dim3(SP_BUILD_WAVES * 64), lds_build, s, w, n, stride);
            if (!dry) hipLaunchKernelGGL(asg_solve, dim3(1, nb), dim3(SP_T), lds_solve, s, w, n, stride);
            issued += 2;
        };
        if (prg == PRG_BULK && bulk <= 0) return 0;
        if (prg == PRG_BULK && head_is_whole()) {
            // The WHOLE solve as the unpolled head when the bid rounds (epsilon > 0 and epsilon = 0) are the one auction
            // launch and the list solver closes the search: 2 init steps, the auction, convert / row minima / column
            // reduction (+ one spare step: an even count), list build, list solver, certificate (+ one spare).  A solve
            // that takes this road — every C3 instance seen so far — is finished when the head is; the others are
            // picked up by the polled chunks.  (Round 4's head was 96 steps, then chunks of 10 steps + the pair + 2: a
            // lone solve paid ~35 no-op launches, 0.15 ms, around its list build and behind its last step.)
            // The lean form: UMIN0, INITRED as sweeps, the auction, CONVERT on one workgroup, UMIN, COLRED as sweeps, the
            // list pair, the certificate as a sweep — 9 launches, no spare ones (the parity contract: above).  A problem
            // that leaves this road (epsilon = 0 rounds left over, more free rows than the list solver takes) finds
            // no-ops or a one-workgroup step here and is picked up by the polled chunks, which are asg_step launches.
            if (sweep) { sweeps(2); auction(); narrow_step(); sweeps(2); list_pair(); sweeps(1); }
            else { steps(2); auction(); steps(4); list_pair(); steps(2); }
        } else if (prg == PRG_BULK) {
            if (sweep) sweeps(2); else steps(2);      // (bulk is even and > 0; a solve starts at UMIN0, INITRED)
            if (bulk > 2) { auction(); steps(bulk - 2); }
        } else {
            auction(); steps(chunk);
            if (sparse) { list_pair(); steps(2); }      // certificate + whatever the guess missed
        }
        if (kinds) { kinds[0] = n_step; kinds[1] = n_sweep; }
        return issued;
    }
    int count(int prg, int* kinds = nullptr) const { return program(prg, true, kinds); }
};

// Step 1: argument checks and the trivial sizes (B <= 1: nothing is left to do behind this).
static int asg_check(const AsgProblem* pr, int nb, int B, void* ws, size_t stride, hipStream_t s, int* cert_out, int* err_out) {
    if (!pr || nb < 1 || nb > ASG_BATCH_MAX || B < 0 || (B > 1 && !ws)) return CFM_EINVAL;
    for (int b = 0; b < nb; ++b) if (!pr[b].M || !pr[b].perm) return CFM_EINVAL;
    if (B > (1 << 20)) return CFM_EINVAL;
    for (int b = 0; b < nb; ++b) { cert_out[b] = 1; err_out[b] = 0; }
    if (B == 0) return 0;
    if (B == 1) {
        for (int b = 0; b < nb; ++b)
            hipLaunchKernelGGL(asg_trivial, dim3(1), dim3(64), 0, s, pr[b].M, B, pr[b].perm, pr[b].certified, pr[b].total_cost, pr[b].stats);
        return cfm_status();
    }
    if (((uintptr_t)ws & 15) != 0 || (stride & 15) != 0) return CFM_EALIGN;
    for (int b = 0; b < nb; ++b) if (((uintptr_t)pr[b].M & 15) != 0) return CFM_EALIGN;
    return 0;
}

// Step 2: the grids, the LDS budgets and the program lengths of a solve of nb problems of size n.
#define ASG_BATCH_WGS 256
#define ASG_BATCH_CHUNK 24
static int asg_size(AsgLaunch& L, int n, int nb, void* ws, size_t stride, hipStream_t s, const AsgParams& P, int use_sparse) {
    L.w = asg_carve(ws, n); L.n = n; L.s = s; L.nb = nb; L.stride = nb > 1 ? stride : 0;
    int wide_blocks = (n + 15) / 16;        // one wave per row when everything bids
    if (wide_blocks > 512) wide_blocks = 512;
    if (P.wide_blocks_cap > 0 && wide_blocks > P.wide_blocks_cap) wide_blocks = P.wide_blocks_cap;
    L.blocks_build = wide_blocks < (n + 63) / 64 ? (n + 63) / 64 : wide_blocks;     // the list build streams the matrix once: its own grid
    if (sp_build_fast(n)) {
        // its fast path runs four waves per SIMD = TWO workgroups per CU, each staging the prices once: two per CU over
        // the whole batch, between 8 rows (the grid the slow path takes) and 1 row per wave
        L.blocks_build = 2 * cfm_device_cus() / nb;
        if (L.blocks_build < n / (8 * SP_BUILD_WAVES)) L.blocks_build = n / (8 * SP_BUILD_WAVES);
        if (L.blocks_build > n / SP_BUILD_WAVES) L.blocks_build = n / SP_BUILD_WAVES;
    }
    // a batch shares the chip: ASG_BATCH_WGS workgroups in all (every workgroup of a bid round stages the prices whether
    // its rows bid or not; measured at n = 4096: 8 problems 9.1 ms with 256 workgroups each, 6.5 ms with 64); the rounds
    // then take the queue form (wide_bid_queue)
    const int floor_blocks = nb > 1 ? (n + ASG_BQ - 1) / ASG_BQ : (n + 63) / 64;
    if (nb > 1 && wide_blocks > ASG_BATCH_WGS / nb) wide_blocks = ASG_BATCH_WGS / nb;
    if (wide_blocks < floor_blocks) wide_blocks = floor_blocks;      // (the queue form takes ASG_BQ rows per workgroup)
    if (wide_blocks < 1) wide_blocks = 1;
    L.blocks = wide_blocks;
    const int raised = asg_raise_lds();
    L.lds_step = sizeof(double) * WT + 2 * sizeof(int) * WT;                      // relax merge buffers
    if (n <= WIDE_PLDS_MAX) {                                            // bid rounds: prices + owner rows
        const size_t need = (size_t)((n + 1) & ~1) * sizeof(double) + (size_t)(n + 2) * sizeof(int);
        if (need > L.lds_step) L.lds_step = need;
    }
    if (n <= 6144 && (size_t)2 * n * sizeof(int) > L.lds_step) L.lds_step = (size_t)2 * n * sizeof(int);   // path walks of MS_FINISH
    L.lds_step = (L.lds_step + 15) & ~(size_t)15;
    if (L.lds_step > 64 * 1024 && !(raised & 1)) return CFM_EINVAL;
    L.sparse = (use_sparse && n <= SP_NMAX && (raised & 2)) ? 1 : 0;
    L.lds_build = sp_build_lds_bytes(n); L.lds_solve = sp_solver_lds_bytes(n);
    // asynchronous phase A: the keys must fit the LDS snapshot and the grid must give every workgroup at most ASG_BQ rows
    L.blocks_auction = wide_blocks;
    if (nb > 1 && P.async_blocks > 0 && P.async_blocks < wide_blocks) L.blocks_auction = P.async_blocks;
    if ((long)L.blocks_auction * ASG_BQ < n) L.blocks_auction = (n + ASG_BQ - 1) / ASG_BQ;      // (a workgroup takes at most ASG_BQ rows)
    {   // its workgroups (16 waves, the whole register file of a CU each) must be able to be resident TOGETHER: a phase ends
        // when the whole grid has reported, and a workgroup that has not started counts as "all rows unmatched"
        // — on the CUs THIS STREAM may use: a CU-masked stream (cfm_stream_create_cu_mask, ChipPartition) gives the grid
        // fewer than the device has, and workgroups that cannot start before others exit would be counted as "all rows
        // unmatched" for the whole grace (~40 ms) and then left out: > 64 free rows, the dense fallback
        int c = asg_stream_cus(s);
        if ((long)L.blocks_auction * nb > c) L.blocks_auction = c / nb > 0 ? c / nb : 1;
    }
    L.async_auction = (P.async_auction && n >= P.async_min_n && n <= WIDE_PLDS_MAX && (raised & 1) && (long)L.blocks_auction * ASG_BQ >= n) ? P.async_auction : 0;

    L.chunk = ((P.chunk > 0 ? P.chunk : 10) + 1) & ~1;        // even: see AsgLaunch::program
    // A batch pays for every problem that is not yet at its list build when the first build + solver pair comes by: it
    // is built and solved by the NEXT chunk, behind the others' solver (~1.9 ms at n = 4096).  The steps before the
    // build vary by ~+-6 between problems: 24 instead of 10 steps in front of the pair (a no-op step costs 3-5 us).
    if (nb > 1 && L.chunk < ASG_BATCH_CHUNK) L.chunk = ASG_BATCH_CHUNK;
    // ... the unpolled head then is: 2 init steps, the auction launch, ~10 epsilon = 0 rounds + convert / row minima / column
    // reduction (the synchronous rounds needed ~96 launches here)
    L.bulk = ((n >= P.bulk_min_n) ? P.bulk : 0) & ~1;
    if (L.async_auction && L.bulk > 16) L.bulk = 16;
    L.sweep = asg_sweep_form(P, nb);
    return 0;
}
// AsgState::pad0 as asg_auction decodes it.  Bits 0-7: the last phase is cut at stop_frac / this (the low byte of
// async_last_div); bit 8: the epsilon = 0 rounds run inside the auction launch too (async mode 2); bits 16+: an
// experiment — grace of unstarted workgroups / 64 (the bits of async_last_div above its low byte).
static inline int asg_pack_pad0(const AsgParams& P) {
    return (P.async_last_div & 0xff) | ((P.async_auction >= 2 ? 1 : 0) << 8) | ((P.async_last_div >> 8) << 16);
}

// Step 3: every problem's state block, as the argument of one small launch each.
static int asg_upload(const AsgLaunch& L, const AsgProblem* pr, void* ws, const AsgParams& P) {
    const int n = L.n;
    for (int b = 0; b < L.nb; ++b) {
        AsgState h; memset(&h, 0, sizeof(h));
        h.wide_blocks = L.blocks;
        h.mode = MODE_UMIN0; h.n = n; h.Mptr = pr[b].M;
        h.out_perm = pr[b].perm; h.out_cert = pr[b].certified; h.out_cost = pr[b].total_cost; h.out_stats = pr[b].stats;
        h.eps = P.eps0_frac; h.eps_last = P.eps_last_frac; h.theta = L.async_auction ? P.async_theta : P.theta;
        h.stop_frac = P.stop_frac; h.round_cap = P.round_cap; h.arr_cap = P.arr_cap;
        h.cmin_bits = 0xffffffffu; h.cmax_bits = 0u; h.minslack_ord = ~0ull;
        h.fr_min = ~0ull; h.fr_max = 0ull;
        h.sparse = L.sparse; h.handoff = P.handoff; h.stop_early = P.stop_early;
        h.tag = 1; h.pad0 = asg_pack_pad0(P);
        { int rb = 1; while ((1 << rb) <= n) ++rb; h.rb = rb; }     // row ids 0 .. n-1 and the all-ones "none"
        hipLaunchKernelGGL(asg_init, dim3(1), dim3(64), 0, L.s, asg_carve((char*)ws + (size_t)b * L.stride, n), h);
    }
    return cfm_status();
}

// Step 4: the slot of this solve (its events are used either way), the programs of L captured into it unless it holds them;
// *use_graph = false: plain launches (CFM_ASG_GRAPH=0, n < 256, or capture failed on this thread once: sticky).
static AsgGraph& asg_programs(const AsgLaunch& L, void* ws, bool* use_graph) {
    const AsgProgramId id = L.id(ws);
    AsgGraph& G = asg_graph_slot(id);
    static const bool enabled = [] { const char* e = getenv("CFM_ASG_GRAPH"); return !(e && e[0] == '0'); }();
    *use_graph = enabled && !g_thr.graph_off && L.n >= 256;
    if (!*use_graph || (G.exec[0] && G.id == id)) return G;
    asg_graph_drop(G);
    hipError_t e = hipSuccess;
    // The programs are captured on a PRIVATE stream of this host thread, not on the caller's: while a stream captures,
    // HIP refuses any other stream's wait on an event that was recorded on it EARLIER (hipErrorStreamCaptureIsolation) —
    // a prefetch worker that starts a job of a new size while the training thread waits for the worker's previous job
    // (cfm_amd.prefetch: _Handle.result) raised exactly that, once in five runs of tests/test_gpu_prefetch.py.  The
    // kernels take workspace-derived arguments only, so where they are captured does not matter.
    if (!g_thr.cap_stream) e = hipStreamCreateWithFlags(&g_thr.cap_stream, hipStreamNonBlocking);
    AsgLaunch Lc = L; Lc.s = g_thr.cap_stream;
    for (int prg = 0; prg < PRG_COUNT && e == hipSuccess; ++prg) {
        if (L.count(prg) == 0) continue;
        hipGraph_t graph = nullptr;
        e = hipStreamBeginCapture(g_thr.cap_stream, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) break;
        Lc.program(prg);
        e = hipStreamEndCapture(g_thr.cap_stream, &graph);
        if (e == hipSuccess && graph) e = hipGraphInstantiate(&G.exec[prg], graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
    }
    if (e == hipSuccess) e = asg_events(G);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        asg_graph_drop(G);
        g_thr.graph_off = 1; *use_graph = false;     // e.g. the legacy default stream
    } else G.id = id;
    return G;
}

// Step 5: run the programs until every problem is done or stopped.
// The head goes out unpolled (a solve at n = 4096 takes ~100 steps before the list solver); the rest
// in chunks that make progress from any state, each followed by a copy of the first 64 bytes of every
// problem's state into its own pinned slot and an event, with the NEXT chunk already queued when the host
// waits for a slot: no idle gap.  A kernel that does not own the current mode is a ~2 us no-op.
static int asg_drive(const AsgLaunch& L, AsgGraph& G, bool use_graph, void* ws, long max_launches, int* cert_out, int* err_out) {
    const int nb = L.nb; hipStream_t s = L.s;
    long launched = 0;
    int* rec = g_thr.last_run;      // {launches, of them asg_step, asg_sweep, chunks run, launches of the head, of a chunk, form, 0}
    for (int q = 0; q < 8; ++q) rec[q] = 0;
    rec[4] = L.count(PRG_BULK); rec[5] = L.count(PRG_CHUNK); rec[6] = L.sweep;
    auto run = [&](int prg) -> int {
        int kinds[2] = {0, 0};
        const int cnt = L.count(prg, kinds);
        launched += cnt;
        rec[0] += cnt; rec[1] += kinds[0]; rec[2] += kinds[1]; rec[3] += (prg == PRG_CHUNK);
        if (cnt == 0) return 0;
        if (use_graph) return cfm_hip(hipGraphLaunch(G.exec[prg], s));
        L.program(prg); return cfm_status();
    };
    auto pinned_slot = [&](int slot) { return g_thr.pinned + ASG_PINNED_SLOT_INTS * slot; };
    // the polled blocks of every problem into pinned slot `slot` (batches: gathered in the staging area first), then the event
    auto issue = [&](int slot, bool with_chunk = true) -> int {
        int r2 = with_chunk ? run(PRG_CHUNK) : 0; if (r2) return r2;
        if (nb == 1) r2 = cfm_hip(hipMemcpyAsync(pinned_slot(slot), L.w.st, ASG_POLL_BYTES, hipMemcpyDeviceToHost, s));
        else {
            int* stage = asg_stage_slot(ws, nb, L.stride, slot);
            hipLaunchKernelGGL(asg_collect, dim3(1), dim3(16 * ASG_BATCH_MAX), 0, s, L.w.st, L.stride, nb, stage);
            r2 = cfm_status();
            if (!r2) r2 = cfm_hip(hipMemcpyAsync(pinned_slot(slot), stage, ASG_POLL_BYTES * (size_t)nb, hipMemcpyDeviceToHost, s));
        }
        if (r2) return r2;
        return cfm_hip(hipEventRecord(G.ev[slot], s));
    };
    int rc = run(PRG_BULK); if (rc) return rc;
    // the head holds the whole solve (see AsgLaunch::program): look at the state behind it BEFORE queueing anything else —
    // a finished solve returns here, with no look-ahead chunk of no-ops to wait for
    if (L.head_is_whole()) {
        rc = issue(0, false); if (rc) return rc;
        rc = cfm_hip(asg_wait(G.ev[0])); if (rc) return rc;
        if (!asg_read_polled(pinned_slot(0), nb, cert_out, err_out)) return 0;      // (else: re-read by the chunk loop)
    }
    rc = issue(0); if (rc) return rc;
    int cur = 0, result = 0;
    for (;;) {
        rc = issue(cur ^ 1); if (rc) return rc;
        rc = cfm_hip(asg_wait(G.ev[cur])); if (rc) return rc;
        if (!asg_read_polled(pinned_slot(cur), nb, cert_out, err_out)) break;
        if (launched >= max_launches) { result = CFM_ETIMEOUT; break; }
        cur ^= 1;
    }
    // the look-ahead chunk is still in flight: it is a string of no-ops on a finished state, but the
    // workspace (and the pinned slot it copies into) must not be reused under it
    rc = cfm_hip(asg_wait(G.ev[cur ^ 1]));
    return rc ? rc : result;
}

// Solves nb problems of the same size on one chain of launches (grid.y = problem).  cert_out[b] / err_out[b]: the
// certificate and the device error code of problem b (0 = none).  nb == 1: the plain solve.
static int asg_run(const AsgProblem* pr, int nb, int B, void* ws, size_t stride, void* stream, const AsgParams& P,
                   int use_sparse, int* cert_out, int* err_out) {
    hipStream_t s = (hipStream_t)stream;
    int rc = asg_check(pr, nb, B, ws, stride, s, cert_out, err_out); if (rc || B <= 1) return rc;
    rc = asg_pinned(); if (rc) return rc;
    AsgLaunch L;
    rc = asg_size(L, B, nb, ws, stride, s, P, use_sparse); if (rc) return rc;
    rc = asg_upload(L, pr, ws, P); if (rc) return rc;
    bool use_graph = false;
    AsgGraph& G = asg_programs(L, ws, &use_graph);
    rc = cfm_hip(asg_events(G)); if (rc) return rc;      // (also: the thread's blocking-sync choice changed since they were made)
    return asg_drive(L, G, use_graph, ws, P.max_launches, cert_out, err_out);
}
// one problem through the candidate-list machine, the dense state machine deciding should its certificate ever fail
static int asg_solve_one(const AsgProblem& pr, int B, void* ws, void* stream, const AsgParams& P, int first_sparse) {
    int cert = 1, err = 0;
    int rc = asg_run(&pr, 1, B, ws, 0, stream, P, first_sparse, &cert, &err);
    if (rc) return rc;
    if (err) { asg_fallback_error(err); rc = CFM_ENOCONV; }
    if (first_sparse && B > 1 && B <= SP_NMAX && (rc == CFM_ENOCONV || !cert)) {
        g_fallback_count.fetch_add(1, std::memory_order_relaxed);
        if (rc == 0) asg_fallback_error(-1);          // uncertified
        rc = asg_run(&pr, 1, B, ws, 0, stream, P, 0, &cert, &err);
        if (rc == 0 && err) { asg_fallback_error(err); rc = CFM_ENOCONV; }
    }
    if (rc == 0 && B > 1 && !cert) rc = CFM_ENOCONV;     // never hand back an uncertified permutation silently
    return rc;
}
// The one-workgroup solver (assign_small.h): one workgroup, one launch; a solve that hits its round caps or fails its
// certificate reports it and the chip-wide state machine takes over
static bool asg_takes_small(const AsgParams& P, int B) { return P.small && B >= 2 && B <= SMA_N; }
static int asg_solve_small(const AsgProblem& pr, int B, void* ws, void* stream, const AsgParams& P) {
    if (!ws) return CFM_EINVAL;
    if (((uintptr_t)ws & 15) != 0) return CFM_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int rc = asg_pinned(); if (rc) return rc;
    SmaParams Q;
    Q.theta = P.async_theta;            // (its epsilon phases are asynchronous since round 6: theta 2-3 measured 10 % ahead of 5, tools/asg_small_sweep.py)
    Q.eps0_frac = P.eps0_frac; Q.eps_last_frac = P.eps_last_frac;
    Q.stop_frac = P.stop_frac;
    Q.round_cap = P.round_cap; Q.arr_cap = P.arr_cap > 15 ? P.arr_cap : 15; Q.total_cap = 20000;   // (the one-workgroup solver was tuned with 15)
    Q.reserved = 0;
    int* status = (int*)ws;            // (the kernel clears `certified` and writes every word of the status block itself)
    hipLaunchKernelGGL(asg_small, dim3(1), dim3(SMA_T), 0, s, pr.M, B, Q, pr.perm, pr.certified, pr.total_cost, pr.stats, status);
    rc = cfm_status(); if (rc) return rc;
    rc = cfm_hip(hipMemcpyAsync(g_thr.pinned, status, 64, hipMemcpyDeviceToHost, s)); if (rc) return rc;
    rc = cfm_hip(hipStreamSynchronize(s)); if (rc) return rc;
    for (int q = 0; q < 16; ++q) g_thr.small_last[q] = g_thr.pinned[q];
    return g_thr.pinned[0] == 1 ? 0 : asg_solve_one(pr, B, ws, stream, P, P.sparse);
}
static int asg_solve_any(const AsgProblem& pr, int B, void* ws, void* stream, const AsgParams& P) {
    return asg_takes_small(P, B) ? asg_solve_small(pr, B, ws, stream, P) : asg_solve_one(pr, B, ws, stream, P, P.sparse);
}
extern "C" int cfm_assign_exact_f32(const float* M, int B, int* perm, int* certified,
                                    double* total_cost, int* stats, void* ws, void* stream) {
    if (!M || !perm) return CFM_EINVAL;
    const AsgProblem pr = {M, perm, certified, total_cost, stats};
    return asg_solve_any(pr, B, ws, stream, asg_params_snapshot());
}

// nb problems of the same size in ONE chain of launches: every launch carries all problems (grid.y), so the
// latency-bound chain — ~110 launch boundaries, a one-workgroup list solver — is paid once per batch.  A problem
// whose candidate-list path stops or ends uncertified is redone alone on the dense state machine, like a single solve.
extern "C" int cfm_assign_exact_batch_f32(const float* const* M, int nb, int B, int* const* perm, int* certified,
                                          double* total_cost, int* stats, void* ws, void* stream) {
    if (!M || !perm || nb < 0) return CFM_EINVAL;
    if (nb == 0) return 0;
    AsgParams P = asg_params_snapshot();
    // The batch entry is the THROUGHPUT form of the solve (couplings prefetched beside a model step): its launches are
    // capped at ASG_TP_WGS workgroups per problem whatever the batch size — also for a batch of one, two or three
    // (the first, small job of a prefetch run; the remainder of a run).  A bid round occupies the chip for as long as
    // its slowest workgroup whatever it does, and every workgroup stages the prices: fewer, fuller workgroups take
    // less of the chip from the other jobs and the dense products.  Measured in the C3 pipelined loop (round 4,
    // CFM_ASG_BLOCKS sweep, same box): 256 / 64 / 32 / 16 per problem for the odd-sized jobs: 1.201 / 1.163 / 1.162 /
    // 1.276 ms per step; a lone solve prefers the wide grid (3.30 vs 3.68 ms sequential): cfm_assign_exact_f32 keeps it.
#define ASG_TP_WGS 64
    if (P.wide_blocks_cap == 0) P.wide_blocks_cap = ASG_TP_WGS;      // (an explicit cfm_assign_set_wide_blocks cap is the caller's: never overridden)
    const size_t stride = asg_batch_stride(B);
    int rc = 0;
    for (int b0 = 0; b0 < nb && rc == 0; b0 += ASG_BATCH_MAX) {
        const int k = nb - b0 < ASG_BATCH_MAX ? nb - b0 : ASG_BATCH_MAX;
        AsgProblem pr[ASG_BATCH_MAX];
        int cert[ASG_BATCH_MAX], err[ASG_BATCH_MAX];
        for (int b = 0; b < k; ++b) {
            if (!M[b0 + b] || !perm[b0 + b]) return CFM_EINVAL;
            pr[b] = {M[b0 + b], perm[b0 + b], certified ? certified + b0 + b : nullptr,
                     total_cost ? total_cost + b0 + b : nullptr, stats ? stats + 8 * (size_t)(b0 + b) : nullptr};
        }
        if (asg_takes_small(P, B) || B <= 1 || k == 1) {      // single problems and the one-workgroup sizes: one after the other
            for (int b = 0; b < k && rc == 0; ++b) rc = asg_solve_any(pr[b], B, ws, stream, P);      // (else: the chip-wide machine on the throughput grid)
            continue;
        }
        rc = asg_run(pr, k, B, ws, stride, stream, P, P.sparse, cert, err);
        for (int b = 0; b < k && rc == 0; ++b) {
            if (!err[b] && cert[b]) continue;
            if (!(P.sparse && B <= SP_NMAX)) { rc = CFM_ENOCONV; break; }
            g_fallback_count.fetch_add(1, std::memory_order_relaxed);
            asg_fallback_error(err[b] ? err[b] : -1);
            rc = asg_solve_one(pr[b], B, (char*)ws + (size_t)b * stride, stream, P, 0);
        }
    }
    return rc;
}

// Test hook (tuning export): ONE sweep step of the chip-wide machine on a caller-made state, with the kernel
// cfm_assign_set_sweep selects (0: asg_step on `blocks` workgroups, 1: asg_sweep on 4 x blocks, unset: as a batch would;
// blocks <= 0: the grid of a lone solve of this size).  mode: MODE_UMIN0 / INITRED / UMIN / COLRED / ROOTMIN / CERT.  M and ws (cfm_workspace_bytes of
// the exact solver) are device pointers, everything else host memory; blocking.
//   in:  p_in [n] prices / duals (UMIN, COLRED, ROOTMIN, CERT), bidval_in [n] row minima (INITRED, COLRED), list [n_list]
//        the free columns (COLRED) or free rows (ROOTMIN), perm_in [n] row -> column (CERT)
//   out: bidval_out / key_out / p_out [n] as the step left them — every array the step may write is filled with a
//        sentinel first (all-ones bytes: NaN / ~0; the keys of INITRED start at 0 as UMIN0 leaves them), so an element a
//        grid skips shows; state_out [8]: {cmin bits, cmax bits, mode after the step, certified, minslack bits (2 words),
//        control steps booked, 0}; cost_out: the certificate's total cost
// mode = -1: no launch — state_out receives the launch record of this thread's last chip-wide solve: {launches, of them
// asg_step, asg_sweep, polled chunks run, launches of the head program, of a chunk program, form (0 / 1), 0}.
extern "C" int cfm_assign_debug_sweep(int mode, const float* M, int n, int blocks, const double* p_in, const double* bidval_in,
                                      const int* list, int n_list, const int* perm_in, double* bidval_out,
                                      unsigned long long* key_out, double* p_out, int* state_out, double* cost_out,
                                      void* ws, void* stream) {
    if (mode == -1) { if (!state_out) return CFM_EINVAL; for (int q = 0; q < 8; ++q) state_out[q] = g_thr.last_run[q]; return 0; }
    const bool known = mode == MODE_UMIN0 || mode == MODE_INITRED || mode == MODE_UMIN || mode == MODE_COLRED || mode == MODE_ROOTMIN || mode == MODE_CERT;
    if (!known || !M || !ws || n < 2 || n > (1 << 20) || !state_out || n_list < 0 || n_list > n) return CFM_EINVAL;
    if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)M & 15) != 0) return CFM_EALIGN;
    const bool need_p = mode != MODE_UMIN0 && mode != MODE_INITRED, need_u = mode == MODE_INITRED || mode == MODE_COLRED;
    const bool need_list = mode == MODE_COLRED || mode == MODE_ROOTMIN;
    if ((need_p && !p_in) || (need_u && !bidval_in) || (need_list && !list) || (mode == MODE_CERT && !perm_in)) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const AsgParams P = asg_params_snapshot();
    AsgLaunch L;
    int rc = asg_size(L, n, 1, ws, 0, s, P, P.sparse); if (rc) return rc;
    if (blocks > 0) L.blocks = blocks > 512 ? 512 : blocks;
    const AsgWs& w = L.w;
    const size_t N = (size_t)n;
    // sentinels, then the caller's state
    rc = cfm_hip(hipMemsetAsync(ws, 0xff, asg_ws_bytes(n), s)); if (rc) return rc;
    const AsgProblem pr = {M, w.listA, nullptr, nullptr, nullptr};      // (the certificate's step exports the permutation: into scratch)
    rc = asg_upload(L, &pr, ws, P); if (rc) return rc;                    // (also clears the arrival words)
    rc = cfm_hip(hipMemsetAsync(w.auc, 0, 512, s)); if (rc) return rc;
    auto put = [&](void* dst, const void* src, size_t bytes) { return cfm_hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)); };
    if (mode == MODE_INITRED) { rc = cfm_hip(hipMemsetAsync(w.key, 0, 8 * N, s)); if (rc) return rc; }
    if (need_p) { rc = put(w.p, p_in, 8 * N); if (rc) return rc; }
    if (need_u) { rc = put(w.bidval, bidval_in, 8 * N); if (rc) return rc; }
    if (need_list) { rc = put(mode == MODE_COLRED ? w.listFC : w.listF, list, 4 * (size_t)n_list); if (rc) return rc; }
    std::vector<int> owner;
    if (mode == MODE_CERT) {
        owner.assign(N, -1);
        for (size_t i = 0; i < N; ++i) if (perm_in[i] >= 0 && perm_in[i] < n) owner[perm_in[i]] = (int)i;
        rc = put(w.a, perm_in, 4 * N); if (rc) return rc;
        rc = put(w.owner, owner.data(), 4 * N); if (rc) return rc;
    }
    // the words of the state block the step reads beside what asg_upload set
    AsgState h;
    rc = cfm_hip(hipMemcpyAsync(&h, w.st, sizeof(h), hipMemcpyDeviceToHost, s)); if (rc) return rc;
    rc = cfm_hip(hipStreamSynchronize(s)); if (rc) return rc;
    h.mode = mode; h.nF = mode == MODE_ROOTMIN ? n_list : 0; h.nFC = mode == MODE_COLRED ? n_list : 0; h.cur = 0;
    h.cert_bad = 0; h.total_cost = 0.0; h.minslack_ord = ~0ull;
    rc = put(w.st, &h, sizeof(h)); if (rc) return rc;
    if (asg_sweep_form(P, 2)) hipLaunchKernelGGL(asg_sweep, dim3(4 * L.blocks, 1), dim3(ASG_SWEEP_T), 0, s, w, n, 1, (size_t)0);
    else hipLaunchKernelGGL(asg_step, dim3(L.blocks, 1), dim3(WT), L.lds_step, s, w, n, 1, (size_t)0);
    rc = cfm_status(); if (rc) return rc;
    rc = cfm_hip(hipStreamSynchronize(s)); if (rc) return rc;
    rc = cfm_hip(hipMemcpy(&h, w.st, sizeof(h), hipMemcpyDeviceToHost)); if (rc) return rc;
    if (bidval_out) { rc = cfm_hip(hipMemcpy(bidval_out, w.bidval, 8 * N, hipMemcpyDeviceToHost)); if (rc) return rc; }
    if (key_out) { rc = cfm_hip(hipMemcpy(key_out, w.key, 8 * N, hipMemcpyDeviceToHost)); if (rc) return rc; }
    if (p_out) { rc = cfm_hip(hipMemcpy(p_out, w.p, 8 * N, hipMemcpyDeviceToHost)); if (rc) return rc; }
    state_out[0] = (int)h.cmin_bits; state_out[1] = (int)h.cmax_bits; state_out[2] = h.mode; state_out[3] = h.certified;
    state_out[4] = (int)(h.minslack_ord & 0xffffffffull); state_out[5] = (int)(h.minslack_ord >> 32);
    state_out[6] = h.st_steps; state_out[7] = 0;
    if (cost_out) *cost_out = h.total_cost;
    return 0;
}
