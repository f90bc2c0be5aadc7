// sinkhorn_state.h — the contract the entropic OT units meet at: the Sinkhorn state block, the workspace behind it, the
// row-strip rule of the column passes, the device-side convergence decision and the host iteration schedule.
//
// Included by sinkhorn.hip (the matrix solver; it defines the init / finish kernels and cfm_sk_ws_bytes_internal),
// sinkhorn_pts.hip (the point-cloud solver: same state, same workspace, same loop), sample.hip (reads u, v and vfinal of
// a solved workspace) and unbalanced.hip (the strip rule only).  A CFM_OP_SINKHORN workspace is
//     state block (SK_STATE_BYTES) | u [B0] | v[0] [B1] | v[1] [B1] | pm [nchunk][B1] | ps [nchunk][B1]      (fp64)
// and its first 48 bytes are read from outside the library as raw words (bench.py, tests/test_gpu_sinkhorn_paths.py):
// the static_asserts below hold that layout.
#pragma once
#include "cfm_common.h"

#define SK_NEG (-1.0e300)
#define SK_STATE_BYTES 256
#define SK_NCHUNK_MAX 64

struct SkState {
    int done;        // set once converged
    int iters_done;  // POT's ii+1 at break, or max_iter
    int vfinal;      // which v buffer holds the final v
    int precise;     // 1: fp64 exp/accumulate (near convergence)
    double err2[2];  // sum of squared marginal violations (ping-pong)
    double last_err;
};
static_assert(sizeof(SkState) <= SK_STATE_BYTES, "SkState must fit the bytes carved for it");
static_assert(offsetof(SkState, done) == 0 && offsetof(SkState, iters_done) == 4 && offsetof(SkState, vfinal) == 8 &&
              offsetof(SkState, precise) == 12, "done / iters_done / vfinal / precise are int words 0..3 for outside readers");
static_assert(offsetof(SkState, err2) == 16 && offsetof(SkState, last_err) == 32, "err2 at byte 16, last_err at byte 32");

struct SkWs {
    SkState* st;
    double* u;
    double* v[2];
    double* pm;  // [nchunk][B1]
    double* ps;  // [nchunk][B1]
};

// Row strips of a column pass over a B0 x B1 matrix (sk_col_pass, ub_coldot): one strip partial per column and strip.
static inline int sk_nchunk(int B0, int B1) {
    int tiles = (B1 + 255) / 256;
    int n = (1024 + tiles - 1) / tiles;  // aim for ~1024 workgroups
    if (n > SK_NCHUNK_MAX) n = SK_NCHUNK_MAX;
    int maxn = (B0 + 31) / 32;           // at least 32 rows per strip
    if (n > maxn) n = maxn;
    if (n < 1) n = 1;
    return n;
}

static inline size_t sk_ws_bytes(int B0, int B1) {
    size_t nchunk = sk_nchunk(B0, B1);
    return SK_STATE_BYTES + sizeof(double) * ((size_t)B0 + 2 * (size_t)B1 + 2 * nchunk * (size_t)B1) + 64;
}

static inline SkWs sk_carve(void* ws, int B0, int B1) {
    SkWs w;
    char* p = (char*)ws;
    w.st = (SkState*)p; p += SK_STATE_BYTES;
    w.u = (double*)p; p += sizeof(double) * (size_t)B0;
    w.v[0] = (double*)p; p += sizeof(double) * (size_t)B1;
    w.v[1] = (double*)p; p += sizeof(double) * (size_t)B1;
    size_t nchunk = sk_nchunk(B0, B1);
    w.pm = (double*)p; p += sizeof(double) * nchunk * (size_t)B1;
    w.ps = (double*)p;
    return w;
}

extern "C" size_t cfm_sk_ws_bytes_internal(int B0, int B1);      // sinkhorn.hip

// The kernels sk_init and sk_finish are defined once, in sinkhorn.hip, behind these launchers.
// sk_launch_init: u = v[0] = v[1] = 0 and the state block of a solve of max_iter iterations.
// sk_launch_finish: f = reg u, g = reg v[vfinal], iters_done, last_err (any of them may be null); with `pending` the
// error the last iteration's column pass left in err2[slot] is taken first.
void sk_launch_init(const SkWs& w, int B0, int B1, int max_iter, hipStream_t s);
void sk_launch_finish(const SkWs& w, int B0, int B1, double reg, float* f, float* g, int* iters_done, float* last_err,
                      int pending, int slot, hipStream_t s);

// The convergence decision for the previous iteration, at the head of a row update: every workgroup derives it from the
// same data, block 0 / thread 0 publishes it.  Returns whether the kernel goes on; `precise` is the regime it runs in.
// A kernel starts cold: call this AFTER the first loads have been requested, or the state block is a dependent hop in
// front of them.
__device__ __forceinline__ bool sk_decide(SkState* __restrict__ st, int check, int slot, double stop_thr, int ii,
                                          double precise_below, int& precise) {
    if (st->done) return false;
    if (check) {
        const double err = sqrt(st->err2[slot]);
        if (err < stop_thr) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                st->last_err = err;
                st->iters_done = ii;          // iterations 0..ii-1 ran; POT broke at ii-1
                st->vfinal = (ii - 1) & 1;
                __threadfence();
                st->done = 1;
            }
            return false;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->last_err = err;
            // fp32 exp leaves ~1e-7 relative noise per column sum -> ~1e-7/sqrt(B1) in the L2
            // violation; go precise well above that floor when the caller asks for less.
            if (!st->precise && err < precise_below && stop_thr < precise_below) st->precise = 1;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->err2[slot ^ 1] = 0.0;  // next accumulation slot
    precise = st->precise;
    return true;
}

// One solve in POT's order, enqueued on `s`: init, then per iteration ii the column half-step col(ii, check, slot) and
// the row half-step row(ii, check, slot), then finish.  v^(ii) -> v[ii & 1]; the error of iteration ii - 1 is measured
// by the column half-step of iteration ii (check, into err2[slot]) and decided at the start of its row half-step
// (sk_decide).  After the last iteration a trailing column half-step measures it when a check is due, and finish reads
// it (pending).  Short runs are enqueued in one go (no host sync); for very long caps (wasserstein() passes
// numItermax = 1e7) the host polls `done` every 512 iterations so the queue stays bounded.
// The half-steps are template parameters: the enqueue loop is on the critical path of a small solve.
template <class ColStep, class RowStep>
static inline int sk_solve(const SkWs& w, int B0, int B1, double reg, int max_iter, int check_every, float* f, float* g,
                           int* iters_done, float* last_err, hipStream_t s, ColStep col, RowStep row) {
    sk_launch_init(w, B0, B1, max_iter, s);
    const bool poll = max_iter > 4096;
    int host_done = 0;
    for (int ii = 0; ii <= max_iter; ++ii) {
        const int check = (ii >= 1) && (((ii - 1) % check_every) == 0);
        const int slot = ii & 1;
        const bool trailing = (ii == max_iter);
        if (trailing && !check) break;  // nothing left to measure
        col(ii, check, slot);
        if (trailing) break;
        row(ii, check, slot);
        if (poll && (ii & 511) == 511) {
            int rc = cfm_hip(hipMemcpyAsync(&host_done, &w.st->done, sizeof(int), hipMemcpyDeviceToHost, s));
            if (rc) return rc;
            rc = cfm_hip(hipStreamSynchronize(s));
            if (rc) return rc;
            if (host_done) break;
        }
    }
    const int pending = (max_iter >= 1) && (((max_iter - 1) % check_every) == 0);
    sk_launch_finish(w, B0, B1, reg, f, g, iters_done, last_err, pending, max_iter & 1, s);
    return cfm_status();
}
