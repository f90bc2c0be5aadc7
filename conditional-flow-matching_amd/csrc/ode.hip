// ode.hip — K11: ODE solve of dx/dt = MLP([x, t]) (torchdyn-style drivers).
//
// Replaces NeuralODE(torch_wrapper(model), solver="euler"|"dopri5").trajectory
// (torchdyn is third-party and absent from the reference tree; the algorithm
// restated here is the one written down in SURVEY.md Appendix A.4 and mirrored,
// line for line, by oracle/cfm_oracle.py::dopri5_trajectory — "torchdyn-style
// dopri5", parity unpinned by the reference itself).
//
//  euler, midpoint, rk4 : fixed steps on t_span (explicit tableaus of 1, 2 and 4 stages; rk4 is the 3/8 rule,
//           "torchdyn-style rk4", unpinned like dopri5), fully asynchronous (no host sync).
//  tsit5  : Tsitouras 5(4): the same driver as dopri5 with another tableau (7 stages, FSAL, last row of a = b).
//  dopri5 : Dormand-Prince 5(4), FSAL, one global RMS error norm over the batch
//           (hairer_norm over all B*d elements), every t_span point is a step
//           end.  Stage combinations and the scaled error norm are fused
//           elementwise kernels; the scalar step controller runs on the host in
//           fp32 (one 8-byte read-back per step attempt).
//
// In dependency order, nothing declared ahead of its definition: elementwise kernels and the workspace, the tile
// kernels, their launch helpers, the host drivers, the C entries.
#include "cfm_common.h"
#include "small_field.h"
#include "grad_field.h"
#include "ode_tableau.h"
#include "ode_envelope.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>

int cfm_mlp_forward_impl(const float* x, const float* t, float tval, int has_t, int t_per_row,
                         const float* const* W, const float* const* b, const int* dims,
                         int n_layers, int B, float* out, void* ws, hipStream_t s);
extern "C" size_t cfm_mlp_ws_bytes_internal(int B, int width);

struct Stages { const float* k[7]; float c[7]; int n; };

// out = x + dt * sum_s c[s] * k[s]
__global__ __launch_bounds__(256) void ode_combine(size_t n, const float* __restrict__ x, float dt,
                                                   Stages st, float* __restrict__ out,
                                                   float* __restrict__ out2) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float acc = st.c[0] * st.k[0][i];
#pragma unroll
        for (int s = 1; s < 7; ++s)
            if (s < st.n) acc = fmaf(st.c[s], st.k[s][i], acc);
        const float v = fmaf(dt, acc, x[i]);
        out[i] = v;
        if (out2) out2[i] = v;
    }
}

// sum over elements of ( dt*sum_s e[s]k[s] / (atol + rtol*max(|x|,|xn|)) )^2
__global__ __launch_bounds__(256) void ode_error(size_t n, const float* __restrict__ x,
                                                 const float* __restrict__ xn, float dt, Stages st,
                                                 float atol, float rtol, double* __restrict__ out) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float e = st.c[0] * st.k[0][i];
#pragma unroll
        for (int s = 1; s < 7; ++s)
            if (s < st.n) e = fmaf(st.c[s], st.k[s][i], e);
        e *= dt;
        const float sc = atol + rtol * fmaxf(fabsf(x[i]), fabsf(xn[i]));
        const float r = e / sc;
        acc += (double)r * (double)r;
    }
    acc = wave_sum_d(acc);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// sum of ((a - b) / (atol + rtol*|x0|))^2   (b may be NULL)
__global__ __launch_bounds__(256) void ode_sqnorm(size_t n, const float* __restrict__ a,
                                                  const float* __restrict__ b,
                                                  const float* __restrict__ x0, float atol,
                                                  float rtol, double* __restrict__ out) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float num = b ? a[i] - b[i] : a[i];
        const float r = num / (atol + rtol * fabsf(x0[i]));
        acc += (double)r * (double)r;
    }
    acc = wave_sum_d(acc);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// adapt_step(dt, ratio, safety=0.9, min_factor=0.2, max_factor=10, order=5): the factor of the next step size
__device__ __forceinline__ float ode_step_factor(float ratio) {
    float factor;
    if (ratio == 0.f) factor = 10.f;
    else {
        const float minf = ratio < 1.f ? 1.f : 0.2f;
        factor = fminf(10.f, fmaxf(0.9f / powf(ratio, 1.f / 5.f), minf));
    }
    return factor;
}

// The controller's scalars of the layer-per-kernel driver, taken where the fused kernel takes them (one lane): the
// device's powf and the host's differ in the last bit on some inputs, and a step size must not depend on the path.
// out[0] = error ratio (RMS over n elements), out[1] = step factor.
__global__ void ode_controller(const double* __restrict__ e2, double n, float* __restrict__ out) {
    const float ratio = (float)sqrt(e2[0] / n);
    out[0] = ratio;
    out[1] = ode_step_factor(ratio);
}

// k <- 0.5f * (k - kb): the stage derivative of the pair from the two nets' outputs (layer driver)
__global__ __launch_bounds__(256) void ode_half_diff(size_t n, float* __restrict__ k, const float* __restrict__ kb) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) k[i] = 0.5f * (k[i] - kb[i]);
}

static inline int ode_blocks(size_t n) {
    size_t b = (n + 255) / 256;
    return (int)(b < 2048 ? (b ? b : 1) : 2048);
}

// rendezvous area of the persistent small-field solver: 3 rows of SM_MAXGRID fp64 partial-sum slots
#define SM_MAXGRID 1024
#define ODE_SYNC_BYTES (3 * SM_MAXGRID * 8 + 128 + 1792)   // tail: profiling stamps (SM_PROF builds)
extern "C" size_t cfm_ode_ws_bytes_internal(int B, int width, int d) {
    return cfm_mlp_ws_bytes_internal(B, width) + sizeof(float) * (size_t)B * d * 10 + 512 + ODE_SYNC_BYTES;
}

struct OdeWs {
    float* act;       // MLP activations
    float* k[7];
    float* x; float* xn; float* xt;
    double* red;      // 32 doubles
    char* sync;       // ODE_SYNC_BYTES
};

static OdeWs ode_carve(void* ws, int B, int width, int d) {
    OdeWs w; char* q = (char*)ws;
    w.red = (double*)q; q += 256;
    w.sync = q; q += ODE_SYNC_BYTES;
    w.act = (float*)q; q += cfm_align_up(cfm_mlp_ws_bytes_internal(B, width), 256) - 256 + 256;
    const size_t n = (size_t)B * d;
    for (int s = 0; s < 7; ++s) { w.k[s] = (float*)q; q += sizeof(float) * n; }
    w.x = (float*)q; q += sizeof(float) * n;
    w.xn = (float*)q; q += sizeof(float) * n;
    w.xt = (float*)q;
    return w;
}

static int maxwidth(const int* dims, int n_layers) {
    int m = 1;
    for (int l = 1; l < n_layers; ++l) m = dims[l] > m ? dims[l] : m;
    return m;
}

static int check_mlp(const int* dims, int n_layers, int* d_out) {
    if (!dims || n_layers < 1) return CFM_EINVAL;
    const int d = dims[n_layers];
    if (dims[0] != d + 1) return CFM_EINVAL;   // time-varying vector field: [x, t] -> dx
    *d_out = d;
    return 0;
}

// The fused-path switch.  -1: not read yet (CFM_ODE_FUSED=0 in the environment disables), else 0 / 1.  Entries run on
// several host threads at once: relaxed accesses, and the first readers all derive the same value from the environment.
static std::atomic<int> g_ode_fused{-1};
extern "C" void cfm_ode_set_fused(int on) { g_ode_fused.store(on ? 1 : 0, std::memory_order_relaxed); }
extern "C" int cfm_ode_fused_internal() {       // not exported: small_grad.hip's entries read the switch through it
    int v = g_ode_fused.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* e = getenv("CFM_ODE_FUSED");
        const int env = (e && e[0] == '0') ? 0 : 1;
        if (g_ode_fused.compare_exchange_strong(v, env, std::memory_order_relaxed)) v = env;   // (else v: what a setter stored)
    }
    return v;
}

// ---- tile kernels: a whole solve (adaptive, fixed-step, pair) or one evaluation of [v, div] in one launch ------------
// OdeStepRec (ode_envelope.h): the record of an accepted step that the recording solve keeps
struct OdeRec { OdeStepRec* log; float* ysteps; int max_steps; };   // log [max_steps], ysteps [max_steps, B, d]: device

struct SmState { float t, dt; int ckpt, steps, evals, par, done, pad; };
// One persistent solve at a time per process, whatever its augmentation mode (see ode_dopri5_small)
static std::mutex g_persistent_mu;

// the step-size clipping the host loop does before every attempt
__device__ __forceinline__ void sm_prestep(const SmState& st, const float* __restrict__ tspan, int n_t,
                                           float& dt, float& dt_old, bool& flag, bool& lands) {
    const float T = tspan[n_t - 1];
    dt = st.dt;
    if (st.t + dt > T) dt = T - st.t;
    dt_old = dt; flag = false;
    if (st.ckpt < n_t && st.t + dt > tspan[st.ckpt]) { dt_old = dt; flag = true; dt = tspan[st.ckpt] - st.t; }
    lands = (st.ckpt < n_t) && (flag || st.t + dt == tspan[st.ckpt]);
}

// Grid-wide rendezvous + all-reduce of a persistent launch (grid <= workgroups that are resident at
// once).  There is no arrival counter: the fp64 partial sum a workgroup publishes IS its arrival.  Slots
// hold a negative NaN until their owner stores its (non-negative) partial; wave 0 of every workgroup polls
// all slots (L2 reads of distinct words, no same-address atomics to serialise) and, once none is NaN, has
// the values in hand: it adds them in a fixed order, so the total is the same bit pattern in every
// workgroup and in every run.  Three slot rows rotate (attempt % 3): at the start of attempt a the owner
// re-arms its slot of row (a + 1) % 3, which held attempt a - 2 (everybody finished reading that before
// publishing a - 1, which the owner saw at rendezvous a - 1), and its release store of attempt a orders
// the re-arm before anything a reader of attempt a + 1 can see.  Measured on MI355X, 256 workgroups:
// an arrival counter + polling cost 7-9 us per rendezvous, a two-level counter tree 15 us.
// The wait is bounded (wall clock, ~4 s): a mis-sized launch turns into an error code, never a hung GPU.
__device__ __forceinline__ bool sm_grid_allsum(double* __restrict__ row, double mine, int lane, int wv, double* sh_total,
                                               int* sh_ok) {
    if (wv == 0) {
        if (lane == 0) __hip_atomic_store(&row[blockIdx.x], mine, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        int ok = 1;
        unsigned spins = 0;
        unsigned long long t0 = 0;
        double tsum;
        for (;;) {
            tsum = 0.0;
            bool all = true;
            for (int i = lane; i < (int)gridDim.x; i += 64) {
                const double v = __hip_atomic_load(&row[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                all = all && (v >= 0.0);
                tsum += v;
            }
            if (__all(all)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 1023u) == 0) {                  // the clock read is slow: look at it rarely
                const unsigned long long now = wall_clock64();
                if (!t0) t0 = now;
                else if (now - t0 > 400000000ull) { ok = 0; break; }
            }
        }
        tsum = wave_sum_d(tsum);
        if (lane == 0) { *sh_total = tsum; *sh_ok = ok; }
    }
    sm_lds_barrier();
    return *sh_ok != 0;
}

// The whole adaptive integration in ONE persistent launch.  A workgroup owns the row tiles
// blockIdx.x, blockIdx.x + gridDim.x, ... for the entire solve.  RESIDENT (one tile per workgroup, B <=
// 32 x resident workgroups = 8192 on MI355X): x and k1 live in registers from the first attempt to the
// last, an accepted step is a register move, and the only global traffic of an attempt is the trajectory
// row it lands on.  Otherwise x / k1 travel between a workgroup and its own rows of the (L2-resident)
// parity buffers.  The only cross-workgroup value of a step attempt is the squared error norm: every
// workgroup stores its fp64 partial, one grid rendezvous, and then every workgroup adds the partials up in
// the same fixed order (so the solve is reproducible bit for bit), derives the same accept / reject
// decision and next step size from that sum (the fp32 controller of the host loop above).  `lines` is only
// touched by SM_PROF builds (phase stamps).  FIELD: what the stage evaluations call (FIELD_GRAD: grad_field.h, plain
// solves only); everything around the call is the same code.
// REC (plain MLP field): every accepted step n leaves the state it started from in R.ysteps[n] (each workgroup its own rows)
// and its record in R.log[n] (workgroup 0, lane 0); the accepted count nacc and the FSAL time tk1 are functions of the
// replicated SmState history, so every workgroup holds the same values.  A full log (nacc == R.max_steps before done) ends
// the loop in every workgroup at the same attempt, before its re-arm and rendezvous, as max_attempts does: err = 3.
template <int TAB, bool RESIDENT, int MODE, int FIELD = FIELD_MLP, bool REC = false>
__global__ __launch_bounds__(256) void ode_small_dopri(SmArgs A, int B, int d, SmState* __restrict__ st_io,
                                                    float* __restrict__ xbuf, float* __restrict__ kbuf,
                                                    const float* __restrict__ tspan, int n_t, float atol, float rtol,
                                                    float* __restrict__ traj, double* __restrict__ partial,
                                                    unsigned long long* __restrict__ lines, int max_attempts,
                                                    float tsign, const float* __restrict__ eps, OdeRec R) {
    static_assert(!REC || (MODE == AUG_NONE && FIELD == FIELD_MLP), "the plain MLP field records its steps");
    // MODE != AUG_NONE: the state is [B, 1 + d] (column 0 = l, the log-density accumulator, d l / dt = -div); each
    // row's l and its stage values sit in the registers of every lane that holds the row
    constexpr bool AUG = MODE != AUG_NONE;
    static_assert(FIELD == FIELD_MLP || !AUG, "the gradient field has fixed-step augmented solves only");
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* Wl = small_lds;                           // [4][64][SM_LD]
    float* bl = Wl + 4 * SM_W * SM_LD;               // [4][64]
    float* wt = bl + 4 * SM_W;                       // [64] time column of layer 0
    float* Ab0 = wt + SM_W;                          // [SM_ROWS][SM_LD]
    float* Ab1 = Ab0 + SM_ROWS * SM_LD;
    float* red = Ab1 + SM_ROWS * SM_LD;              // AUG: [4][SM_ROWS] row sums
    __shared__ double redw[4];
    __shared__ double sh_total;
    __shared__ int sh_ok;
    SmState st = st_io[0];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    sm_stage_weights(A, d, Wl, bl, wt, tid);
    const int D = AUG ? d + 1 : d;                   // row stride of the state, trajectory and stage buffers
    const int c0 = AUG ? 1 : 0;                      // column of x[.., 0]
    const size_t n = (size_t)B * D;
    const int col = wv * 16 + (lane & 15);
    const bool lw = wv == 0 && (lane & 15) == 0;     // AUG: the lanes that store / count a row's l
    const float T = tspan[n_t - 1];
    SmTile x, k0, k1, k2, k3, k4, k5, k6, y;
    SmTile xl, l0, l1, l2, l3, l4, l5, l6, yl, ep;   // AUG: l, its stage derivatives (-div), the probe tile
    if (RESIDENT) {
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = blockIdx.x * SM_ROWS + sm_row(i, lane);
            const bool ok = gr < B && col < d;
            x.v[i] = ok ? xbuf[(size_t)gr * D + c0 + col] : 0.f;
            k0.v[i] = ok ? kbuf[(size_t)gr * D + c0 + col] : 0.f;
            if constexpr (AUG) {
                xl.v[i] = gr < B ? xbuf[(size_t)gr * D] : 0.f;
                l0.v[i] = gr < B ? kbuf[(size_t)gr * D] : 0.f;
                ep.v[i] = (MODE == AUG_HUTCH && ok) ? eps[(size_t)gr * d + col] : 0.f;
            }
        }
    }
    __syncthreads();                                  // weights staged
    int attempt = 0, err = 0;
    int nacc = 0;                                     // REC: accepted steps so far
    float tk1 = st.t;                                 // REC: the time k_1 of the next accepted step was evaluated at
    for (; !st.done; ++attempt) {
        if (attempt >= max_attempts) { err = 1; break; }
        if (REC && nacc >= R.max_steps) { err = 3; break; }
        if (tid == 0)                                 // re-arm this workgroup's slot of the next attempt
            __hip_atomic_store(&partial[(size_t)((attempt + 1) % 3) * SM_MAXGRID + blockIdx.x], __longlong_as_double(-1ll),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        float dt, dt_old; bool flag, lands;
        sm_prestep(st, tspan, n_t, dt, dt_old, flag, lands);
        const float hdt = tsign * dt;                 // stage coefficient sign (reverse time: g = -f(-s, y))
        const float* x_in = xbuf + (size_t)st.par * n;
        const float* k1_in = kbuf + (size_t)st.par * n;
        float* x_out = xbuf + (size_t)(st.par ^ 1) * n;
        float* k7_out = kbuf + (size_t)(st.par ^ 1) * n;
        double esum = 0.0;
        for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
            if (!RESIDENT) {
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const int gr = row0 + sm_row(i, lane);
                    const bool ok = gr < B && col < d;
                    x.v[i] = ok ? x_in[(size_t)gr * D + c0 + col] : 0.f;
                    k0.v[i] = ok ? k1_in[(size_t)gr * D + c0 + col] : 0.f;
                    if constexpr (AUG) {
                        xl.v[i] = gr < B ? x_in[(size_t)gr * D] : 0.f;
                        l0.v[i] = gr < B ? k1_in[(size_t)gr * D] : 0.f;
                        ep.v[i] = (MODE == AUG_HUTCH && ok) ? eps[(size_t)gr * d + col] : 0.f;
                    }
                }
                sm_lds_barrier();                     // previous tile done with the activation buffers
            }
            // stage S (a literal): y = x + dt * sum_{q<=S} a[S][q] k_q ; KOUT = f(t + c[S] dt, y)
#define SM_COMBINE(S, Y, X, K0, K1, K2, K3, K4, K5)                                                  \
            _Pragma("unroll") for (int i = 0; i < SM_V; ++i) {                                       \
                float acc = (float)rk_a<TAB>(S, 0) * K0.v[i];                                         \
                if (S >= 1) acc = fmaf((float)rk_a<TAB>(S, 1), K1.v[i], acc);                         \
                if (S >= 2) acc = fmaf((float)rk_a<TAB>(S, 2), K2.v[i], acc);                         \
                if (S >= 3) acc = fmaf((float)rk_a<TAB>(S, 3), K3.v[i], acc);                         \
                if (S >= 4) acc = fmaf((float)rk_a<TAB>(S, 4), K4.v[i], acc);                         \
                if (S >= 5) acc = fmaf((float)rk_a<TAB>(S, 5), K5.v[i], acc);                         \
                Y.v[i] = fmaf(hdt, acc, X.v[i]);                                                     \
            }
#define SM_STAGE(S, KOUT, LOUT)                                                                      \
            {                                                                                        \
                SM_COMBINE(S, y, x, k0, k1, k2, k3, k4, k5)                                          \
                const float tf = tsign * (st.t + rk_c<TAB>(S) * dt);                                  \
                if constexpr (AUG) {                                                                 \
                    SM_COMBINE(S, yl, xl, l0, l1, l2, l3, l4, l5)                                    \
                    SmTile dv;                                                                       \
                    KOUT = sm_field_aug<MODE>(y, tf, A, d, Ab0, Ab1, Wl, bl, wt, ep, B - row0, red, wv, lane, dv); \
                    _Pragma("unroll") for (int i = 0; i < SM_V; ++i) LOUT.v[i] = -dv.v[i];         \
                } else if constexpr (FIELD == FIELD_GRAD) {                                          \
                    SmTile dv;                                                                       \
                    KOUT = gf_field<false>(y, tf, A, d, Ab0, Ab1, Wl, bl, wt, B - row0, red, wv, lane, dv); \
                } else {                                                                             \
                    KOUT = sm_field(y, tf, A, d, Ab0, Ab1, Wl, bl, wt, wv, lane);                    \
                }                                                                                    \
            }
            SM_STAGE(0, k1, l1) SM_STAGE(1, k2, l2) SM_STAGE(2, k3, l3) SM_STAGE(3, k4, l4) SM_STAGE(4, k5, l5)
            SM_STAGE(5, k6, l6)
#undef SM_STAGE
#undef SM_COMBINE
            // y is x_new (the 5th-order solution), k6 = f(t + dt, x_new): error + outputs
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const int gr = row0 + sm_row(i, lane);
                if (gr < B && col < d) {
                    float e = (float)rk_e<TAB>(0) * k0.v[i];
                    e = fmaf((float)rk_e<TAB>(1), k1.v[i], e);
                    e = fmaf((float)rk_e<TAB>(2), k2.v[i], e);
                    e = fmaf((float)rk_e<TAB>(3), k3.v[i], e);
                    e = fmaf((float)rk_e<TAB>(4), k4.v[i], e);
                    e = fmaf((float)rk_e<TAB>(5), k5.v[i], e);
                    e = fmaf((float)rk_e<TAB>(6), k6.v[i], e);
                    e *= dt;
                    const float sc = atol + rtol * fmaxf(fabsf(x.v[i]), fabsf(y.v[i]));
                    const float rr = e / sc;
                    esum += (double)rr * (double)rr;
                    if (!RESIDENT) {
                        x_out[(size_t)gr * D + c0 + col] = y.v[i];
                        k7_out[(size_t)gr * D + c0 + col] = k6.v[i];
                    }
                }
                if constexpr (AUG) {
                    if (gr < B && lw) {               // each row's l counts once in the norm
                        float e = (float)rk_e<TAB>(0) * l0.v[i];
                        e = fmaf((float)rk_e<TAB>(1), l1.v[i], e);
                        e = fmaf((float)rk_e<TAB>(2), l2.v[i], e);
                        e = fmaf((float)rk_e<TAB>(3), l3.v[i], e);
                        e = fmaf((float)rk_e<TAB>(4), l4.v[i], e);
                        e = fmaf((float)rk_e<TAB>(5), l5.v[i], e);
                        e = fmaf((float)rk_e<TAB>(6), l6.v[i], e);
                        e *= dt;
                        const float sc = atol + rtol * fmaxf(fabsf(xl.v[i]), fabsf(yl.v[i]));
                        const float rr = e / sc;
                        esum += (double)rr * (double)rr;
                        if (!RESIDENT) {
                            x_out[(size_t)gr * D] = yl.v[i];
                            k7_out[(size_t)gr * D] = l6.v[i];
                        }
                    }
                }
            }
        }
        esum = wave_sum_d(esum);
        if (lane == 0) redw[wv] = esum;
        if (RESIDENT) sm_lds_barrier(); else __syncthreads();   // (the streamed path re-reads its rows below)
        if (!sm_grid_allsum(partial + (size_t)(attempt % 3) * SM_MAXGRID, redw[0] + redw[1] + redw[2] + redw[3], lane, wv,
                            &sh_total, &sh_ok)) { err = 2; break; }
        // accept / reject, next step size (identical in every workgroup and lane)
        const float ratio = (float)sqrt(sh_total / (double)n);
        const bool accept = ratio <= 1.f;
        if (RESIDENT) {
            if (accept) {
                if (lands) {
                    float* dst = traj + (size_t)st.ckpt * n;
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        const int gr = blockIdx.x * SM_ROWS + sm_row(i, lane);
                        if (gr < B && col < d) dst[(size_t)gr * D + c0 + col] = y.v[i];
                        if constexpr (AUG) {
                            if (gr < B && lw) dst[(size_t)gr * D] = yl.v[i];
                        }
                    }
                }
                if constexpr (REC) {
                    float* ys = R.ysteps + (size_t)nacc * n;
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        const int gr = blockIdx.x * SM_ROWS + sm_row(i, lane);
                        if (gr < B && col < d) ys[(size_t)gr * D + col] = x.v[i];
                    }
                }
                x = y; k0 = k6;                       // FSAL
                if constexpr (AUG) { xl = yl; l0 = l6; }
            }
        } else if (accept && lands) {
            const float* xn = xbuf + (size_t)(st.par ^ 1) * n;
            float* dst = traj + (size_t)st.ckpt * n;
            for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
                const int rows = (B - row0 < SM_ROWS) ? B - row0 : SM_ROWS;
                const size_t base = (size_t)row0 * D;
                for (int e = tid; e < rows * D; e += 256) dst[base + e] = xn[base + e];   // own rows, written above
            }
        }
        if constexpr (REC && !RESIDENT) {
            if (accept) {
                float* ys = R.ysteps + (size_t)nacc * n;
                for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
                    const int rows = (B - row0 < SM_ROWS) ? B - row0 : SM_ROWS;
                    const size_t base = (size_t)row0 * D;
                    for (int e = tid; e < rows * D; e += 256) ys[base + e] = x_in[base + e];   // own rows
                }
            }
        }
        if constexpr (REC) {
            if (accept) {
                if (blockIdx.x == 0 && tid == 0) R.log[nacc] = OdeStepRec{st.t, dt, tk1, lands ? st.ckpt : -1};
                tk1 = st.t + rk_c<TAB>(5) * dt;       // the stage time of k_7, the next accepted step's k_1
                ++nacc;
            }
        }
        SmState nx = st;
        nx.steps = st.steps + 1; nx.evals = st.evals + 6;
        if (accept) {
            nx.t = lands ? tspan[st.ckpt] : st.t + dt;
            if (lands) nx.ckpt = st.ckpt + 1;
            nx.par = st.par ^ 1;
        }
        float ndt = dt;
        if (flag) ndt = dt_old - dt;
        ndt = ndt * ode_step_factor(ratio);
        if (!(ndt > 1e-12f)) ndt = 1e-12f;
        nx.dt = ndt;
        nx.done = (nx.t < T) ? 0 : 1;
        st = nx;
    }
    if (blockIdx.x == 0 && tid == 0) {
        st.pad = err; st_io[1] = st;
        if constexpr (REC) { SmState cnt = st; cnt.steps = nacc; st_io[2] = cnt; }
    }
}

#include "sde_small.h"

// Fixed-step explicit Runge-Kutta (euler / midpoint / rk4: fx_stages<SCHEME>() = 1, 2 or 4 stages) for the same small
// fields: every step of the tile inside one launch, the stage tiles in registers.  Same arithmetic as the layer driver's
// ode_combine calls: stage y = fmaf(dt, a0 k0 (+ fma chain), x), x_{k+1} = fmaf(dt, b0 k0 (+ fma chain), x_k); for
// euler that is fmaf(dt, 1.f * k, x).  A decreasing t_span needs nothing else: dt < 0 steps it, bit for bit the forward
// solve of -f(-s, x) on s = -t_span.  MODE != AUG_NONE: the trajectory is [n_t, B, 1 + d] with column 0 = l, whose
// stage derivatives are -div f at the stage points (the field does not read l, so l has no stage states); the x columns
// are bitwise those of the plain solve.  FIELD_GRAD: the field is grad_field.h's; AUG_EXACT carries its Laplacian.
template <int SCHEME, int MODE, int FIELD = FIELD_MLP>
__global__ __launch_bounds__(256) void ode_small_fixed(SmArgs A, int B, int d, const float* __restrict__ tspan, int n_t,
                                                    float* __restrict__ traj, const float* __restrict__ eps) {
    constexpr bool AUG = MODE != AUG_NONE;
    constexpr int NS = fx_stages<SCHEME>();
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* Wl = small_lds;
    float* bl = Wl + 4 * SM_W * SM_LD;
    float* wt = bl + 4 * SM_W;
    float* Ab0 = wt + SM_W;
    float* Ab1 = Ab0 + SM_ROWS * SM_LD;
    float* red = Ab1 + SM_ROWS * SM_LD;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    sm_stage_weights(A, d, Wl, bl, wt, tid);
    const int D = AUG ? d + 1 : d;
    const int c0 = AUG ? 1 : 0;
    const size_t n = (size_t)B * D;
    const int col = wv * 16 + (lane & 15);
    const bool lw = wv == 0 && (lane & 15) == 0;
    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        SmTile x, xl, ep;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            x.v[i] = (gr < B && col < d) ? traj[(size_t)gr * D + c0 + col] : 0.f;
            if constexpr (AUG) {
                xl.v[i] = gr < B ? traj[(size_t)gr * D] : 0.f;
                ep.v[i] = (MODE == AUG_HUTCH && gr < B && col < d) ? eps[(size_t)gr * d + col] : 0.f;
            }
        }
        __syncthreads();
        for (int k = 0; k + 1 < n_t; ++k) {
            const float t = tspan[k], dt = tspan[k + 1] - tspan[k];
            SmTile f[NS], lf[NS];
#pragma unroll
            for (int sg = 0; sg < NS; ++sg) {
                SmTile y = x;
                float tsg = t;
                if (sg > 0) {
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        float acc = (float)fx_a<SCHEME>(sg - 1, 0) * f[0].v[i];
#pragma unroll
                        for (int q = 1; q < NS - 1; ++q)
                            if (q < sg) acc = fmaf((float)fx_a<SCHEME>(sg - 1, q), f[q].v[i], acc);
                        y.v[i] = fmaf(dt, acc, x.v[i]);
                    }
                    tsg = t + (float)fx_c<SCHEME>(sg - 1) * dt;
                }
                if constexpr (FIELD == FIELD_GRAD) {
                    static_assert(FIELD == FIELD_MLP || MODE != AUG_HUTCH, "exact trace only");
                    SmTile dv;
                    f[sg] = gf_field<AUG>(y, tsg, A, d, Ab0, Ab1, Wl, bl, wt, B - row0, red, wv, lane, dv);
                    if constexpr (AUG) {
#pragma unroll
                        for (int i = 0; i < SM_V; ++i) lf[sg].v[i] = -dv.v[i];
                    }
                } else if constexpr (AUG) {
                    SmTile dv;
                    f[sg] = sm_field_aug<MODE>(y, tsg, A, d, Ab0, Ab1, Wl, bl, wt, ep, B - row0, red, wv, lane, dv);
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) lf[sg].v[i] = -dv.v[i];
                } else {
                    f[sg] = sm_field(y, tsg, A, d, Ab0, Ab1, Wl, bl, wt, wv, lane);
                }
            }
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                float acc = (float)fx_b<SCHEME>(0) * f[0].v[i];
#pragma unroll
                for (int q = 1; q < NS; ++q) acc = fmaf((float)fx_b<SCHEME>(q), f[q].v[i], acc);
                x.v[i] = fmaf(dt, acc, x.v[i]);
                const int gr = row0 + sm_row(i, lane);
                if (gr < B && col < d) traj[(size_t)(k + 1) * n + (size_t)gr * D + c0 + col] = x.v[i];
                if constexpr (AUG) {
                    float lacc = (float)fx_b<SCHEME>(0) * lf[0].v[i];
#pragma unroll
                    for (int q = 1; q < NS; ++q) lacc = fmaf((float)fx_b<SCHEME>(q), lf[q].v[i], lacc);
                    xl.v[i] = fmaf(dt, lacc, xl.v[i]);
                    if (gr < B && lw) traj[(size_t)(k + 1) * n + (size_t)gr * D] = xl.v[i];
                }
            }
        }
    }
}

// ---- DSBM: the probability-flow ODE of a forward and a backward drift net, dx/dt = (f(t, x) - b(t, x)) / 2 ----------
// runner/src/models/components/solver.py:259-263 (DSBMFlowSolver.forward_ode_drift).  ode_small_fixed with two fields: both
// nets' weights in LDS in the layout of the SDE kernels (sde_small.h: small_lds_bytes(2, 2, false)), every stage derivative
// k = 0.5f * (f - b) — one rounded subtraction and an exact halving, so `/ 2` and `* 0.5f` agree — and the stage and step
// arithmetic of ode_small_fixed.  Bit-equal to the layer driver below (two forward passes on mlp_layer, ode_half_diff,
// ode_combine).
template <int SCHEME>
__global__ __launch_bounds__(256) void ode_small_fixed_pair(SmArgs F, SmArgs S, int B, int d, const float* __restrict__ tspan,
                                                            int n_t, float* __restrict__ traj) {
    constexpr int NS = fx_stages<SCHEME>();
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* WlF = small_lds;
    float* blF = WlF + 4 * SM_W * SM_LD;
    float* wtF = blF + 4 * SM_W;
    float* WlS = wtF + SM_W;
    float* blS = WlS + 4 * SM_W * SM_LD;
    float* wtS = blS + 4 * SM_W;
    float* Ab0 = wtS + SM_W;
    float* Ab1 = Ab0 + SM_ROWS * SM_LD;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    sm_stage_weights(F, d, WlF, blF, wtF, tid);
    sm_stage_weights(S, d, WlS, blS, wtS, tid);
    const size_t n = (size_t)B * d;
    const int col = wv * 16 + (lane & 15);
    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        SmTile x;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            x.v[i] = (gr < B && col < d) ? traj[(size_t)gr * d + col] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k + 1 < n_t; ++k) {
            const float t = tspan[k], dt = tspan[k + 1] - tspan[k];
            SmTile f[NS];
#pragma unroll
            for (int sg = 0; sg < NS; ++sg) {
                SmTile y = x;
                float tsg = t;
                if (sg > 0) {
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        float acc = (float)fx_a<SCHEME>(sg - 1, 0) * f[0].v[i];
#pragma unroll
                        for (int q = 1; q < NS - 1; ++q)
                            if (q < sg) acc = fmaf((float)fx_a<SCHEME>(sg - 1, q), f[q].v[i], acc);
                        y.v[i] = fmaf(dt, acc, x.v[i]);
                    }
                    tsg = t + (float)fx_c<SCHEME>(sg - 1) * dt;
                }
                const SmTile fv = sm_field(y, tsg, F, d, Ab0, Ab1, WlF, blF, wtF, wv, lane);
                const SmTile bv = sm_field(y, tsg, S, d, Ab0, Ab1, WlS, blS, wtS, wv, lane);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) f[sg].v[i] = 0.5f * (fv.v[i] - bv.v[i]);
            }
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                float acc = (float)fx_b<SCHEME>(0) * f[0].v[i];
#pragma unroll
                for (int q = 1; q < NS; ++q) acc = fmaf((float)fx_b<SCHEME>(q), f[q].v[i], acc);
                x.v[i] = fmaf(dt, acc, x.v[i]);
                const int gr = row0 + sm_row(i, lane);
                if (gr < B && col < d) traj[(size_t)(k + 1) * n + (size_t)gr * d + col] = x.v[i];
            }
        }
        __syncthreads();
    }
}

// ---- CNF: one evaluation of [v, div] (the tile kernel of the augmented solves, once) --------------------------
// x: rows of stride ldx (d values each); v: rows of stride ldv; div[row * lddiv] = dsign * div.
// FIELD_GRAD: v = grad_x s and div = its Laplacian (AUG_EXACT), or v alone (AUG_NONE: div is not touched).
template <int MODE, int FIELD = FIELD_MLP>
__global__ __launch_bounds__(256) void ode_small_div(SmArgs A, int B, int d, const float* __restrict__ x, int ldx,
                                                  float t, const float* __restrict__ eps, float* __restrict__ v,
                                                  int ldv, float* __restrict__ div, int lddiv, float dsign) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* Wl = small_lds;
    float* bl = Wl + 4 * SM_W * SM_LD;
    float* wt = bl + 4 * SM_W;
    float* Ab0 = wt + SM_W;
    float* Ab1 = Ab0 + SM_ROWS * SM_LD;
    float* red = Ab1 + SM_ROWS * SM_LD;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    sm_stage_weights(A, d, Wl, bl, wt, tid);
    const int col = wv * 16 + (lane & 15);
    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        SmTile y, ep;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            const bool ok = gr < B && col < d;
            y.v[i] = ok ? x[(size_t)gr * ldx + col] : 0.f;
            ep.v[i] = (MODE == AUG_HUTCH && ok) ? eps[(size_t)gr * d + col] : 0.f;
        }
        __syncthreads();
        SmTile dv, f;
        if constexpr (FIELD == FIELD_GRAD) f = gf_field<MODE == AUG_EXACT>(y, t, A, d, Ab0, Ab1, Wl, bl, wt, B - row0, red, wv, lane, dv);
        else f = sm_field_aug<MODE>(y, t, A, d, Ab0, Ab1, Wl, bl, wt, ep, B - row0, red, wv, lane, dv);
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            if (gr < B && col < d) v[(size_t)gr * ldv + col] = f.v[i];
            if constexpr (MODE != AUG_NONE) {
                if (gr < B && wv == 0 && (lane & 15) == 0) div[(size_t)gr * lddiv] = dsign * dv.v[i];
            }
        }
    }
}

// ---- launch helpers of the tile kernels ---------------------------------------------------------------------------
// Workgroups of ode_small_dopri<TAB, ., MODE, FIELD, REC> that can be resident at once (the grid rendezvous needs grid <= this);
// -1: the query failed.  One result per device and instantiation: the grid is sized from the occupancy of the kernel launched.
template <int TAB, int MODE, int FIELD, bool REC>
static int ode_dopri_resident() {
    constexpr size_t lds = small_lds_bytes(1, 2, MODE != AUG_NONE);
    return cfm_once_per_device([] {
        hipError_t e = hipFuncSetAttribute((const void*)ode_small_dopri<TAB, true, MODE, FIELD, REC>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        hipError_t e2 = hipFuncSetAttribute((const void*)ode_small_dopri<TAB, false, MODE, FIELD, REC>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        int pa = 0, pb = 0;
        if (e == hipSuccess && e2 == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&pa, (const void*)ode_small_dopri<TAB, true, MODE, FIELD, REC>, 256, lds) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&pb, (const void*)ode_small_dopri<TAB, false, MODE, FIELD, REC>, 256, lds) == hipSuccess &&
            pa > 0 && pb > 0)
            return cfm_device_cus() * (pa < pb ? pa : pb);
        return -1;
    });
}

template <int TAB, int MODE, int FIELD, bool REC = false>
static int ode_dopri5_small(const float* const* W, const float* const* b, const int* dims, int B, int d,
                            const float* t_span, int n_t, float tsign, const float* eps, float atol, float rtol,
                            float* traj, int* n_steps, int* nfe, float* xbuf, float* kbuf, float* tspan_dev,
                            void* state_dev, char* sync_dev, float t0, float dt0, int evals0, hipStream_t s,
                            OdeRec rec = OdeRec{nullptr, nullptr, 0}, int* n_accepted = nullptr) {
    const SmArgs A = small_args(W, b, dims);
    constexpr size_t lds = small_lds_bytes(1, 2, MODE != AUG_NONE);
    const int resident = ode_dopri_resident<TAB, MODE, FIELD, REC>();
    // (the recording entry answers CFM_EINVAL only before any GPU work, as a decline its caller may act on: a query that
    // fails here, after the first evaluations, is an error of its own)
    if (resident < 0) return REC ? (int)hipErrorInvalidDeviceFunction : CFM_EINVAL;
    int rc = cfm_hip(hipMemcpyAsync(tspan_dev, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    SmState h[2];
    memset(h, 0, sizeof(h));
    h[0].t = t0; h[0].dt = dt0; h[0].ckpt = 1; h[0].steps = 0; h[0].evals = evals0; h[0].par = 0; h[0].done = 0;
    rc = cfm_hip(hipMemcpyAsync(state_dev, h, sizeof(h), hipMemcpyHostToDevice, s));
    if (rc) return rc;
    double* partial = (double*)sync_dev;
    unsigned long long* lines = (unsigned long long*)(sync_dev + 3 * SM_MAXGRID * 8);
    rc = cfm_hip(hipMemsetAsync(partial, 0xFF, 3 * SM_MAXGRID * 8, s));   // every slot: negative NaN = not arrived
    if (rc) return rc;
    SmState* st = (SmState*)state_dev;
    const int tiles = (B + SM_ROWS - 1) / SM_ROWS;
    int grid = tiles < resident ? tiles : resident;
    if (grid > SM_MAXGRID) grid = SM_MAXGRID;
    // One persistent solve at a time per process: two of them launched from two streams could each get only part
    // of their workgroups resident and wait for the rest forever (the bounded wait would turn that into
    // CFM_ETIMEOUT after 4 s).  The call is synchronous anyway: the lock is held until the solve has finished.
    std::lock_guard<std::mutex> persistent_lock(g_persistent_mu);
    if (tiles <= grid)
        hipLaunchKernelGGL((ode_small_dopri<TAB, true, MODE, FIELD, REC>), dim3(grid), dim3(256), lds, s, A, B, d, st, xbuf, kbuf, tspan_dev, n_t,
                           atol, rtol, traj, partial, lines, 1000000, tsign, eps, rec);
    else
        hipLaunchKernelGGL((ode_small_dopri<TAB, false, MODE, FIELD, REC>), dim3(grid), dim3(256), lds, s, A, B, d, st, xbuf, kbuf, tspan_dev, n_t,
                           atol, rtol, traj, partial, lines, 1000000, tsign, eps, rec);
    rc = cfm_status();
    if (rc) return rc;
    SmState cur, cnt;
    rc = cfm_hip(hipMemcpyAsync(&cur, st + 1, sizeof(SmState), hipMemcpyDeviceToHost, s));
    if (rc) return rc;
    if (REC) {
        rc = cfm_hip(hipMemcpyAsync(&cnt, st + 2, sizeof(SmState), hipMemcpyDeviceToHost, s));
        if (rc) return rc;
    }
    rc = cfm_hip(hipStreamSynchronize(s));
    if (rc) return rc;
    if (REC && n_accepted) *n_accepted = cnt.steps;
    if (n_steps) *n_steps = cur.steps;
    if (nfe) *nfe = cur.evals;
    if (cur.pad == 2) return CFM_ETIMEOUT;
    return cur.done && cur.pad == 0 ? 0 : CFM_ENOCONV;     // (pad 1: max_attempts, pad 3: the step log is full)
}

// the tableau selector (validated by the entry points) picks the instantiation (REC: the plain MLP field only)
template <int MODE, int FIELD = FIELD_MLP, bool REC = false, class... Args>
static int ode_adaptive_small(int tab, Args... args) {
    return tab == CFM_ODE_TSIT5 ? ode_dopri5_small<CFM_ODE_TSIT5, MODE, FIELD, REC>(args...)
                                : ode_dopri5_small<CFM_ODE_DOPRI5, MODE, FIELD, REC>(args...);
}

template <int SCHEME, int MODE, int FIELD>
static int ode_fixed_small_t(const float* const* W, const float* const* b, const int* dims, int B, int d,
                             const float* t_span, int n_t, float* traj, float* tspan_dev, const float* eps,
                             hipStream_t s) {
    const int grid = small_grid<ode_small_fixed<SCHEME, MODE, FIELD>, 128 * 1024>(B);
    if (grid < 0) return CFM_EINVAL;
    int rc = cfm_hip(hipMemcpyAsync(tspan_dev, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    hipLaunchKernelGGL((ode_small_fixed<SCHEME, MODE, FIELD>), dim3(grid), dim3(256), small_lds_bytes(1, 2, MODE != AUG_NONE), s,
                       small_args(W, b, dims), B, d, tspan_dev, n_t, traj, eps);
    return cfm_status();
}

// the scheme selector (validated by the entry points) picks the instantiation
template <int MODE, int FIELD = FIELD_MLP>
static int ode_fixed_small_m(int scheme, const float* const* W, const float* const* b, const int* dims, int B, int d,
                             const float* t_span, int n_t, float* traj, float* tspan_dev, const float* eps, hipStream_t s) {
    if (scheme == CFM_ODE_RK4) return ode_fixed_small_t<CFM_ODE_RK4, MODE, FIELD>(W, b, dims, B, d, t_span, n_t, traj, tspan_dev, eps, s);
    if (scheme == CFM_ODE_MIDPOINT) return ode_fixed_small_t<CFM_ODE_MIDPOINT, MODE, FIELD>(W, b, dims, B, d, t_span, n_t, traj, tspan_dev, eps, s);
    return ode_fixed_small_t<CFM_ODE_EULER, MODE, FIELD>(W, b, dims, B, d, t_span, n_t, traj, tspan_dev, eps, s);
}

static int ode_fixed_small(int scheme, const float* const* W, const float* const* b, const int* dims, int B, int d,
                           const float* t_span, int n_t, float* traj, float* tspan_dev, hipStream_t s) {
    return ode_fixed_small_m<AUG_NONE>(scheme, W, b, dims, B, d, t_span, n_t, traj, tspan_dev, nullptr, s);
}

template <int SCHEME>
static int ode_fixed_pair_small_t(const SmArgs& F, const SmArgs& S, int B, int d, const float* t_span, int n_t, float* traj,
                                  float* tspan_dev, hipStream_t s) {
    const int grid = small_grid<ode_small_fixed_pair<SCHEME>, 160 * 1024>(B);
    if (grid < 0) return CFM_EINVAL;
    int rc = cfm_hip(hipMemcpyAsync(tspan_dev, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    hipLaunchKernelGGL((ode_small_fixed_pair<SCHEME>), dim3(grid), dim3(256), small_lds_bytes(2, 2, false), s, F, S, B, d,
                       tspan_dev, n_t, traj);
    return cfm_status();
}

template <int MODE, int FIELD = FIELD_MLP>
static int cnf_eval(const SmArgs& A, int B, int d, const float* x, int ldx, float t, const float* eps, float* v, int ldv,
                    float* div, int lddiv, float dsign, hipStream_t s) {
    const int grid = small_grid<ode_small_div<MODE, FIELD>, 128 * 1024>(B);
    if (grid < 0) return CFM_EINVAL;
    hipLaunchKernelGGL((ode_small_div<MODE, FIELD>), dim3(grid), dim3(256), small_lds_bytes(1, 2, true), s, A, B, d, x, ldx, t, eps, v, ldv,
                       div, lddiv, dsign);
    return cfm_status();
}

// ---- host drivers: what the entries below share, each written once ------------------------------------------------
// Read-back buffer of the adaptive host drivers (pinned host memory, 64 bytes): one per HOST THREAD, as the assignment
// driver's poll buffer (assign_driver.h, AsgThread) — two threads in adaptive solves on their own streams read their own
// norms and controller words, never each other's.  Allocated by the thread's first read and kept for its lifetime.
static thread_local double* g_ode_pinned = nullptr;

static int read_red(hipStream_t s, const double* dev, int count, double* host) {
    if (count < 1 || count > 8) return CFM_EINVAL;
    double* pinned = g_ode_pinned;
    if (!pinned) {
        int rc = cfm_hip(hipHostMalloc((void**)&pinned, 64, hipHostMallocDefault));
        if (rc) return rc;
        g_ode_pinned = pinned;
    }
    int rc = cfm_hip(hipMemcpyAsync(pinned, dev, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    if (rc) return rc;
    rc = cfm_hip(hipStreamSynchronize(s));
    if (rc) return rc;
    for (int i = 0; i < count; ++i) host[i] = pinned[i];
    return 0;
}

// The argument of ode_combine / ode_error: k[q] and coef(q) for q < n; the kernels read nothing beyond n, where the
// struct holds k[0] and 0.
template <class C>
static Stages ode_stages(float* const* k, int n, C&& coef) {
    Stages st{}; st.n = n;
    for (int q = 0; q < 7; ++q) { st.k[q] = k[q < n ? q : 0]; st.c[q] = q < n ? (float)coef(q) : 0.f; }
    return st;
}

// Whether the one-launch kernels take a solve of the plain MLP field: fused path on, the field inside the tile engine's
// envelope, and room for the t_span copy in w.xt (n = B d >= n_t).  fixed_step: the fixed-step entries also want a step
// to take (n_t >= 2); the adaptive entries have refused n_t < 2 before they ask.
static bool ode_small_path(const int* dims, int n_layers, int d, size_t n, int n_t, bool fixed_step) {
    return cfm_ode_fused_internal() && small_envelope(dims, n_layers, nullptr) == 0 && d + 1 <= SM_W && n >= (size_t)n_t &&
           (!fixed_step || n_t >= 2);
}

// The fixed-step layer-per-kernel driver: explicit RK steps on t_span, one ode_combine per stage state and per step end,
// traj[0] = x0 already in place.  f(t, xin, kout) evaluates a stage derivative.  Any grid is taken as it comes, on purpose
// (the one-launch kernels of these entries do the same): a repeated or non-monotone point is a step of dt <= 0.
template <class F>
static int ode_fixed_layers(F&& f, int scheme, size_t n, const float* t_span, int n_t, float* traj, const OdeWs& w, int* nfe,
                            hipStream_t s) {
    const int ns = fx_stages_host(scheme), nb = ode_blocks(n);
    int evals = 0;
    for (int k = 0; k + 1 < n_t; ++k) {
        const float t = t_span[k], dt = t_span[k + 1] - t_span[k];
        const float* xk = traj + (size_t)k * n;
        for (int sg = 0; sg < ns; ++sg) {
            const float* yin = xk;
            float tsg = t;
            if (sg > 0) {
                hipLaunchKernelGGL(ode_combine, dim3(nb), dim3(256), 0, s, n, xk, dt,
                                   ode_stages(w.k, sg, [&](int q) { return fx_a_host(scheme, sg - 1, q); }), w.xt, (float*)nullptr);
                yin = w.xt;
                tsg = t + (float)fx_c_host(scheme, sg - 1) * dt;
            }
            const int rc = f(tsg, yin, w.k[sg]);
            if (rc) return rc;
            ++evals;
        }
        hipLaunchKernelGGL(ode_combine, dim3(nb), dim3(256), 0, s, n, xk, dt,
                           ode_stages(w.k, ns, [&](int q) { return fx_b_host(scheme, q); }), traj + (size_t)(k + 1) * n, (float*)nullptr);
    }
    if (nfe) *nfe = evals;
    return cfm_status();
}

// Time direction of a t_span (torchdyn's rule): a strictly decreasing grid is integrated as
// g(s, y) = -f(-s, y) on s = -t_span.  ts receives the (increasing) grid the solver steps on; the returned sign
// goes into the field's time argument (f is evaluated at sign * s) and into every stage / init-step coefficient
// (y = x + (sign * dt) * sum a k), so the field arithmetic never changes and the solve is, bit for bit, the
// forward solve of the field whose time column and last layer are negated.  0: not strictly monotone.
static float ode_direction(const float* t_span, int n_t, float* ts) {
    int up = 1, down = 1;
    for (int k = 0; k + 1 < n_t; ++k) {
        if (!(t_span[k + 1] > t_span[k])) up = 0;
        if (!(t_span[k + 1] < t_span[k])) down = 0;
    }
    if (!up && !down) return 0.f;
    const float sg = up ? 1.f : -1.f;
    for (int k = 0; k < n_t; ++k) ts[k] = sg * t_span[k];
    return sg;
}

// The solver-time grid of an adaptive entry, for the length of the call.  sign == 0: no memory, or a t_span that is not
// strictly monotone; the entries answer CFM_EINVAL to both.  (malloc, not new: nothing here throws across the C boundary.)
struct OdeGrid {
    float* ts;
    float sign;
    OdeGrid(const float* t_span, int n_t) : ts((float*)malloc(sizeof(float) * (size_t)n_t)), sign(ts ? ode_direction(t_span, n_t, ts) : 0.f) {}
    ~OdeGrid() { free(ts); }
    OdeGrid(const OdeGrid&) = delete;
    OdeGrid& operator=(const OdeGrid&) = delete;
};

// Hairer II.4 initial step of the host drivers (d0, d1, d2 as RMS norms over n elements).  f(t, x, k) evaluates
// the field at solver time t (s-space: the caller applies the time sign); hsign = the time sign.
template <class F>
static int ode_init_step(F&& f, size_t n, float t, float hsign, float atol, float rtol, const OdeWs& w,
                         hipStream_t s, float* dt_out) {
    const int nb = ode_blocks(n);
    const float order = 5.f;
    auto rms = [&](double sumsq) -> float { return (float)sqrt(sumsq / (double)n); };
    int rc = cfm_hip(hipMemsetAsync(w.red, 0, 64, s));
    if (rc) return rc;
    hipLaunchKernelGGL(ode_sqnorm, dim3(nb), dim3(256), 0, s, n, w.x, (const float*)nullptr, w.x, atol, rtol, w.red + 0);
    hipLaunchKernelGGL(ode_sqnorm, dim3(nb), dim3(256), 0, s, n, w.k[0], (const float*)nullptr, w.x, atol, rtol, w.red + 1);
    double r2[3];
    rc = read_red(s, w.red, 2, r2);
    if (rc) return rc;
    const float d0 = rms(r2[0]), d1 = rms(r2[1]);
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1;
    hipLaunchKernelGGL(ode_combine, dim3(nb), dim3(256), 0, s, n, w.x, hsign * h0, ode_stages(w.k, 1, [](int) { return 1.f; }), w.xt,
                       (float*)nullptr);
    rc = f(t + h0, w.xt, w.k[1]);
    if (rc) return rc;
    hipLaunchKernelGGL(ode_sqnorm, dim3(nb), dim3(256), 0, s, n, w.k[1], w.k[0], w.x, atol, rtol, w.red + 2);
    rc = read_red(s, w.red + 2, 1, r2);
    if (rc) return rc;
    const float d2 = rms(r2[0]) / h0;
    float h1;
    if (d1 <= 1e-15f && d2 <= 1e-15f) h1 = fmaxf(1e-6f, h0 * 1e-3f);
    else h1 = powf(0.01f / fmaxf(d1, d2), 1.0f / (order + 1.f));
    *dt_out = fminf(100.f * h0, h1);
    return 0;
}

// The start of an adaptive solve on the host: x0 into w.x and traj[0], k_1 = f(t0, x0) into w.k[0], the initial step.
template <class F>
static int ode_adaptive_start(F&& f, const float* x0, size_t n, float t0, float tsign, float atol, float rtol, const OdeWs& w,
                              float* traj, hipStream_t s, float* dt_out) {
    int rc = cfm_hip(hipMemcpyAsync(w.x, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (rc) return rc;
    rc = cfm_hip(hipMemcpyAsync(traj, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (rc) return rc;
    rc = f(t0, w.x, w.k[0]);
    if (rc) return rc;
    return ode_init_step(f, n, t0, tsign, atol, rtol, w, s, dt_out);
}

static int ode_dopri5_layers(int tab, const float* const* W, const float* const* b, const int* dims, int n_layers, int d,
                             const float* x0, int B, const float* t_span, int n_t, float tsign, float atol,
                             float rtol, float* traj, int* n_steps, int* nfe, void* ws, void* stream,
                             const OdeRec* rec = nullptr, int* n_accepted = nullptr) {
    hipStream_t s = (hipStream_t)stream;
    OdeWs w = ode_carve(ws, B, maxwidth(dims, n_layers), d);
    const size_t n = (size_t)B * d;
    // small vector fields: the whole step attempt in one kernel, controller on the device
    const bool small = ode_small_path(dims, n_layers, d, n, n_t, false);
    if (rec && !small) return CFM_EINVAL;              // only the one-launch kernel records its steps: declined before any GPU work
    const int nb = ode_blocks(n);
    int evals = 0, steps = 0;

    auto f = [&](float t, const float* xin, float* kout) -> int {
        ++evals;
        return cfm_mlp_forward_impl(xin, nullptr, tsign * t, 1, 0, W, b, dims, n_layers, B, kout, w.act, s);
    };
    float t = t_span[0], dt;
    const float T = t_span[n_t - 1];
    int rc = ode_adaptive_start(f, x0, n, t, tsign, atol, rtol, w, traj, s, &dt);
    if (rc) return rc;

    if (small && rec)
        return ode_adaptive_small<AUG_NONE, FIELD_MLP, true>(tab, W, b, dims, B, d, t_span, n_t, tsign, nullptr, atol, rtol, traj, n_steps,
                                                             nfe, w.x, w.k[0], w.xt, (void*)(w.red + 16), w.sync, t, dt, evals, s, *rec,
                                                             n_accepted);
    if (small)
        return ode_adaptive_small<0>(tab, W, b, dims, B, d, t_span, n_t, tsign, nullptr, atol, rtol, traj, n_steps, nfe, w.x,
                                   w.k[0], w.xt, (void*)(w.red + 16), w.sync, t, dt, evals, s);

    int ckpt = 1;  // next t_span index to land on
    const int max_attempts = 1000000;
    while (t < T && steps < max_attempts) {
        if (t + dt > T) dt = T - t;
        float dt_old = dt; bool flag = false;
        if (ckpt < n_t && t + dt > t_span[ckpt]) { dt_old = dt; flag = true; dt = t_span[ckpt] - t; }
        const bool lands = (ckpt < n_t) && (flag || t + dt == t_span[ckpt]);
        // stages k2..k6, then x_new and k7 (FSAL)
        for (int sIdx = 0; sIdx < 6; ++sIdx) {
            float* dst = (sIdx == 5) ? w.xn : w.xt;
            hipLaunchKernelGGL(ode_combine, dim3(nb), dim3(256), 0, s, n, w.x, tsign * dt,
                               ode_stages(w.k, sIdx + 1, [&](int q) { return rk_a_host(tab, sIdx, q); }), dst, (float*)nullptr);
            rc = f(t + rk_c_host(tab, sIdx) * dt, dst, w.k[sIdx + 1]);
            if (rc) return rc;
        }
        rc = cfm_hip(hipMemsetAsync(w.red + 4, 0, 8, s));
        if (rc) return rc;
        hipLaunchKernelGGL(ode_error, dim3(nb), dim3(256), 0, s, n, w.x, w.xn, dt, ode_stages(w.k, 7, [&](int q) { return rk_e_host(tab, q); }),
                           atol, rtol, w.red + 4);
        hipLaunchKernelGGL(ode_controller, dim3(1), dim3(1), 0, s, w.red + 4, (double)n, (float*)(w.red + 6));
        double ctl;
        rc = read_red(s, w.red + 6, 1, &ctl);
        if (rc) return rc;
        ++steps;
        float ratio, factor;
        memcpy(&ratio, (const char*)&ctl, 4); memcpy(&factor, (const char*)&ctl + 4, 4);
        const bool accept = ratio <= 1.f;
        if (accept) {
            if (lands) {
                t = t_span[ckpt];
                rc = cfm_hip(hipMemcpyAsync(traj + (size_t)ckpt * n, w.xn, n * sizeof(float), hipMemcpyDeviceToDevice, s));
                if (rc) return rc;
                ++ckpt;
            } else {
                t = t + dt;
            }
            float* tmp = w.x; w.x = w.xn; w.xn = tmp;          // x <- x_new
            tmp = w.k[0]; w.k[0] = w.k[6]; w.k[6] = tmp;        // k1 <- k7 (FSAL)
        }
        if (flag) dt = dt_old - dt;
        dt = dt * factor;                  // (ode_step_factor on the device, see ode_controller)
        if (!(dt > 1e-12f)) dt = 1e-12f;   // guard (documented deviation)
    }
    if (n_steps) *n_steps = steps;
    if (nfe) *nfe = evals;
    rc = cfm_hip(hipStreamSynchronize(s));
    if (rc) return rc;
    return (t < T) ? CFM_ENOCONV : 0;
}

// Adaptive solve of a small field whose first evaluations and initial step come from the one-evaluation kernel:
// the augmented MLP field (state [B, 1 + d]) and the plain gradient field (state [B, d]).
template <int MODE, int FIELD = FIELD_MLP>
static int cnf_dopri5(int tab, const SmArgs& A, const float* const* W, const float* const* b, const int* dims, int d,
                      const float* x0, int B, const float* ts, int n_t, float tsign, const float* eps, float atol,
                      float rtol, float* traj, int* n_steps, int* nfe, void* ws, hipStream_t s) {
    const int D = MODE != AUG_NONE ? d + 1 : d;
    OdeWs w = ode_carve(ws, B, maxwidth(dims, 4), D);  // workspace of CFM_OP_ODE at D: every buffer is [B, D] (4: both envelopes)
    const size_t n = (size_t)B * D;
    if (n < (size_t)n_t) return CFM_EINVAL;            // t_span copy: w.xt (the kernel's x / k buffers are w.x and w.k[0]); deliberate
    int evals = 0;
    // the field in solver time, at tsign * t (the sign of g = -f(-s, .) rides on the coefficients); augmented: k = [-div, v]
    auto f = [&](float t, const float* xin, float* kout) -> int {
        ++evals;
        if constexpr (MODE == AUG_NONE) return cnf_eval<MODE, FIELD>(A, B, d, xin, D, tsign * t, eps, kout, D, nullptr, 0, 0.f, s);
        else return cnf_eval<MODE, FIELD>(A, B, d, xin + 1, D, tsign * t, eps, kout + 1, D, kout, D, -1.f, s);
    };
    const float t = ts[0];
    float dt;
    const int rc = ode_adaptive_start(f, x0, n, t, tsign, atol, rtol, w, traj, s, &dt);   // d0, d1, d2 over all B D elements
    if (rc) return rc;
    return ode_adaptive_small<MODE, FIELD>(tab, W, b, dims, B, d, ts, n_t, tsign, eps, atol, rtol, traj, n_steps, nfe, w.x, w.k[0],
                                         w.xt, (void*)(w.red + 16), w.sync, t, dt, evals, s);
}

// a fixed-step grid: strictly monotone, either way
static int fx_monotone(const float* t_span, int n_t) {
    for (int k = 0; k + 1 < n_t; ++k)
        if (!(t_span[k + 1] > t_span[k]) && !(t_span[k + 1] < t_span[k])) return 0;
    if (n_t > 2) {
        const int up = t_span[1] > t_span[0];
        for (int k = 1; k + 1 < n_t; ++k) if ((t_span[k + 1] > t_span[k]) != up) return 0;
    }
    return 1;
}

// The fixed-step entries that have the one launch only (CNF, gradient field, regularised CNF), up to the launch.
// envelope(&d) is the entry's own check; the state of x0 / traj and the CFM_OP_ODE workspace are [B, D], D = d + aug_cols.
// Deliberately unlike the plain and pair entries: the grid must be strictly monotone (fx_monotone), and the t_span copy
// lives in w.x .. w.xt, so only n_t > 3 B D is refused, before any GPU work.  traj[0] = x0 and *nfe are written before
// the launch (nfe stands even when the launch fails); n_t = 1 ends there.  launch(d, tspan_dev, s) does the rest.
template <class Envelope, class Launch>
static int ode_fixed_onelaunch(const float* x0, int B, const float* t_span, int n_t, float* traj, int* nfe, int stages,
                               int aug_cols, const int* dims, int n_layers, void* ws, void* stream, Envelope&& envelope,
                               Launch&& launch) {
    int d;
    if (!x0 || !t_span || !traj || !ws || n_t < 1) return CFM_EINVAL;
    int rc = envelope(&d);
    if (rc) return rc;
    if (!fx_monotone(t_span, n_t)) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    OdeWs w = ode_carve(ws, B, maxwidth(dims, n_layers), d + aug_cols);
    const size_t n = (size_t)B * (d + aug_cols);
    if ((size_t)n_t > 3 * n) return CFM_EINVAL;
    rc = cfm_hip(hipMemcpyAsync(traj, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (rc) return rc;
    if (nfe) *nfe = stages * (n_t - 1);
    if (n_t < 2) return 0;
    return launch(d, w.x, s);
}

// ---- the C entries ------------------------------------------------------------------------------------------------
extern "C" int cfm_ode_fixed_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                                     int n_layers, const float* x0, int B, const float* t_span,
                                     int n_t, int scheme, float* traj, int* nfe, void* ws, void* stream) {
    int d;
    if (!W || !b || !x0 || !t_span || !traj || !ws || B <= 0 || n_t < 1 || !fx_known(scheme)) return CFM_EINVAL;
    int rc = check_mlp(dims, n_layers, &d);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    OdeWs w = ode_carve(ws, B, maxwidth(dims, n_layers), d);
    const size_t n = (size_t)B * d;
    rc = cfm_hip(hipMemcpyAsync(traj, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (rc) return rc;
    // small vector fields: rows are independent and the steps are fixed, so ONE launch integrates the
    // whole t_span (a workgroup walks its 64-row tile through every step, weights resident in LDS)
    if (ode_small_path(dims, n_layers, d, n, n_t, true)) {
        rc = ode_fixed_small(scheme, W, b, dims, B, d, t_span, n_t, traj, w.xt, s);
        if (nfe) *nfe = fx_stages_host(scheme) * (n_t - 1);        // (written even when the launch failed)
        return rc;
    }
    return ode_fixed_layers([&](float t, const float* xin, float* kout) {
        return cfm_mlp_forward_impl(xin, nullptr, t, 1, 0, W, b, dims, n_layers, B, kout, w.act, s);
    }, scheme, n, t_span, n_t, traj, w, nfe, s);
}

extern "C" int cfm_ode_euler_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                                     int n_layers, const float* x0, int B, const float* t_span,
                                     int n_t, float* traj, int* nfe, void* ws, void* stream) {
    return cfm_ode_fixed_mlp_f32(W, b, dims, n_layers, x0, B, t_span, n_t, CFM_ODE_EULER, traj, nfe, ws, stream);
}

extern "C" int cfm_ode_fixed_pair_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Wb,
                                          const float* const* bb, const int* dims, int n_layers, const float* x0, int B,
                                          const float* t_span, int n_t, int scheme, float* traj, int* nfe, void* ws,
                                          void* stream) {
    int d;
    if (!Wf || !bf || !Wb || !bb || !x0 || !t_span || !traj || !ws || B <= 0 || n_t < 1 || !fx_known(scheme)) return CFM_EINVAL;
    int rc = check_mlp(dims, n_layers, &d);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    OdeWs w = ode_carve(ws, B, maxwidth(dims, n_layers), d);
    const size_t n = (size_t)B * d;
    rc = cfm_hip(hipMemcpyAsync(traj, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (rc) return rc;
    if (ode_small_path(dims, n_layers, d, n, n_t, true)) {
        const SmArgs F = small_args(Wf, bf, dims), S = small_args(Wb, bb, dims);
        if (scheme == CFM_ODE_RK4) rc = ode_fixed_pair_small_t<CFM_ODE_RK4>(F, S, B, d, t_span, n_t, traj, w.xt, s);
        else if (scheme == CFM_ODE_MIDPOINT) rc = ode_fixed_pair_small_t<CFM_ODE_MIDPOINT>(F, S, B, d, t_span, n_t, traj, w.xt, s);
        else rc = ode_fixed_pair_small_t<CFM_ODE_EULER>(F, S, B, d, t_span, n_t, traj, w.xt, s);
        if (nfe) *nfe = fx_stages_host(scheme) * (n_t - 1);        // (written even when the launch failed)
        return rc;
    }
    // the stage derivative of the layer driver: two forward passes (the second net's output in w.x) and the halved difference
    return ode_fixed_layers([&](float t, const float* xin, float* kout) {
        int rc = cfm_mlp_forward_impl(xin, nullptr, t, 1, 0, Wf, bf, dims, n_layers, B, kout, w.act, s);
        if (rc) return rc;
        rc = cfm_mlp_forward_impl(xin, nullptr, t, 1, 0, Wb, bb, dims, n_layers, B, w.x, w.act, s);
        if (rc) return rc;
        hipLaunchKernelGGL(ode_half_diff, dim3(ode_blocks(n)), dim3(256), 0, s, n, kout, w.x);
        return 0;
    }, scheme, n, t_span, n_t, traj, w, nfe, s);
}

extern "C" int cfm_ode_adaptive_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                                        int n_layers, const float* x0, int B, const float* t_span,
                                        int n_t, int tableau, float atol, float rtol, float* traj, int* n_steps,
                                        int* nfe, void* ws, void* stream) {
    int d;
    if (!W || !b || !x0 || !t_span || !traj || !ws || B <= 0 || n_t < 2 || !rk_adaptive_known(tableau)) return CFM_EINVAL;
    int rc = check_mlp(dims, n_layers, &d);
    if (rc) return rc;
    const OdeGrid g(t_span, n_t);
    if (g.sign == 0.f) return CFM_EINVAL;
    return ode_dopri5_layers(tableau, W, b, dims, n_layers, d, x0, B, g.ts, n_t, g.sign, atol, rtol, traj, n_steps, nfe, ws, stream);
}

extern "C" int cfm_ode_dopri5_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                                      int n_layers, const float* x0, int B, const float* t_span,
                                      int n_t, float atol, float rtol, float* traj, int* n_steps,
                                      int* nfe, void* ws, void* stream) {
    return cfm_ode_adaptive_mlp_f32(W, b, dims, n_layers, x0, B, t_span, n_t, CFM_ODE_DOPRI5, atol, rtol, traj, n_steps, nfe, ws, stream);
}

// cfm_ode_adaptive_mlp_f32 on the recording instantiation of the one-launch kernel: the same arithmetic (traj, n_steps and
// nfe are its bits), plus the starting state and the record of every accepted step.  CFM_EINVAL wherever the plain entry
// would leave that kernel; CFM_ENOCONV when the log filled up before the end of the grid.
extern "C" int cfm_ode_adaptive_rec_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                                            int n_layers, const float* x0, int B, const float* t_span,
                                            int n_t, int tableau, float atol, float rtol, float* traj, int* n_steps,
                                            int* nfe, int max_steps, void* log, float* ysteps, int* n_accepted, void* ws,
                                            void* stream) {
    int d;
    if (!W || !b || !x0 || !t_span || !traj || !ws || B <= 0 || n_t < 2 || !rk_adaptive_known(tableau)) return CFM_EINVAL;
    if (max_steps < 1 || !log || !ysteps || !n_accepted) return CFM_EINVAL;
    int rc = check_mlp(dims, n_layers, &d);
    if (rc) return rc;
    const OdeGrid g(t_span, n_t);
    if (g.sign == 0.f) return CFM_EINVAL;
    const OdeRec rec{(OdeStepRec*)log, ysteps, max_steps};
    *n_accepted = 0;                // (a decline off the one-launch path, below, already reads 0)
    return ode_dopri5_layers(tableau, W, b, dims, n_layers, d, x0, B, g.ts, n_t, g.sign, atol, rtol, traj, n_steps, nfe, ws, stream,
                             &rec, n_accepted);
}

// Rows up to which the recording solve keeps its state in registers (one 16-row tile per resident workgroup); above, x and
// k_1 travel through the parity buffers.  For tests and measurements that must sit on either side of that limit; < 0: the
// occupancy query failed or the tableau is unknown.
extern "C" int cfm_ode_rec_resident_rows(int tableau) {
    if (!rk_adaptive_known(tableau)) return CFM_EINVAL;
    int g = tableau == CFM_ODE_TSIT5 ? ode_dopri_resident<CFM_ODE_TSIT5, AUG_NONE, FIELD_MLP, true>()
                                     : ode_dopri_resident<CFM_ODE_DOPRI5, AUG_NONE, FIELD_MLP, true>();
    if (g < 0) return CFM_EINVAL;
    return SM_ROWS * (g < SM_MAXGRID ? g : SM_MAXGRID);
}

extern "C" int cfm_mlp_divergence_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                      const float* x, int B, float t, int mode, const float* eps, float* v, float* div,
                                      void* ws, void* stream) {
    int d; SmArgs A;
    (void)ws;
    if (!x || !v || !div) return CFM_EINVAL;
    int rc = cnf_check(W, b, dims, n_layers, B, mode, eps, &d, &A);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return mode == 0 ? cnf_eval<AUG_EXACT>(A, B, d, x, d, t, eps, v, d, div, 1, 1.f, s)
                     : cnf_eval<AUG_HUTCH>(A, B, d, x, d, t, eps, v, d, div, 1, 1.f, s);
}

extern "C" int cfm_ode_fixed_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                         const float* x0, int B, const float* t_span, int n_t, int mode,
                                         const float* eps, int scheme, float* traj, int* nfe, void* ws, void* stream) {
    SmArgs A;
    if (!fx_known(scheme)) return CFM_EINVAL;
    return ode_fixed_onelaunch(x0, B, t_span, n_t, traj, nfe, fx_stages_host(scheme), 1, dims, n_layers, ws, stream,
        [&](int* d) { return cnf_check(W, b, dims, n_layers, B, mode, eps, d, &A); },
        [&](int d, float* tspan_dev, hipStream_t s) {
            return mode == 0 ? ode_fixed_small_m<AUG_EXACT>(scheme, W, b, dims, B, d, t_span, n_t, traj, tspan_dev, eps, s)
                             : ode_fixed_small_m<AUG_HUTCH>(scheme, W, b, dims, B, d, t_span, n_t, traj, tspan_dev, eps, s);
        });
}

extern "C" int cfm_ode_euler_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                         const float* x0, int B, const float* t_span, int n_t, int mode,
                                         const float* eps, float* traj, int* nfe, void* ws, void* stream) {
    return cfm_ode_fixed_cnf_mlp_f32(W, b, dims, n_layers, x0, B, t_span, n_t, mode, eps, CFM_ODE_EULER, traj, nfe, ws, stream);
}

extern "C" int cfm_ode_adaptive_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                            const float* x0, int B, const float* t_span, int n_t, int mode,
                                            const float* eps, int tableau, float atol, float rtol, float* traj,
                                            int* n_steps, int* nfe, void* ws, void* stream) {
    int d; SmArgs A;
    if (!x0 || !t_span || !traj || !ws || n_t < 2 || !rk_adaptive_known(tableau)) return CFM_EINVAL;
    int rc = cnf_check(W, b, dims, n_layers, B, mode, eps, &d, &A);
    if (rc) return rc;
    const OdeGrid g(t_span, n_t);
    if (g.sign == 0.f) return CFM_EINVAL;
    return mode == 0 ? cnf_dopri5<AUG_EXACT>(tableau, A, W, b, dims, d, x0, B, g.ts, n_t, g.sign, eps, atol, rtol, traj, n_steps, nfe, ws,
                                             (hipStream_t)stream)
                     : cnf_dopri5<AUG_HUTCH>(tableau, A, W, b, dims, d, x0, B, g.ts, n_t, g.sign, eps, atol, rtol, traj, n_steps, nfe, ws,
                                             (hipStream_t)stream);
}

extern "C" int cfm_ode_dopri5_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                          const float* x0, int B, const float* t_span, int n_t, int mode,
                                          const float* eps, float atol, float rtol, float* traj, int* n_steps,
                                          int* nfe, void* ws, void* stream) {
    return cfm_ode_adaptive_cnf_mlp_f32(W, b, dims, n_layers, x0, B, t_span, n_t, mode, eps, CFM_ODE_DOPRI5, atol, rtol, traj,
                                        n_steps, nfe, ws, stream);
}

// ---- action matching: v = grad_x s(x, t) of a scalar action net (grad_field.h) -------------------------------------
// (the envelope of these entries: grad_check, ode_envelope.h)
extern "C" int cfm_mlp_grad_field_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                      const float* x, int ldx, int B, float t, float* v, float* lap, void* ws,
                                      void* stream) {
    int d; SmArgs A;
    (void)ws;
    if (!x || !v) return CFM_EINVAL;
    int rc = grad_check(W, b, dims, n_layers, B, &d, &A);
    if (rc) return rc;
    if (ldx < d) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    return lap ? cnf_eval<AUG_EXACT, FIELD_GRAD>(A, B, d, x, ldx, t, nullptr, v, d, lap, 1, 1.f, s)
               : cnf_eval<AUG_NONE, FIELD_GRAD>(A, B, d, x, ldx, t, nullptr, v, d, nullptr, 0, 0.f, s);
}

// D = d (plain) or d + 1 (augmented, MODE = AUG_EXACT): the state width of x0 / traj and of the CFM_OP_ODE workspace
template <int MODE>
static int grad_fixed(const float* const* W, const float* const* b, const int* dims, int n_layers, const float* x0, int B,
                      const float* t_span, int n_t, int scheme, float* traj, int* nfe, void* ws, void* stream) {
    SmArgs A;
    if (!fx_known(scheme)) return CFM_EINVAL;
    return ode_fixed_onelaunch(x0, B, t_span, n_t, traj, nfe, fx_stages_host(scheme), MODE != AUG_NONE, dims, n_layers, ws, stream,
        [&](int* d) { return grad_check(W, b, dims, n_layers, B, d, &A); },
        [&](int d, float* tspan_dev, hipStream_t s) {
            return ode_fixed_small_m<MODE, FIELD_GRAD>(scheme, W, b, dims, B, d, t_span, n_t, traj, tspan_dev, nullptr, s);
        });
}

extern "C" int cfm_ode_fixed_gradmlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                         const float* x0, int B, const float* t_span, int n_t, int scheme, float* traj,
                                         int* nfe, void* ws, void* stream) {
    return grad_fixed<AUG_NONE>(W, b, dims, n_layers, x0, B, t_span, n_t, scheme, traj, nfe, ws, stream);
}

extern "C" int cfm_ode_fixed_cnf_gradmlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                             const float* x0, int B, const float* t_span, int n_t, int mode,
                                             const float* eps, int scheme, float* traj, int* nfe, void* ws, void* stream) {
    (void)eps;
    if (mode != 0) return CFM_EINVAL;                  // the exact trace only
    return grad_fixed<AUG_EXACT>(W, b, dims, n_layers, x0, B, t_span, n_t, scheme, traj, nfe, ws, stream);
}

extern "C" int cfm_ode_adaptive_gradmlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                            const float* x0, int B, const float* t_span, int n_t, int tableau, float atol,
                                            float rtol, float* traj, int* n_steps, int* nfe, void* ws, void* stream) {
    int d; SmArgs A;
    if (!x0 || !t_span || !traj || !ws || n_t < 2 || !rk_adaptive_known(tableau)) return CFM_EINVAL;
    int rc = grad_check(W, b, dims, n_layers, B, &d, &A);
    if (rc) return rc;
    const OdeGrid g(t_span, n_t);
    if (g.sign == 0.f) return CFM_EINVAL;
    return cnf_dopri5<AUG_NONE, FIELD_GRAD>(tableau, A, W, b, dims, d, x0, B, g.ts, n_t, g.sign, nullptr, atol, rtol, traj, n_steps, nfe,
                                            ws, (hipStream_t)stream);
}

// ---- regularised CNF training: the Euler solve with the kinetic / Jacobian path integrals (ode_small_euler_reg of
// cnf_reg.hip, cfm_ode_euler_cnf_reg_mlp_f32) ----
#include "cnf_reg.h"

// The gradients of these solves (CNF, regularised CNF, fixed-step, adaptive, action matching) are a translation unit of
// their own, small_grad.hip: folding or moving their code cannot perturb the kernels above.  Host code of this file can
// be folded and moved freely, as long as the device text of every kernel stays what it was (profiles/ode_host_fold.txt:
// all 51 kernels compared before and after); the device-side folds that were measured and lost are in
// profiles/ode_unit_fold.txt and profiles/grad_unit_split.txt.
