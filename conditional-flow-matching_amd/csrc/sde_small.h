// sde_small.h — the one-launch SDE samplers of the small fields (included by ode.hip): Philox normals, ode_small_em,
// ode_small_srk (per-element arithmetic: sde_srk.h) and their entry points, on the tile engine of small_field.h.
#pragma once
#include "small_field.h"
#include "sde_srk.h"

// ------------------------------------------------------------ SF2M: Euler-Maruyama ----
// y <- y + h (v(te, y) + s(te, y)) + g sqrt|h| xi  for every step of the grid, the whole trajectory of a tile in ONE
// launch: both small fields (flow v and score s: 4 layers, widths <= 64) live in LDS (2 x 69 KB), the state in
// registers.  Same arithmetic, in the same order, as the launch-per-step scheme (sde.py: two forward passes on
// mlp_layer + cfm_sde_em_step_f32: f = fma(1, s, +-v); r = fma(h, f, y); r = fma(g sqrt|h|, xi, r)) — with the
// caller's noise (xi != NULL) the trajectory is bit-equal to it.  xi == NULL: N(0, 1) from Philox4x32-10 in the
// kernel (counter = step, element index; key = seed), Box-Muller.
// Replaces torchsde.sdeint(SDE(model, score_model), x0, ts, method="euler", dt=...), i.e.
// runner/src/models/components/solver.py:157-182 at sde_solver: euler, for the small fields the examples train.  (The
// notebooks themselves do not select it: SF2M_tutorial.ipynb cell 5 passes solver="euler", a keyword torchsde ignores,
// and runs torchsde's default "srk" — ode_small_srk below.)
__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
// w3: counter word 3 names the stream (0x5f2d: the Euler-Maruyama increments and xi1 of srk; 0x5f2e: xi2 of srk)
__device__ __forceinline__ void philox_normal4_w3(unsigned long long seed, unsigned step, unsigned long long elem, unsigned w3,
                                                  float (&z)[4]) {
    unsigned c[4] = {(unsigned)elem, (unsigned)(elem >> 32), step, w3};
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    // Box-Muller on (0, 1] uniforms
    const float u0 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f), u1 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 1.0f) * (1.0f / 16777216.0f), u3 = (float)(c[3] >> 8) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u1, &s0, &c0); sincosf(6.283185307179586f * u3, &s1, &c1);
    z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned step, unsigned long long elem, float (&z)[4]) {
    philox_normal4_w3(seed, step, elem, 0x5f2du, z);
}

struct EmStep { float te, h, gs; int is_out; };      // per step: field time, step, g sqrt|h|, trajectory point after it

// ---- LOGQP: the path KL beside the state (torchsde's sdeint(..., logqp=True) with h = 0) ----
// One more drift-only component, lr' = 1/2 sum_j (f_j / g)^2, integrated by the scheme that runs the state and written
// per OUTPUT INTERVAL (logratio [n_out, B]: the increase since the previous trajectory point, not a running sum).  The
// step's drift tile is squared where the step forms it, reduced per row (sm_rowsum: 16 lanes, then the four waves
// through `red`, the 4 x SM_ROWS floats behind the tile buffers) and accumulated as lr = fma(qw_k, rowsum, lr) with
// ONE host-computed float per step (Euler-Maruyama: qw_k = h_k / (2 g_k^2); srk: h / (12 sigma^2), the sum being
// (k1^2 + k2^2) + 4 k3^2).  Columns >= d of a drift tile are zero; rows >= B are summed and never stored.  sm_rowsum
// runs once per step: its next write to `red` comes a whole field evaluation (several barriers) after its reads.
// The state update is the plain kernel's, statement for statement: the trajectory keeps its bits.
enum { SDE_REVERSE = 1, SDE_LOGQP = 2 };              // the entries' flag word
static_assert(small_lds_bytes(2, 2, true) == 150784 && small_lds_bytes(2, 2, true) <= 160 * 1024,
              "the two-net SDE kernels with the row-sum scratch of LOGQP");

// wave 0's lanes that lead a row group hand the interval's log-ratio out; every lane starts the next interval at zero
__device__ __forceinline__ void sde_logqp_out(SmTile& lr, float* __restrict__ logratio, int oidx, int row0, int B, int wv,
                                              int lane) {
    if (wv == 0 && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            if (gr < B) logratio[(size_t)oidx * B + gr] = lr.v[i];
        }
    }
#pragma unroll
    for (int i = 0; i < SM_V; ++i) lr.v[i] = 0.f;
}

template <bool LOGQP>
__global__ __launch_bounds__(256) void ode_small_em(SmArgs F, SmArgs S, int has_s, int B, int d,
                                                    const EmStep* __restrict__ steps, int n_steps, int flags,
                                                    const float* __restrict__ xi, unsigned long long seed,
                                                    const float* __restrict__ y0, float* __restrict__ out,
                                                    const float* __restrict__ qw, float* __restrict__ logratio) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* WlF = small_lds;
    float* blF = WlF + 4 * SM_W * SM_LD;
    float* wtF = blF + 4 * SM_W;
    float* WlS = wtF + SM_W;
    float* blS = WlS + 4 * SM_W * SM_LD;
    float* wtS = blS + 4 * SM_W;
    float* Ab0 = wtS + SM_W;
    float* Ab1 = Ab0 + SM_ROWS * SM_LD;
    float* red = Ab1 + SM_ROWS * SM_LD;               // (LOGQP alone carves and touches it)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool reverse = (flags & SDE_REVERSE) != 0;
    sm_stage_weights(F, d, WlF, blF, wtF, tid);
    if (has_s) sm_stage_weights(S, d, WlS, blS, wtS, tid);
    const size_t n = (size_t)B * d;
    const int col = wv * 16 + (lane & 15);
    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        SmTile x;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            x.v[i] = (gr < B && col < d) ? y0[(size_t)gr * d + col] : 0.f;
        }
        __syncthreads();
        int oidx = 0;
        SmTile lr, q;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) lr.v[i] = q.v[i] = 0.f;
        for (int k = 0; k < n_steps; ++k) {
            const EmStep st = steps[k];
            const SmTile v = sm_field(x, st.te, F, d, Ab0, Ab1, WlF, blF, wtF, wv, lane);
            SmTile sc;
            if (has_s) sc = sm_field(x, st.te, S, d, Ab0, Ab1, WlS, blS, wtS, wv, lane);
            static_assert(SM_V == 4, "ode_small_em draws ONE Philox block of 4 normals per lane and step: with SM_MB > 1 "
                                     "elements i and i + 4 would share a normal (draw SM_V / 4 blocks, counter word + (i >> 2))");
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (!xi && st.gs != 0.f) philox_normal4(seed, (unsigned)k, (unsigned long long)(row0 / SM_ROWS) * 256 + tid, z);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const int gr = row0 + sm_row(i, lane);
                const bool ok = gr < B && col < d;
                float f = reverse ? -v.v[i] : v.v[i];
                if (has_s) f = fmaf(1.0f, sc.v[i], f);
                if constexpr (LOGQP) q.v[i] = f * f;
                float r = fmaf(st.h, f, x.v[i]);
                const float noise = xi ? (ok ? xi[(size_t)k * n + (size_t)gr * d + col] : 0.f) : z[i & 3];
                r = fmaf(st.gs, noise, r);
                x.v[i] = ok ? r : 0.f;
                if (st.is_out && ok) out[(size_t)oidx * n + (size_t)gr * d + col] = r;
            }
            if constexpr (LOGQP) {
                const float w = qw[k];
                const SmTile rs = sm_rowsum(q, red, wv, lane);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) lr.v[i] = fmaf(w, rs.v[i], lr.v[i]);
                if (st.is_out) sde_logqp_out(lr, logratio, oidx, row0, B, wv, lane);
            }
            oidx += st.is_out ? 1 : 0;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------ SF2M: srk (SRI2W1, constant g) ----
// The scheme torchsde.sdeint runs when no method is given (diagonal Ito noise -> "srk"), which is how the reference's
// notebooks call it (single-cell_example.ipynb, mnist_example.ipynb, conditional_mnist.ipynb; SF2M_tutorial.ipynb's
// solver="euler" is an ignored keyword) and what runner/src/models/components/solver.py:169-179 runs for
// sde_solver: srk.  Per step three evaluations of the field pair, at t, t + h and t + h/2 (sde_srk.h has the
// scheme); x, k1, k2 stay in registers for the whole trajectory of the tile.  Layout, LDS use and the xi == NULL
// Philox mode are ode_small_em's; xi != NULL is [n_steps, 2, B, d] (plane 0: xi1, plane 1: xi2) and the trajectory
// is then bit-equal to the launch-per-step scheme (three forward passes per field + cfm_sde_srk_step_f32).
template <bool LOGQP>
__global__ __launch_bounds__(256) void ode_small_srk(SmArgs F, SmArgs S, int has_s, int B, int d,
                                                     const SrkStep* __restrict__ steps, int n_steps, int flags,
                                                     const float* __restrict__ xi, unsigned long long seed,
                                                     const float* __restrict__ y0, float* __restrict__ out,
                                                     const float* __restrict__ qw, float* __restrict__ logratio) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* WlF = small_lds;
    float* blF = WlF + 4 * SM_W * SM_LD;
    float* wtF = blF + 4 * SM_W;
    float* WlS = wtF + SM_W;
    float* blS = WlS + 4 * SM_W * SM_LD;
    float* wtS = blS + 4 * SM_W;
    float* Ab0 = wtS + SM_W;
    float* Ab1 = Ab0 + SM_ROWS * SM_LD;
    float* red = Ab1 + SM_ROWS * SM_LD;               // (LOGQP alone carves and touches it)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool reverse = (flags & SDE_REVERSE) != 0;
    sm_stage_weights(F, d, WlF, blF, wtF, tid);
    if (has_s) sm_stage_weights(S, d, WlS, blS, wtS, tid);
    const size_t n = (size_t)B * d;
    const int col = wv * 16 + (lane & 15);
    // drift of the pair at (te, y): +-v [+ 1 * s], the sum the launch-per-step kernel forms
    auto drift = [&](const SmTile& y, float te) {
        SmTile f = sm_field(y, te, F, d, Ab0, Ab1, WlF, blF, wtF, wv, lane);
        SmTile sc;
        if (has_s) sc = sm_field(y, te, S, d, Ab0, Ab1, WlS, blS, wtS, wv, lane);
#pragma unroll
        for (int i = 0; i < SM_V; ++i) f.v[i] = srk_drift(reverse ? -f.v[i] : f.v[i], has_s ? sc.v[i] : 0.f, has_s, 1.0f);
        return f;
    };
    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        SmTile x;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            x.v[i] = (gr < B && col < d) ? y0[(size_t)gr * d + col] : 0.f;
        }
        __syncthreads();
        int oidx = 0;
        SmTile lr;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) lr.v[i] = 0.f;
        for (int k = 0; k < n_steps; ++k) {
            const SrkStep st = steps[k];
            static_assert(SM_V == 4, "ode_small_srk draws TWO Philox blocks of 4 normals per lane and step (xi1, xi2): with "
                                     "SM_MB > 1 elements i and i + 4 would share them (draw 2 SM_V / 4 blocks)");
            float z1[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f};
            if (xi) {
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const int gr = row0 + sm_row(i, lane);
                    if (gr < B && col < d) {
                        const size_t e = (size_t)gr * d + col;
                        z1[i] = xi[(size_t)(2 * k) * n + e];
                        z2[i] = xi[(size_t)(2 * k + 1) * n + e];
                    }
                }
            } else if (st.gs != 0.f) {
                const unsigned long long elem = (unsigned long long)(row0 / SM_ROWS) * 256 + tid;
                philox_normal4_w3(seed, (unsigned)k, elem, 0x5f2du, z1);
                philox_normal4_w3(seed, (unsigned)k, elem, 0x5f2eu, z2);
            }
            const SmTile k1 = drift(x, st.te1);
            SmTile ys;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) ys.v[i] = srk_stage2(x.v[i], k1.v[i], st.h);
            const SmTile k2 = drift(ys, st.te2);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) ys.v[i] = srk_stage3(x.v[i], k1.v[i], k2.v[i], st.h, st.c3, z1[i], z2[i]);
            const SmTile k3 = drift(ys, st.te3);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const int gr = row0 + sm_row(i, lane);
                const bool ok = gr < B && col < d;
                const float r = srk_final(x.v[i], k1.v[i], k2.v[i], k3.v[i], st.h, st.gs, z1[i]);
                x.v[i] = ok ? r : 0.f;
                if (st.is_out && ok) out[(size_t)oidx * n + (size_t)gr * d + col] = r;
            }
            if constexpr (LOGQP) {
                // the three stage drifts combined elementwise first: ONE row reduction per step
                SmTile q;
#pragma unroll
                for (int i = 0; i < SM_V; ++i) q.v[i] = fmaf(4.0f, k3.v[i] * k3.v[i], k1.v[i] * k1.v[i] + k2.v[i] * k2.v[i]);
                const float w = qw[k];
                const SmTile rs = sm_rowsum(q, red, wv, lane);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) lr.v[i] = fmaf(w, rs.v[i], lr.v[i]);
                if (st.is_out) sde_logqp_out(lr, logratio, oidx, row0, B, wv, lane);
            }
            oidx += st.is_out ? 1 : 0;
        }
        __syncthreads();
    }
}

// ---- entry points.  steps_host: n_steps Step records (host; EmStep: {te, h, g sqrt|h|, is_out}); ws: device scratch
// of >= sizeof(Step) n_steps bytes.  Ws == NULL: no score field.  Returns CFM_EINVAL for anything but two 4-layer fields
// of widths <= 64 with a time column (the caller then steps launch by launch).
// flags: SDE_REVERSE | SDE_LOGQP, any other bit CFM_EINVAL.  With SDE_LOGQP the n_steps records are followed by n_steps
// floats qw (one copy moves both into ws: (sizeof(Step) + 4) n_steps bytes) and out [n_out, B, d] by logratio [n_out, B],
// n_out counted from the records; without it every byte read and written is what it was before the flag existed.
template <auto KERNEL, auto KERNEL_LOGQP, class Step>
static int sde_small(const float* const* Wf, const float* const* bf, const float* const* Ws, const float* const* bs,
                     const int* dims, int n_layers, const float* y0, int B, const void* steps_host, int n_steps,
                     int flags, const float* xi, unsigned long long seed, float* out, void* ws, void* stream) {
    int d;
    if (!Wf || !bf || !y0 || !out || !steps_host || !ws || B < 0 || n_steps < 0) return CFM_EINVAL;
    if (flags & ~(SDE_REVERSE | SDE_LOGQP)) return CFM_EINVAL;
    if (small_envelope(dims, n_layers, &d)) return CFM_EINVAL;
    for (int l = 1; l <= 3; ++l) if (dims[l] < 1) return CFM_EINVAL;
    if (B == 0 || n_steps == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool logqp = (flags & SDE_LOGQP) != 0;
    const SmArgs F = small_args(Wf, bf, dims), S = small_args(Ws ? Ws : Wf, bs ? bs : bf, dims);
    const int grid = logqp ? small_grid<KERNEL_LOGQP, 160 * 1024>(B) : small_grid<KERNEL, 160 * 1024>(B);
    if (grid < 0) return CFM_EINVAL;
    const size_t rec_bytes = sizeof(Step) * (size_t)n_steps;
    int rc = cfm_hip(hipMemcpyAsync(ws, steps_host, rec_bytes + (logqp ? sizeof(float) * (size_t)n_steps : 0),
                                    hipMemcpyHostToDevice, s));
    if (rc) return rc;
    const int has_s = (Ws && bs) ? 1 : 0;
    if (logqp) {
        size_t n_out = 0;
        for (int k = 0; k < n_steps; ++k) n_out += ((const Step*)steps_host)[k].is_out ? 1 : 0;
        hipLaunchKernelGGL(KERNEL_LOGQP, dim3(grid), dim3(256), small_lds_bytes(2, 2, true), s, F, S, has_s, B, d,
                           (const Step*)ws, n_steps, flags, xi, seed, y0, out, (const float*)((const char*)ws + rec_bytes),
                           out + n_out * (size_t)B * d);
    } else {
        hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(256), small_lds_bytes(2, 2, false), s, F, S, has_s, B, d,
                           (const Step*)ws, n_steps, flags, xi, seed, y0, out, (const float*)nullptr, (float*)nullptr);
    }
    return cfm_status();
}

extern "C" int cfm_sde_em_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Ws,
                                  const float* const* bs, const int* dims, int n_layers, const float* y0, int B,
                                  const void* steps_host, int n_steps, int flags, const float* xi,
                                  unsigned long long seed, float* out, void* ws, void* stream) {
    return sde_small<ode_small_em<false>, ode_small_em<true>, EmStep>(Wf, bf, Ws, bs, dims, n_layers, y0, B, steps_host, n_steps,
                                                                      flags, xi, seed, out, ws, stream);
}

// as cfm_sde_em_mlp_f32, on SrkStep records; d >= 1 (the Euler-Maruyama entry accepts an empty state)
extern "C" int cfm_sde_srk_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Ws,
                                   const float* const* bs, const int* dims, int n_layers, const float* y0, int B,
                                   const void* steps_host, int n_steps, int flags, const float* xi,
                                   unsigned long long seed, float* out, void* ws, void* stream) {
    static_assert(sizeof(SrkStep) == 32, "the host packs 32-byte records");
    if (dims && n_layers == 4 && dims[4] < 1) return CFM_EINVAL;
    return sde_small<ode_small_srk<false>, ode_small_srk<true>, SrkStep>(Wf, bf, Ws, bs, dims, n_layers, y0, B, steps_host,
                                                                         n_steps, flags, xi, seed, out, ws, stream);
}
