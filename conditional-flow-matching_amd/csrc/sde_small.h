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

__global__ __launch_bounds__(256) void ode_small_em(SmArgs F, SmArgs S, int has_s, int B, int d,
                                                    const EmStep* __restrict__ steps, int n_steps, int reverse,
                                                    const float* __restrict__ xi, unsigned long long seed,
                                                    const float* __restrict__ y0, float* __restrict__ out) {
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
                float r = fmaf(st.h, f, x.v[i]);
                const float noise = xi ? (ok ? xi[(size_t)k * n + (size_t)gr * d + col] : 0.f) : z[i & 3];
                r = fmaf(st.gs, noise, r);
                x.v[i] = ok ? r : 0.f;
                if (st.is_out && ok) out[(size_t)oidx * n + (size_t)gr * d + col] = r;
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
__global__ __launch_bounds__(256) void ode_small_srk(SmArgs F, SmArgs S, int has_s, int B, int d,
                                                     const SrkStep* __restrict__ steps, int n_steps, int reverse,
                                                     const float* __restrict__ xi, unsigned long long seed,
                                                     const float* __restrict__ y0, float* __restrict__ out) {
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
            oidx += st.is_out ? 1 : 0;
        }
        __syncthreads();
    }
}

// ---- entry points.  steps_host: n_steps Step records (host; EmStep: {te, h, g sqrt|h|, is_out}); ws: device scratch
// of >= sizeof(Step) n_steps bytes.  Ws == NULL: no score field.  Returns CFM_EINVAL for anything but two 4-layer fields
// of widths <= 64 with a time column (the caller then steps launch by launch).
template <auto KERNEL, class Step>
static int sde_small(const float* const* Wf, const float* const* bf, const float* const* Ws, const float* const* bs,
                     const int* dims, int n_layers, const float* y0, int B, const void* steps_host, int n_steps,
                     int reverse, const float* xi, unsigned long long seed, float* out, void* ws, void* stream) {
    int d;
    if (!Wf || !bf || !y0 || !out || !steps_host || !ws || B < 0 || n_steps < 0) return CFM_EINVAL;
    if (small_envelope(dims, n_layers, &d)) return CFM_EINVAL;
    for (int l = 1; l <= 3; ++l) if (dims[l] < 1) return CFM_EINVAL;
    if (B == 0 || n_steps == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const SmArgs F = small_args(Wf, bf, dims), S = small_args(Ws ? Ws : Wf, bs ? bs : bf, dims);
    const int grid = small_grid<KERNEL, 160 * 1024>(B);
    if (grid < 0) return CFM_EINVAL;
    int rc = cfm_hip(hipMemcpyAsync(ws, steps_host, sizeof(Step) * (size_t)n_steps, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(256), small_lds_bytes(2, 2, false), s, F, S, (Ws && bs) ? 1 : 0, B, d,
                       (const Step*)ws, n_steps, reverse, xi, seed, y0, out);
    return cfm_status();
}

extern "C" int cfm_sde_em_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Ws,
                                  const float* const* bs, const int* dims, int n_layers, const float* y0, int B,
                                  const void* steps_host, int n_steps, int reverse, const float* xi,
                                  unsigned long long seed, float* out, void* ws, void* stream) {
    return sde_small<ode_small_em, EmStep>(Wf, bf, Ws, bs, dims, n_layers, y0, B, steps_host, n_steps, reverse, xi, seed, out,
                                           ws, stream);
}

// as cfm_sde_em_mlp_f32, on SrkStep records; d >= 1 (the Euler-Maruyama entry accepts an empty state)
extern "C" int cfm_sde_srk_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Ws,
                                   const float* const* bs, const int* dims, int n_layers, const float* y0, int B,
                                   const void* steps_host, int n_steps, int reverse, const float* xi,
                                   unsigned long long seed, float* out, void* ws, void* stream) {
    static_assert(sizeof(SrkStep) == 32, "the host packs 32-byte records");
    if (dims && n_layers == 4 && dims[4] < 1) return CFM_EINVAL;
    return sde_small<ode_small_srk, SrkStep>(Wf, bf, Ws, bs, dims, n_layers, y0, B, steps_host, n_steps, reverse, xi, seed,
                                             out, ws, stream);
}
