// ode_grad.h — gradient of the fixed-step solves of ode_small_fixed<SCHEME, AUG_NONE> (euler, midpoint, rk4) with respect
// to the field's parameters and the initial state (included by small_grad.hip after cnf_grad.h, whose
// cg_stage_transposed and cg_store_partial it runs on; the host tail is small_grad.hip's, the tile engine with cg_put,
// cg_outer and cg_sum4 small_field.h's, the reverse step ode_reverse.h's: one text for this kernel and ode_small_adaptive_grad).
//
// Forward, per step n with h = tspan[n + 1] - tspan[n]:  Y_1 = y_n,  Y_s = fmaf(h, sum_{q<s} a_sq k_q, y_n),
// k_s = f(t_n + c_s h, Y_s),  y_{n+1} = fmaf(h, sum_s b_s k_s, y_n).  Given G = dL/d traj [n_t, B, d]:  lam_N = G[N], and for
// n = N-1 .. 0, s = NS .. 1:
//   kb_s = h (b_s lam_{n+1} + sum_{r>s} a_rs Yb_r)        Yb_s = kb_s^T df/dy (t_n + c_s h, Y_s)        theta_bar += kb_s^T df/dtheta
//   lam_n = lam_{n+1} + sum_s Yb_s + G[n]                 g_initial = lam_0
// the gradient of the recurrence the forward ran (discretise-then-optimise).
//
// One reverse step on a 16-row tile:
//   stages forward from y_n (read from the saved trajectory) in the arithmetic of sm_field and the stage combination of
//   ode_small_fixed: the same fmaf chains, (float)fx_a / fx_c constants and stage times, so every pre-activation has the
//   forward's bits and sits on the forward's side of every SELU kink.  s_l = selu'(z_l), h_l and Y_s of every stage stay
//   in registers (7 tiles per stage); the last stage's last layer is never evaluated (no Y depends on k_NS), the other
//   stages' exactly once.
//   stages backward, one vector-Jacobian product each (the primal reverse of ode_small_euler_grad with sb_l = 0):
//     dW_3 += kb^T h_3, db_3 += kb, hb_3 = kb W_3;  for l = 3..1: zb_l = hb_l * s_l, dW_{l-1} += zb_l^T h_{l-1},
//     db_{l-1} += zb_l, hb_{l-1} = zb_l W_{l-1};  Yb = hb_0[:, :d];  the time column of W_0 gets (t_n + c_s h) sum zb_1.
// Products with W_l^T run through sm_gemm on transposed copies of the two 64 x 64 layers and through cg_gemm_t for the two
// thin ones; weight gradients are MFMA accumulators (cg_outer) kept over all stages, steps and tiles of the workgroup.
// Every workgroup writes one partial gradient, ode_small_grad_reduce adds them in workgroup order: the same bits run to
// run.  Rows are independent: no cross-workgroup wait of any kind.
//
// LDS buffers: a buffer written in a phase is not read in it, and a barrier ends every phase.  The forward alternates
// (P0, P1) as sm_field does; a vector-Jacobian product has four phases that write (Q0, Q1), (P0, P1), (Q0, Q1), (P0, P1) and
// read what they wrote after the phase's barrier, so the first of them never touches what the forward's last layer still
// reads, and one barrier at the end of the step separates the last phase's reads of (P0, P1) from the next step's y_n.
#pragma once

#include "ode_reverse.h"

// the layout of cfm_cnf_grad_ws_bytes_internal: the device copy of t_span, then one partial gradient per workgroup
extern "C" size_t cfm_ode_grad_ws_bytes_internal(int B, int n_t) { return cfm_cnf_grad_ws_bytes_internal(B, n_t); }

// traj [n_t, B, d]: the forward solve (y_n is read); G [n_t, B, d]; g0 [B, d] or null; part [gridDim.x][P] as in
// ode_small_euler_grad
template <int SCHEME>
__global__ __launch_bounds__(256) void ode_small_fixed_grad(SmArgs A, int B, int d, const float* __restrict__ tspan, int n_t,
                                                         const float* __restrict__ traj, const float* __restrict__ G,
                                                         float* __restrict__ g0, float* __restrict__ part, int P) {
    using T = FxCoef<SCHEME>;
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const OgLds L = og_prologue(A, d, small_lds, tid);
    const size_t n = (size_t)B * d;
    const int col = wv * 16 + (lane & 15);

    f32x4 dWa[4][4];
    float dba[4], dwt = 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        dba[l] = 0.f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) dWa[l][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        const int nrows = B - row0;
        SmTile lam, yn, gn;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            const bool ok = gr < B && col < d;
            lam.v[i] = ok ? G[(size_t)(n_t - 1) * n + (size_t)gr * d + col] : 0.f;
            yn.v[i] = (ok && n_t >= 2) ? traj[(size_t)(n_t - 2) * n + (size_t)gr * d + col] : 0.f;
            gn.v[i] = (ok && n_t >= 2) ? G[(size_t)(n_t - 2) * n + (size_t)gr * d + col] : 0.f;
        }
        __syncthreads();
        for (int st = n_t - 2; st >= 0; --st) {
            const float t = tspan[st], h = tspan[st + 1] - tspan[st];
            const SmTile y = yn, g = gn;
            if (st > 0) {                                  // y_{n-1} and G[n-1] travel while this step runs
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const int gr = row0 + sm_row(i, lane);
                    const bool ok = gr < B && col < d;
                    yn.v[i] = ok ? traj[(size_t)(st - 1) * n + (size_t)gr * d + col] : 0.f;
                    gn.v[i] = ok ? G[(size_t)(st - 1) * n + (size_t)gr * d + col] : 0.f;
                }
            }

            float tsg[T::NS];
            tsg[0] = t;
#pragma unroll
            for (int sg = 1; sg < T::NS; ++sg) tsg[sg] = t + (float)fx_c<SCHEME>(sg - 1) * h;
            og_reverse_step<T>(A, L, nrows, wv, lane, col, y, lam, h, tsg, dWa, dba, dwt);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) lam.v[i] = lam.v[i] + g.v[i];
        }
        if (g0) {
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const int gr = row0 + sm_row(i, lane);
                if (gr < B && col < d) g0[(size_t)gr * d + col] = lam.v[i];
            }
        }
    }
    cg_store_partial(A, d, part + (size_t)blockIdx.x * P, dWa, dba, dwt, lane, col);
}

template <int SCHEME>
static int ode_grad_launch(const SmArgs& A, int B, int d, const float* tspan_dev, int n_t, const float* traj, const float* G,
                           float* g0, float* part, int P, const CgOut& O, hipStream_t s) {
    return cg_launch<ode_small_fixed_grad<SCHEME>, 128 * 1024>(og_lds_bytes, s, B, part, P, A, O, 1.f, nullptr, A, B, d, tspan_dev,
                                                               n_t, traj, G, g0, part, P);
}

// the envelope of the gradient of the fixed-step solves: the small-field kernels (every width >= 1, d + 1 <= SM_W), fused
// path on.  No GPU work: the host asks before the forward, since an autograd backward cannot fall back.
extern "C" int cfm_ode_fixed_grad_available(const int* dims, int n_layers) {
    int d;
    if (small_envelope(dims, n_layers, &d)) return CFM_EINVAL;
    for (int l = 1; l <= 3; ++l) if (dims[l] < 1) return CFM_EINVAL;
    return (d < 1 || d + 1 > SM_W || !cfm_ode_fused_internal()) ? CFM_EINVAL : 0;
}

extern "C" int cfm_ode_fixed_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                      const float* traj, int B, const float* t_span, int n_t, int scheme,
                                      const float* g_traj, float* const* dW, float* const* db, float* g_initial, void* ws,
                                      void* stream) {
    if (!W || !b || !traj || !t_span || !g_traj || !dW || !db || !ws || B <= 0 || n_t < 1 || !fx_known(scheme)) return CFM_EINVAL;
    int rc = cfm_ode_fixed_grad_available(dims, n_layers);
    if (rc) return rc;
    const int d = dims[4];
    const SmArgs A = small_args(W, b, dims);
    CgOut O;
    const int P = cg_out(dims, dW, db, &O);
    if (P < 0) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const CgWs w = cg_carve(ws, n_t);
    rc = cfm_hip(hipMemcpyAsync(w.tspan, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    if (scheme == CFM_ODE_RK4) return ode_grad_launch<CFM_ODE_RK4>(A, B, d, w.tspan, n_t, traj, g_traj, g_initial, w.part, P, O, s);
    if (scheme == CFM_ODE_MIDPOINT) return ode_grad_launch<CFM_ODE_MIDPOINT>(A, B, d, w.tspan, n_t, traj, g_traj, g_initial, w.part, P, O, s);
    return ode_grad_launch<CFM_ODE_EULER>(A, B, d, w.tspan, n_t, traj, g_traj, g_initial, w.part, P, O, s);
}
