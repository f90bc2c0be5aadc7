// ode_grad.h — gradient of the fixed-step solves of ode_small_fixed<SCHEME, AUG_NONE> (euler, midpoint, rk4) with respect
// to the field's parameters and the initial state (included by ode.hip after cnf_grad.h, whose cg_put, cg_outer, cg_sum4,
// cg_stage_transposed, cg_store_partial, CgOut, CG_MAXGRID, CG_PMAX and ode_small_grad_reduce it runs on; the tile engine is small_field.h's).
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

// one staged net, the transposed copies of its two 64 x 64 layers, four tile buffers
constexpr size_t og_lds_bytes = small_lds_bytes(1, 4, false) + sizeof(float) * 2 * SM_W * SM_LD;
static_assert(og_lds_bytes == 123136 && og_lds_bytes <= cg_lds_bytes, "the ODE gradient kernel");

// the layout of cfm_cnf_grad_ws_bytes_internal: the device copy of t_span, then one partial gradient per workgroup
extern "C" size_t cfm_ode_grad_ws_bytes_internal(int B, int n_t) { return cfm_cnf_grad_ws_bytes_internal(B, n_t); }

// traj [n_t, B, d]: the forward solve (y_n is read); G [n_t, B, d]; g0 [B, d] or null; part [gridDim.x][P] as in
// ode_small_euler_grad
template <int SCHEME>
__global__ __launch_bounds__(256) void ode_small_fixed_grad(SmArgs A, int B, int d, const float* __restrict__ tspan, int n_t,
                                                         const float* __restrict__ traj, const float* __restrict__ G,
                                                         float* __restrict__ g0, float* __restrict__ part, int P) {
    constexpr int NS = fx_stages<SCHEME>();
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    constexpr int TS = SM_ROWS * SM_LD, WS = SM_W * SM_LD;
    float* Wl = small_lds;
    float* WT = Wl + 4 * WS;                  // W1^T, W2^T
    float* bl = WT + 2 * WS;
    float* wt = bl + 4 * SM_W;
    float* P0 = wt + SM_W;
    float* P1 = P0 + TS;
    float* Q0 = P1 + TS;
    float* Q1 = Q0 + TS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    sm_stage_weights(A, d, Wl, bl, wt, tid);
    cg_stage_transposed(A, WT, tid);
    const size_t n = (size_t)B * d;
    const int col = wv * 16 + (lane & 15);
    const float* W1T = WT;
    const float* W2T = WT + WS;
    const float* W3 = Wl + 3 * WS;

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

            // ---- the stages forward: s_l, h_l, Y_s (the arithmetic of sm_field and of ode_small_fixed) ----
            SmTile s[NS][3], hh[NS][3], Y[NS], f[NS];
            float tsg[NS];
            f32x4 c[SM_MB];
#pragma unroll
            for (int sg = 0; sg < NS; ++sg) {
                Y[sg] = y;
                tsg[sg] = t;
                if (sg > 0) {
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        float acc = (float)fx_a<SCHEME>(sg - 1, 0) * f[0].v[i];
#pragma unroll
                        for (int q = 1; q < NS - 1; ++q)
                            if (q < sg) acc = fmaf((float)fx_a<SCHEME>(sg - 1, q), f[q].v[i], acc);
                        Y[sg].v[i] = fmaf(h, acc, y.v[i]);
                    }
                    tsg[sg] = t + (float)fx_c<SCHEME>(sg - 1) * h;
                }
                cg_put(P0, Y[sg], lane, col);
                sm_lds_barrier();
                float* src = P0; float* dst = P1;
#pragma unroll
                for (int l = 0; l < (sg < NS - 1 ? 4 : 3); ++l) {          // no Y depends on the last stage's slope
                    const int N = A.dims[l + 1];
                    sm_gemm(src, Wl + l * WS, wv, lane, c);
                    const float bv = (col < N) ? bl[l * SM_W + col] : 0.f;
                    const float wtc = (l == 0 && col < N) ? wt[col] : 0.f;
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        float z = c[0][i] + bv;
                        if (l == 0) z = fmaf(tsg[sg], wtc, z);
                        if (l < 3) {
                            s[sg][l].v[i] = (col < N && sm_row(i, lane) < nrows) ? selu_slope(z) : 0.f;
                            hh[sg][l].v[i] = (col < N) ? selu_f(z) : 0.f;
                        } else {
                            f[sg].v[i] = (col < N) ? z : 0.f;
                        }
                    }
                    if (l < 2 || (l == 2 && sg < NS - 1)) {
                        cg_put(dst, hh[sg][l], lane, col);
                        sm_lds_barrier();
                        float* tmp = src; src = dst; dst = tmp;
                    }
                }
            }

            // ---- the stages backward: one vector-Jacobian product each ----
            SmTile Yb[NS], lamn = lam;
#pragma unroll
            for (int sg = NS - 1; sg >= 0; --sg) {
                SmTile kb, zb;
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    float acc = (float)fx_b<SCHEME>(sg) * lam.v[i];
#pragma unroll
                    for (int r = sg + 1; r < NS; ++r) acc = fmaf((float)fx_a<SCHEME>(r - 1, sg), Yb[r].v[i], acc);
                    kb.v[i] = h * acc;
                }
                cg_put(Q0, kb, lane, col);
                cg_put(Q1, hh[sg][2], lane, col);
                sm_lds_barrier();
                dba[3] += cg_sum4(kb);
                cg_outer(Q0, Q1, wv, lane, dWa[3]);
                cg_gemm_t(Q0, W3, wv, lane, c[0]);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[sg][2].v[i];
                dba[2] += cg_sum4(zb);
                cg_put(P0, zb, lane, col);
                cg_put(P1, hh[sg][1], lane, col);
                sm_lds_barrier();
                cg_outer(P0, P1, wv, lane, dWa[2]);
                sm_gemm(P0, W2T, wv, lane, c);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[sg][1].v[i];
                dba[1] += cg_sum4(zb);
                cg_put(Q0, zb, lane, col);
                cg_put(Q1, hh[sg][0], lane, col);
                sm_lds_barrier();
                cg_outer(Q0, Q1, wv, lane, dWa[1]);
                sm_gemm(Q0, W1T, wv, lane, c);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[sg][0].v[i];
                {
                    const float zs = cg_sum4(zb);
                    dba[0] += zs;
                    dwt = fmaf(tsg[sg], zs, dwt);
                }
                cg_put(P0, zb, lane, col);
                cg_put(P1, Y[sg], lane, col);
                sm_lds_barrier();
                cg_outer(P0, P1, wv, lane, dWa[0]);
                cg_gemm_t(P0, Wl, wv, lane, c[0]);                                          // zb1 W0[:, :d]
#pragma unroll
                for (int i = 0; i < SM_V; ++i) { Yb[sg].v[i] = c[0][i]; lamn.v[i] += c[0][i]; }
            }
#pragma unroll
            for (int i = 0; i < SM_V; ++i) lam.v[i] = lamn.v[i] + g.v[i];
            sm_lds_barrier();       // the last product read (P0, P1): the next step writes y_n there first
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
    const int grid = small_grid<ode_small_fixed_grad<SCHEME>, 128 * 1024>(B, CG_MAXGRID);
    if (grid < 0) return CFM_EINVAL;
    hipLaunchKernelGGL(ode_small_fixed_grad<SCHEME>, dim3(grid), dim3(256), og_lds_bytes, s, A, B, d, tspan_dev, n_t, traj, G, g0,
                       part, P);
    int rc = cfm_status();
    if (rc) return rc;
    hipLaunchKernelGGL(ode_small_grad_reduce, dim3((P + 255) / 256), dim3(256), 0, s, (const float*)part, grid, P, A, O, 1.f, nullptr);
    return cfm_status();
}

// the envelope of the gradient of the fixed-step solves: the small-field kernels (every width >= 1, d + 1 <= SM_W), fused
// path on.  No GPU work: the host asks before the forward, since an autograd backward cannot fall back.
extern "C" int cfm_ode_fixed_grad_available(const int* dims, int n_layers) {
    int d;
    if (small_envelope(dims, n_layers, &d)) return CFM_EINVAL;
    for (int l = 1; l <= 3; ++l) if (dims[l] < 1) return CFM_EINVAL;
    return (d < 1 || d + 1 > SM_W || !ode_small_enabled()) ? CFM_EINVAL : 0;
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
    int P = 0;
    for (int l = 0; l < 4; ++l) {
        if (!dW[l] || !db[l]) return CFM_EINVAL;
        O.dW[l] = dW[l]; O.db[l] = db[l];
        P += dims[l + 1] * (dims[l] + 1);
    }
    hipStream_t s = (hipStream_t)stream;
    float* tspan_dev = (float*)ws;
    float* part = (float*)((char*)ws + cfm_align_up(sizeof(float) * (size_t)n_t, 256));
    rc = cfm_hip(hipMemcpyAsync(tspan_dev, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    if (scheme == CFM_ODE_RK4) return ode_grad_launch<CFM_ODE_RK4>(A, B, d, tspan_dev, n_t, traj, g_traj, g_initial, part, P, O, s);
    if (scheme == CFM_ODE_MIDPOINT) return ode_grad_launch<CFM_ODE_MIDPOINT>(A, B, d, tspan_dev, n_t, traj, g_traj, g_initial, part, P, O, s);
    return ode_grad_launch<CFM_ODE_EULER>(A, B, d, tspan_dev, n_t, traj, g_traj, g_initial, part, P, O, s);
}
