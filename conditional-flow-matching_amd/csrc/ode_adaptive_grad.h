// ode_adaptive_grad.h — gradient of the adaptive solves (dopri5, tsit5) of ode_small_dopri<TAB, ., AUG_NONE, FIELD_MLP, true>
// with respect to the field's parameters and the initial state (included by small_grad.hip after ode_grad.h; it runs on the
// helpers of cnf_grad.h and on the reverse step of ode_reverse.h as ode_grad.h does, and on the tile engine of small_field.h).
//
// The accepted step sequence is a constant of the gradient (discretise-then-optimise): rejected attempts
// contribute nothing, and the controller's scalars are not differentiated.  Row 6 of a is b and the seventh slope feeds
// only the error estimate and the next step's k_1 (FSAL), so an accepted step n with record {t, dt, t_k1, out} is a 6-stage
// explicit Runge-Kutta step with weights b = a[5], with hdt = tsign dt:
//   Y_1 = y_n, k_1 = f(tsign t_k1, Y_1);  Y_s = fmaf(hdt, sum_{q<s} a_{s-1,q} k_q, y_n), k_s = f(tsign (t + c_{s-1} dt), Y_s);
//   y_{n+1} = fmaf(hdt, sum_s a_{5,s} k_s, y_n);  traj[out] = y_{n+1} when out >= 0.
// Given G = dL/d traj [n_t, B, d]:  lam = 0, and for n = n_accepted - 1 .. 0:  lam += G[out] (out >= 0), then for s = 6 .. 1
//   kb_s = hdt (b_s lam + sum_{r>s} a_rs Yb_r)     Yb_s = kb_s^T df/dy (stage time, Y_s)     theta_bar += kb_s^T df/dtheta
//   lam <- lam + sum_s Yb_s;                        g_initial = lam + G[0]
// the recurrence of ode_grad.h's header with a step that varies.  The time column of W_0 gets (stage time) sum zb_1, the
// stage time being the field's argument, tsign included.
//
// One reverse step on a 16-row tile is that of ode_small_fixed_grad with six stages: the stages forward from y_n (read from
// ysteps[n]) in the arithmetic of sm_field and of SM_COMBINE (the same fmaf chains, (float)rk_a<TAB> constants, hdt and
// stage times, k_1 at tsign t_k1), so every pre-activation has the forward's bits; s_l, h_l and Y_s of all six stages stay
// in registers (7 tiles per stage: the kernel runs one wave per SIMD and has the 512 registers of a lane to itself);
// then one vector-Jacobian product per stage.  LDS buffers and barriers: as ode_grad.h describes them.
// Every workgroup writes one partial gradient, ode_small_grad_reduce adds them in workgroup order: the same bits run to
// run.  Rows are independent: no cross-workgroup wait of any kind.
#pragma once

// log [n_acc], ysteps [n_acc, B, d]: the recording solve's; G [n_t, B, d]; g0 [B, d] or null; part [gridDim.x][P]
template <int TAB>
__global__ __launch_bounds__(256) void ode_small_adaptive_grad(SmArgs A, int B, int d, const OdeStepRec* __restrict__ log,
                                                            int n_acc, const float* __restrict__ ysteps, float tsign,
                                                            const float* __restrict__ G, int n_t, float* __restrict__ g0,
                                                            float* __restrict__ part, int P) {
    using T = RkCoef<TAB>;
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
        OdeStepRec rn = OdeStepRec{0.f, 0.f, 0.f, -1};
        if (n_acc > 0) rn = log[n_acc - 1];
        bool gok = rn.out >= 0 && rn.out < n_t;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            const bool ok = gr < B && col < d;
            lam.v[i] = 0.f;
            yn.v[i] = (ok && n_acc > 0) ? ysteps[(size_t)(n_acc - 1) * n + (size_t)gr * d + col] : 0.f;
            gn.v[i] = (ok && gok) ? G[(size_t)rn.out * n + (size_t)gr * d + col] : 0.f;
        }
        __syncthreads();
        for (int st = n_acc - 1; st >= 0; --st) {
            const OdeStepRec r = rn;
            const float hdt = tsign * r.dt;
            const SmTile y = yn;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) lam.v[i] += gn.v[i];          // lam_{n+1}: the step end is traj[out]
            if (st > 0) {                                  // the record, y_{n-1} and its G travel while this step runs
                rn = log[st - 1];
                gok = rn.out >= 0 && rn.out < n_t;
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const int gr = row0 + sm_row(i, lane);
                    const bool ok = gr < B && col < d;
                    yn.v[i] = ok ? ysteps[(size_t)(st - 1) * n + (size_t)gr * d + col] : 0.f;
                    gn.v[i] = (ok && gok) ? G[(size_t)rn.out * n + (size_t)gr * d + col] : 0.f;
                }
            }

            float tsg[T::NS];
            tsg[0] = tsign * r.t_k1;                       // k_1 is the previous step's k_7 (FSAL): evaluated there
#pragma unroll
            for (int sg = 1; sg < T::NS; ++sg) tsg[sg] = tsign * (r.t + rk_c<TAB>(sg - 1) * r.dt);
            og_reverse_step<T>(A, L, nrows, wv, lane, col, y, lam, hdt, tsg, dWa, dba, dwt);
        }
        if (g0) {
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const int gr = row0 + sm_row(i, lane);
                if (gr < B && col < d) g0[(size_t)gr * d + col] = lam.v[i] + G[(size_t)gr * d + col];
            }
        }
    }
    cg_store_partial(A, d, part + (size_t)blockIdx.x * P, dWa, dba, dwt, lane, col);
}

template <int TAB>
static int ode_adaptive_grad_launch(const SmArgs& A, int B, int d, const OdeStepRec* log, int n_acc, const float* ysteps,
                                    float tsign, const float* G, int n_t, float* g0, float* part, int P, const CgOut& O,
                                    hipStream_t s) {
    return cg_launch<ode_small_adaptive_grad<TAB>, 128 * 1024>(og_lds_bytes, s, B, part, P, A, O, 1.f, nullptr, A, B, d, log, n_acc,
                                                               ysteps, tsign, G, n_t, g0, part, P);
}

// the envelope of the gradient of the adaptive solves: that of the fixed-step gradient.  No GPU work.
extern "C" int cfm_ode_adaptive_grad_available(const int* dims, int n_layers) { return cfm_ode_fixed_grad_available(dims, n_layers); }

extern "C" int cfm_ode_adaptive_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                         const float* ysteps, const void* log, int n_accepted, int B, int n_t, int tableau,
                                         float tsign, const float* g_traj, float* const* dW, float* const* db,
                                         float* g_initial, void* ws, void* stream) {
    if (!W || !b || !ysteps || !log || !g_traj || !dW || !db || !ws || B <= 0 || n_t < 2 || n_accepted < 1 ||
        !rk_adaptive_known(tableau) || !(tsign == 1.f || tsign == -1.f))
        return CFM_EINVAL;
    int rc = cfm_ode_adaptive_grad_available(dims, n_layers);
    if (rc) return rc;
    const int d = dims[4];
    const SmArgs A = small_args(W, b, dims);
    CgOut O;
    const int P = cg_out(dims, dW, db, &O);
    if (P < 0) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float* part = cg_carve(ws, n_t).part;          // the t_span area is not used: the log carries the times
    const OdeStepRec* lg = (const OdeStepRec*)log;
    if (tableau == CFM_ODE_TSIT5)
        return ode_adaptive_grad_launch<CFM_ODE_TSIT5>(A, B, d, lg, n_accepted, ysteps, tsign, g_traj, n_t, g_initial, part, P, O, s);
    return ode_adaptive_grad_launch<CFM_ODE_DOPRI5>(A, B, d, lg, n_accepted, ysteps, tsign, g_traj, n_t, g_initial, part, P, O, s);
}
