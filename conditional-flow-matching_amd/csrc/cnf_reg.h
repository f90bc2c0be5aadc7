// cnf_reg.h — the C entries of the regularised CNF solve (RNODE / TrajectoryNet) and of its gradient (included by ode.hip
// behind cnf_grad.h: the envelope check, the CFM_OP_ODE workspace and the backward kernel ode_small_euler_grad<MODE, REG>
// live there).  The forward kernel is a translation unit of its own, cnf_reg.hip, which says what the solve computes: the
// small-field kernels of ode.hip are compiled exactly as they were before it existed.
#pragma once

// cnf_reg.hip: the solve, one launch (mode 0 exact / 1 Hutchinson; reg_mask checked by the caller)
extern "C" int cfm_cnf_reg_solve_internal(const SmArgs* A, int B, int d, const float* t_span, int n_t, float* traj,
                                          float* tspan_dev, const float* eps, float* jsq, int mode, int reg_mask,
                                          hipStream_t s);

// reg_mask of the two entries: bit 0 squared_L2, bit 1 jacobian_frobenius; at least one; the Jacobian penalty with the
// exact trace only (mode 0) and with its side buffer
static int cnf_reg_check(int mode, int reg_mask, const float* jac_sq) {
    if (reg_mask < 1 || reg_mask > 3) return CFM_EINVAL;
    if ((reg_mask & 2) && (mode != 0 || !jac_sq)) return CFM_EINVAL;
    return 0;
}

extern "C" int cfm_ode_euler_cnf_reg_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                             const float* x0, int B, const float* t_span, int n_t, int mode,
                                             const float* eps, int reg_mask, float* traj, float* jac_sq, int* nfe, void* ws,
                                             void* stream) {
    int d; SmArgs A;
    if (!x0 || !t_span || !traj || !ws || n_t < 1 || cnf_reg_check(mode, reg_mask, jac_sq)) return CFM_EINVAL;
    int rc = cnf_check(W, b, dims, n_layers, B, mode, eps, &d, &A);
    if (rc) return rc;
    if (!fx_monotone(t_span, n_t)) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int D = d + 1 + cg_reg_cols(reg_mask);
    OdeWs w = ode_carve(ws, B, maxwidth(dims, n_layers), D);       // workspace of CFM_OP_ODE at D
    const size_t n = (size_t)B * D;
    if ((size_t)n_t > 3 * n) return CFM_EINVAL;                    // t_span copy: w.x .. w.xt
    rc = cfm_hip(hipMemcpyAsync(traj, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (rc) return rc;
    if (nfe) *nfe = n_t - 1;
    if (n_t < 2) return 0;
    return cfm_cnf_reg_solve_internal(&A, B, d, t_span, n_t, traj, w.x, eps, jac_sq, mode, reg_mask, s);
}

extern "C" int cfm_cnf_reg_euler_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                          const float* traj, int B, const float* t_span, int n_t, int mode, const float* eps,
                                          int reg_mask, const float* jac_sq, const float* g_final, float* const* dW,
                                          float* const* db, float* g_initial, void* ws, void* stream) {
    int d; SmArgs A;
    if (!traj || !t_span || !g_final || !dW || !db || !ws || n_t < 1 || cnf_reg_check(mode, reg_mask, jac_sq)) return CFM_EINVAL;
    int rc = cnf_check(W, b, dims, n_layers, B, mode, eps, &d, &A);
    if (rc) return rc;
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
    if (mode == 1) return cnf_grad_launch<AUG_HUTCH, 1>(A, B, d, tspan_dev, n_t, traj, eps, g_final, g_initial, part, P, O, s, jac_sq);
    if (reg_mask == 1) return cnf_grad_launch<AUG_EXACT, 1>(A, B, d, tspan_dev, n_t, traj, eps, g_final, g_initial, part, P, O, s, jac_sq);
    if (reg_mask == 2) return cnf_grad_launch<AUG_EXACT, 2>(A, B, d, tspan_dev, n_t, traj, eps, g_final, g_initial, part, P, O, s, jac_sq);
    return cnf_grad_launch<AUG_EXACT, 3>(A, B, d, tspan_dev, n_t, traj, eps, g_final, g_initial, part, P, O, s, jac_sq);
}
