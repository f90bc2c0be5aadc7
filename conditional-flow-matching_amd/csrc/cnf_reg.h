// cnf_reg.h — the C entry of the regularised CNF solve (RNODE / TrajectoryNet) (included by ode.hip: the CFM_OP_ODE
// workspace and the prelude of the one-launch fixed-step entries, ode_fixed_onelaunch, live there; the envelope checks
// cnf_check and cnf_reg_check come from ode_envelope.h).  The forward kernel is a
// translation unit of its own, cnf_reg.hip, which says what the solve computes: the small-field kernels of ode.hip are
// compiled exactly as they were before it existed.  The gradient entry cfm_cnf_reg_euler_grad_f32 sits
// with its kernel ode_small_euler_grad<MODE, REG> in cnf_grad.h (small_grad.hip).
#pragma once

// cnf_reg.hip: the solve, one launch (mode 0 exact / 1 Hutchinson / 2 no trace; reg_mask checked by the caller)
extern "C" int cfm_cnf_reg_solve_internal(const SmArgs* A, int B, int d, const float* t_span, int n_t, float* traj,
                                          float* tspan_dev, const float* eps, float* jsq, int mode, int reg_mask,
                                          hipStream_t s);

extern "C" int cfm_ode_euler_cnf_reg_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                             const float* x0, int B, const float* t_span, int n_t, int mode,
                                             const float* eps, int reg_mask, float* traj, float* jac_sq, int* nfe, void* ws,
                                             void* stream) {
    SmArgs A;
    if (cnf_reg_check(mode, reg_mask, jac_sq)) return CFM_EINVAL;
    // Euler: one evaluation per step; the state is [(l), (L1), (L2), (e), (f), y]
    return ode_fixed_onelaunch(x0, B, t_span, n_t, traj, nfe, 1, cg_aug_cols(mode, reg_mask), dims, n_layers, ws, stream,
        [&](int* d) { return cnf_check(W, b, dims, n_layers, B, mode, eps, d, &A, CFM_TRACE_NONE); },
        [&](int d, float* tspan_dev, hipStream_t s) {
            return cfm_cnf_reg_solve_internal(&A, B, d, t_span, n_t, traj, tspan_dev, eps, jac_sq, mode, reg_mask, s);
        });
}
