// ode_envelope.h — what the forward solvers (ode.hip) and their gradient kernels (small_grad.hip) both see besides the
// tile engine and the tableaus: the envelope checks of the small-field entries, the regulariser columns of the CNF state
// and the step record of the recording solve.  Pure functions over small_field.h's small_envelope plus the fused-path
// switch, whose state is ode.hip's.
#pragma once

// ode.hip: the fused-path switch (cfm_ode_set_fused, else CFM_ODE_FUSED=0 in the environment disables)
extern "C" int cfm_ode_fused_internal();

// The record of an accepted step that the recording solve keeps (cfm_ode_adaptive_rec_mlp_f32) and its gradient replays
// (ode_adaptive_grad.h): solver-space t and dt of the stages, the time k_1 was evaluated at (FSAL: the previous step's
// last stage time, which is not t in general after a landing step), the t_span index the step end lands on or -1.
struct OdeStepRec { float t, dt, t_k1; int out; };
static_assert(sizeof(OdeStepRec) == 16, "the step log's record");

// the envelope of the CNF entries: the small-field kernels (small_envelope, every width >= 1, d + 1 <= SM_W), fused path
// on, mode 0 (exact trace) or 1 (Hutchinson, eps given); max_mode 2 lets the regularised solve's "no trace" through
static inline int cnf_check(const float* const* W, const float* const* b, const int* dims, int n_layers, int B, int mode,
                            const float* eps, int* d_out, SmArgs* A, int max_mode = 1) {
    int d;
    if (!W || !b || B <= 0 || mode < 0 || mode > max_mode || (mode == 1 && !eps)) return CFM_EINVAL;
    if (small_envelope(dims, n_layers, &d)) return CFM_EINVAL;
    for (int l = 1; l <= 3; ++l) if (dims[l] < 1) return CFM_EINVAL;
    if (d < 1 || d + 1 > SM_W || !cfm_ode_fused_internal()) return CFM_EINVAL;
    *A = small_args(W, b, dims);
    *d_out = d;
    return 0;
}

// the regularised CNF state [(l), (L1), (L2), (e), (f), y], the reference's order, not bit order:
// reg_mask bit 0 squared_L2, bit 1 jacobian_frobenius, bit 2 L1, bit 3 L2; at least one; the Jacobian penalty with the
// exact trace only (mode 0) and with its side buffer; mode 2 (no trace) carries no l column
constexpr int cg_reg_cols(int REG) { return (REG & 1) + ((REG >> 1) & 1); }
constexpr int cg_aug_cols(int mode, int reg_mask) {
    return (mode != 2) + (reg_mask & 1) + ((reg_mask >> 1) & 1) + ((reg_mask >> 2) & 1) + ((reg_mask >> 3) & 1);
}
static inline int cnf_reg_check(int mode, int reg_mask, const float* jac_sq) {
    if (mode < 0 || mode > 2 || reg_mask < 1 || reg_mask > 15) return CFM_EINVAL;
    if ((reg_mask & 2) && (mode != 0 || !jac_sq)) return CFM_EINVAL;
    return 0;
}

// The envelope of the gradient-field entries: 4 layers [d + 1, n1, n2, n3, 1], 1 <= every width <= SM_W, d + 1 <= SM_W,
// fused path on.  There is no layer-per-kernel form of this field.
static inline int grad_check(const float* const* W, const float* const* b, const int* dims, int n_layers, int B, int* d_out,
                             SmArgs* A) {
    if (!W || !b || !dims || B <= 0 || n_layers != 4) return CFM_EINVAL;
    const int d = dims[0] - 1;
    if (dims[4] != 1 || d < 1 || d + 1 > SM_W) return CFM_EINVAL;
    for (int l = 1; l <= 3; ++l) if (dims[l] < 1 || dims[l] > SM_W) return CFM_EINVAL;
    if (!cfm_ode_fused_internal()) return CFM_EINVAL;
    *A = small_args(W, b, dims);
    *d_out = d;
    return 0;
}
