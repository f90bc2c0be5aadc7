// small_grad.hip — the training-gradient kernels of the small fields: the gradients of the CNF Euler solve and of its
// regularised form (cnf_grad.h), of the fixed-step and adaptive ODE solves (ode_grad.h, ode_adaptive_grad.h, on the one
// reverse step of ode_reverse.h) and the action-matching loss with its gradient (action_grad.h).
//
// A translation unit of its own: inside ode.hip, device-side changes to these kernels moved the code and register counts
// of the forward solvers (profiles/ode_unit_fold.txt); here only gradient kernels can be perturbed.  What the two units
// share has one definition each: the tile engine (small_field.h), the tableaus (ode_tableau.h), the envelope checks and
// the step record (ode_envelope.h).
//
// Every gradient kernel runs on at most CG_MAXGRID workgroups, each of which writes one partial gradient; the reduce
// launch adds the partials in workgroup order (the same bits run to run, no float atomics).  This file holds that common
// end of the five entries: the outputs, the workspace split, the two launches.
#include "cfm_common.h"
#include "small_field.h"
#include "ode_tableau.h"
#include "ode_envelope.h"

#define CG_PMAX (4 * SM_W * SM_W + 4 * SM_W)           // floats of one partial gradient at most

struct CgOut { float* dW[4]; float* db[4]; };

extern "C" size_t cfm_cnf_grad_ws_bytes_internal(int B, int n_t) {
    if (B <= 0 || n_t < 1) return 0;
    const size_t tiles = ((size_t)B + SM_ROWS - 1) / SM_ROWS;
    const size_t g = tiles < CG_MAXGRID ? tiles : CG_MAXGRID;
    return cfm_align_up(sizeof(float) * (size_t)n_t, 256) + sizeof(float) * g * CG_PMAX;
}

// dW[], db[] = scale * the partials added in workgroup order (scale = 1 changes no bit); tail: null, or where the one
// element that a partial carries behind db[3] goes (action_grad.h: the loss)
__global__ __launch_bounds__(256) void ode_small_grad_reduce(const float* __restrict__ part, int nparts, int P, SmArgs A,
                                                          CgOut O, float scale, float* __restrict__ tail) {
    int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float sum = 0.f;
    for (int g = 0; g < nparts; ++g) sum += part[(size_t)g * P + p];
    sum *= scale;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int nw = A.dims[l + 1] * A.dims[l], nb = A.dims[l + 1];
        if (p >= 0 && p < nw) O.dW[l][p] = sum;
        p -= nw;
        if (p >= 0 && p < nb) O.db[l][p] = sum;
        p -= nb;
    }
    if (tail && p == 0) *tail = sum;
}

// the outputs of a gradient entry, every one given: the floats of one partial gradient (W0, b0, .., W3, b3), or -1
static int cg_out(const int* dims, float* const* dW, float* const* db, CgOut* O) {
    int P = 0;
    for (int l = 0; l < 4; ++l) {
        if (!dW[l] || !db[l]) return -1;
        O->dW[l] = dW[l]; O->db[l] = db[l];
        P += dims[l + 1] * (dims[l] + 1);
    }
    return P;
}

// the layout of cfm_cnf_grad_ws_bytes_internal: the device copy of t_span, then one partial gradient per workgroup
struct CgWs { float* tspan; float* part; };
static CgWs cg_carve(void* ws, int n_t) {
    return CgWs{(float*)ws, (float*)((char*)ws + cfm_align_up(sizeof(float) * (size_t)n_t, 256))};
}

// KERNEL(args...) on one workgroup per 16-row tile (CG_MAXGRID at most), each writing its partial part[workgroup][P], then
// the reduce into O
template <auto KERNEL, int LDS_LIMIT, class... Args>
static int cg_launch(size_t lds, hipStream_t s, int B, float* part, int P, const SmArgs& A, const CgOut& O, float scale,
                     float* tail, Args... args) {
    const int grid = small_grid<KERNEL, LDS_LIMIT>(B, CG_MAXGRID);
    if (grid < 0) return CFM_EINVAL;
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(256), lds, s, args...);
    int rc = cfm_status();
    if (rc) return rc;
    hipLaunchKernelGGL(ode_small_grad_reduce, dim3((P + 255) / 256), dim3(256), 0, s, (const float*)part, grid, P, A, O, scale, tail);
    return cfm_status();
}

// ---- CNF training: the gradient of the Euler augmented solve, plain and regularised (ode_small_euler_grad,
// cfm_cnf_euler_grad_f32, cfm_cnf_reg_euler_grad_f32) ----
#include "cnf_grad.h"

// ---- training through the sampler: the gradient of the plain fixed-step solves (ode_small_fixed_grad, cfm_ode_fixed_grad_f32) ----
#include "ode_grad.h"

// ---- training through the adaptive sampler: the gradient of the accepted steps of the recording solve
// (ode_small_adaptive_grad, cfm_ode_adaptive_grad_f32) ----
#include "ode_adaptive_grad.h"

// ---- action-matching training: loss and parameter gradient in one launch (cfm_action_matching_grad_f32) ----
#include "action_grad.h"
