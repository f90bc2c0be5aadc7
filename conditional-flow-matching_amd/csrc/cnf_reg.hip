// cnf_reg.hip — the regularised CNF solve (RNODE / TrajectoryNet): the Euler solve of the augmented state with the kinetic
// and Jacobian penalties as path integrals, on the tile engine of small_field.h.  The C entry is
// ode.hip's (cnf_reg.h), the gradient small_grad.hip's (cnf_grad.h: ode_small_euler_grad<MODE, REG>).  A unit of its own: with
// these kernels inside ode.hip the compiler gave two of that unit's existing kernels four more registers each.
//
// State [l, (e), (f), y], D = 1 + r + d; REG bit 0 carries e (squared_L2), bit 1 carries f (jacobian_frobenius), in the
// reference's order (runner/src/models/components/augmentation.py:158-177).  Per step, everything at (y_n, t_n):
//   y += h v      l -= h tr J      e += h |v|^2      f += h sqrt(S) / d,  S = sum_k |J e_k|^2,  J e_k = W_3 T_3^k
// v and div are computed by the arithmetic of sm_field_aug, operation for operation, and stepped by the arithmetic of
// ode_small_fixed<CFM_ODE_EULER>: columns l and y carry the bits of cfm_ode_fixed_cnf_mlp_f32 at Euler.  The additions:
//   |v|^2: one more sm_rowsum over the output tile;
//   S:     per exact direction T_3^k goes to a third tile buffer and one more sm_gemm gives the full column J e_k (the
//          trace needs entry k alone); its squares are summed per lane over k and per row by a third sm_rowsum.
// The three row sums use three scratch regions, so none is overwritten while another wave still reads it.  S_n is written
// per (step, row) to the caller's side buffer jsq [n_t - 1, B]: the backward divides by sqrt(S) and reads the forward's
// bits there in place of a second pass over the directions.
//
// NV: the sampler's path diagnostics, AugmentationModule's L1 and L2 columns, and the "no trace" mode.
// State [(l), (L1), (L2), (e), (f), y] in the reference's order; per step, at (y_n, t_n):
//   L1 += h (sum_j |v_j|) / d        L2 += h sqrt(sum_j v_j^2) / sqrt(d)
// L2 and e share the row sum |v|^2; L1 takes one more sm_rowsum in a fourth scratch region.  The trace mode and the
// Jacobian bit change the sweep and are template parameters; which of L1, L2 and e are carried only changes which
// columns are stepped and stored, so an NV kernel reads that from `mask` at run time (REG is 0 or 2 there).  NV = false
// is the kernel as it was: every NV branch is an `if constexpr`.  MODE == AUG_NONE has no l column and no direction
// sweep: sm_field and two row sums, the y columns those of ode_small_fixed<CFM_ODE_EULER, AUG_NONE>.
#include "small_field.h"

constexpr int cg_reg_cols(int REG) { return (REG & 1) + ((REG >> 1) & 1); }

// sm_field_aug<MODE> with the penalties' integrands: vsq = |v|^2 (REG bit 0) and jsq = S (REG bit 1, exact trace only),
// per row in every lane holding the row.  Ab2: the third tile buffer; red: 3 x [4][SM_ROWS].  NV: vsq always, and
// l1 = sum_j |v_j| through a fourth region of red.
template <int MODE, int REG, bool NV = false>
__device__ __forceinline__ SmTile sm_field_reg(const SmTile& y, float t, const SmArgs& A, int d, float* Abuf0, float* Abuf1,
                                               float* Abuf2, const float* Wl, const float* bl, const float* wt,
                                               const SmTile& eps, int nrows, float* red, int wv, int lane, SmTile& div,
                                               SmTile& vsq, SmTile& jsq, SmTile& l1) {
    static_assert(NV ? (REG == 0 || (REG == 2 && MODE == AUG_EXACT))
                     : (REG >= 1 && REG <= 3 && (MODE == AUG_EXACT || (MODE == AUG_HUTCH && REG == 1))),
                  "exact x {e, f, e + f}; Hutchinson x {e}; NV: the Jacobian bit alone is compile-time");
    const int col = wv * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) Abuf0[sm_row(i, lane) * SM_LD + col] = (col < d) ? y.v[i] : 0.f;
    sm_lds_barrier();
    SmTile acc, sl[3];
    float* src = Abuf0; float* dst = Abuf1;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int N = A.dims[l + 1];
        f32x4 c[SM_MB];
        sm_gemm(src, Wl + l * SM_W * SM_LD, wv, lane, c);
        const float bv = (col < N) ? bl[l * SM_W + col] : 0.f;
        const float wtc = (l == 0 && col < N) ? wt[col] : 0.f;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            float v = c[i >> 2][i & 3] + bv;
            if (l == 0) v = fmaf(t, wtc, v);
            if (l < 3) {
                sl[l].v[i] = (col < N && sm_row(i, lane) < nrows) ? selu_slope(v) : 0.f;
                v = selu_f(v);
            }
            acc.v[i] = (col < N) ? v : 0.f;
        }
        if (l < 3) {
#pragma unroll
            for (int i = 0; i < SM_V; ++i) dst[sm_row(i, lane) * SM_LD + col] = acc.v[i];
            sm_lds_barrier();
            float* tmp = src; src = dst; dst = tmp;
        }
    }
    SmTile q, sq;
#pragma unroll
    for (int i = 0; i < SM_V; ++i) sq.v[i] = 0.f;
    if constexpr (MODE == AUG_HUTCH) {
#pragma unroll
        for (int i = 0; i < SM_V; ++i) Abuf0[sm_row(i, lane) * SM_LD + col] = (col < d) ? eps.v[i] : 0.f;
        sm_lds_barrier();
        src = Abuf0; dst = Abuf1;
        SmTile tg;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const int N = A.dims[l + 1];
            f32x4 c[SM_MB];
            sm_gemm(src, Wl + l * SM_W * SM_LD, wv, lane, c);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                float u = c[i >> 2][i & 3];
                if (l < 3) u = sl[l].v[i] * u;
                tg.v[i] = (col < N) ? u : 0.f;
            }
            if (l < 3) {
#pragma unroll
                for (int i = 0; i < SM_V; ++i) dst[sm_row(i, lane) * SM_LD + col] = tg.v[i];
                sm_lds_barrier();
                float* tmp = src; src = dst; dst = tmp;
            }
        }
#pragma unroll
        for (int i = 0; i < SM_V; ++i) q.v[i] = (col < d) ? eps.v[i] * tg.v[i] : 0.f;
    } else {
        (void)eps;
        const int N1 = A.dims[1], N2 = A.dims[2], N3 = A.dims[3];
#pragma unroll
        for (int i = 0; i < SM_V; ++i) q.v[i] = 0.f;
        for (int k = 0; k < d; ++k) {
            const float w0 = (col < N1) ? Wl[col * SM_LD + k] : 0.f;                      // W0[col][k]
#pragma unroll
            for (int i = 0; i < SM_V; ++i) Abuf0[sm_row(i, lane) * SM_LD + col] = sl[0].v[i] * w0;
            sm_lds_barrier();
            f32x4 c[SM_MB];
            sm_gemm(Abuf0, Wl + 1 * SM_W * SM_LD, wv, lane, c);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) Abuf1[sm_row(i, lane) * SM_LD + col] = (col < N2) ? sl[1].v[i] * c[i >> 2][i & 3] : 0.f;
            sm_lds_barrier();
            sm_gemm(Abuf1, Wl + 2 * SM_W * SM_LD, wv, lane, c);
            const float w3 = (col < N3) ? Wl[3 * SM_W * SM_LD + k * SM_LD + col] : 0.f;  // W3[k][col]
            SmTile t3;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                t3.v[i] = (col < N3) ? sl[2].v[i] * c[i >> 2][i & 3] : 0.f;
                q.v[i] = fmaf(w3, t3.v[i], q.v[i]);
            }
            if constexpr (REG & 2) {
                // Abuf2 was last read two barriers ago (the previous direction's column product)
#pragma unroll
                for (int i = 0; i < SM_V; ++i) Abuf2[sm_row(i, lane) * SM_LD + col] = t3.v[i];
                sm_lds_barrier();
                sm_gemm(Abuf2, Wl + 3 * SM_W * SM_LD, wv, lane, c);                       // J e_k (columns >= d are 0)
#pragma unroll
                for (int i = 0; i < SM_V; ++i) sq.v[i] = fmaf(c[i >> 2][i & 3], c[i >> 2][i & 3], sq.v[i]);
            }
        }
    }
    div = sm_rowsum(q, red, wv, lane);
    if constexpr ((REG & 1) || NV) {
        SmTile p;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) p.v[i] = acc.v[i] * acc.v[i];
        vsq = sm_rowsum(p, red + 4 * SM_ROWS, wv, lane);
    }
    if constexpr (REG & 2) jsq = sm_rowsum(sq, red + 8 * SM_ROWS, wv, lane);
    if constexpr (NV) {
        SmTile p;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) p.v[i] = fabsf(acc.v[i]);
        l1 = sm_rowsum(p, red + 12 * SM_ROWS, wv, lane);
    }
    return acc;
}

constexpr size_t cr_lds_bytes = small_lds_bytes(1, 3, true) + sizeof(float) * 8 * SM_ROWS;
static_assert(cr_lds_bytes == 84736, "the regularised solve");
// NV: a fourth row-sum region; without a trace two tile buffers and two regions (vsq, l1): two workgroups fit a CU
constexpr size_t cr_lds_bytes_nv = cr_lds_bytes + sizeof(float) * 4 * SM_ROWS;
constexpr size_t cr_lds_bytes_notrace = small_lds_bytes(1, 2, true) + sizeof(float) * 4 * SM_ROWS;
static_assert(cr_lds_bytes_nv == 84992 && cr_lds_bytes_notrace == 80128 && 2 * cr_lds_bytes_notrace <= 160 * 1024,
              "the regularised solve with the |v| integrals");

// traj [n_t, B, D], slice 0 = the initial state; jsq [n_t - 1, B] (written with REG bit 1 only); mask: reg_mask, read by
// the NV kernels only (bits 0, 2, 3: which of e, L1, L2 the state carries)
template <int MODE, int REG, bool NV = false>
__global__ __launch_bounds__(256) void ode_small_euler_reg(SmArgs A, int B, int d, const float* __restrict__ tspan, int n_t,
                                                        float* __restrict__ traj, const float* __restrict__ eps,
                                                        float* __restrict__ jsq, int mask) {
    static_assert(MODE != AUG_NONE || (NV && REG == 0), "no trace: an NV kernel without the Jacobian bit");
    constexpr bool TRACE = MODE != AUG_NONE;
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* Wl = small_lds;
    float* bl = Wl + 4 * SM_W * SM_LD;
    float* wt = bl + 4 * SM_W;
    float* Ab0 = wt + SM_W;
    float* Ab1 = Ab0 + SM_ROWS * SM_LD;
    float* Ab2 = Ab1 + SM_ROWS * SM_LD;
    float* red = TRACE ? Ab2 + SM_ROWS * SM_LD : Ab2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    sm_stage_weights(A, d, Wl, bl, wt, tid);
    // the columns of L1, L2, e, f and y_0: [(l), (L1), (L2), (e), (f), y]
    const bool h1 = NV && (mask & 4), h2 = NV && (mask & 8), he = NV ? (mask & 1) != 0 : (REG & 1) != 0;
    const int c1 = TRACE ? 1 : 0, c2 = c1 + (h1 ? 1 : 0);
    const int ce = NV ? c2 + (h2 ? 1 : 0) : 1, cf = NV ? ce + (he ? 1 : 0) : 1 + (REG & 1);
    const int c0 = NV ? cf + ((REG >> 1) & 1) : 1 + cg_reg_cols(REG);
    const int D = d + c0;
    const size_t n = (size_t)B * D;
    const int col = wv * 16 + (lane & 15);
    const bool lw = wv == 0 && (lane & 15) == 0;
    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        SmTile x, xl, xe, xf, ep, x1, x2;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            x.v[i] = (gr < B && col < d) ? traj[(size_t)gr * D + c0 + col] : 0.f;
            xl.v[i] = (TRACE && gr < B) ? traj[(size_t)gr * D] : 0.f;
            xe.v[i] = (he && gr < B) ? traj[(size_t)gr * D + ce] : 0.f;
            xf.v[i] = ((REG & 2) && gr < B) ? traj[(size_t)gr * D + cf] : 0.f;
            ep.v[i] = (MODE == AUG_HUTCH && gr < B && col < d) ? eps[(size_t)gr * d + col] : 0.f;
            if constexpr (NV) {
                x1.v[i] = (h1 && gr < B) ? traj[(size_t)gr * D + c1] : 0.f;
                x2.v[i] = (h2 && gr < B) ? traj[(size_t)gr * D + c2] : 0.f;
            }
        }
        __syncthreads();
        for (int k = 0; k + 1 < n_t; ++k) {
            const float t = tspan[k], dt = tspan[k + 1] - tspan[k];
            SmTile dv, vs, js, ls;
            SmTile f;
            if constexpr (TRACE) {
                f = sm_field_reg<MODE, REG, NV>(x, t, A, d, Ab0, Ab1, Ab2, Wl, bl, wt, ep, B - row0, red, wv, lane, dv, vs, js, ls);
            } else {
                f = sm_field(x, t, A, d, Ab0, Ab1, Wl, bl, wt, wv, lane);
                SmTile p;
#pragma unroll
                for (int i = 0; i < SM_V; ++i) p.v[i] = f.v[i] * f.v[i];
                vs = sm_rowsum(p, red, wv, lane);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) p.v[i] = fabsf(f.v[i]);
                ls = sm_rowsum(p, red + 4 * SM_ROWS, wv, lane);
            }
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const float acc = 1.f * f.v[i];                                   // fx_b<CFM_ODE_EULER>(0)
                x.v[i] = fmaf(dt, acc, x.v[i]);
                const int gr = row0 + sm_row(i, lane);
                const size_t at = (size_t)(k + 1) * n + (size_t)gr * D;
                if (gr < B && col < d) traj[at + c0 + col] = x.v[i];
                if constexpr (TRACE) {
                    const float lf = -dv.v[i];
                    const float lacc = 1.f * lf;
                    xl.v[i] = fmaf(dt, lacc, xl.v[i]);
                    if (gr < B && lw) traj[at] = xl.v[i];
                }
                if constexpr (NV) {
                    x1.v[i] = fmaf(dt, ls.v[i] / (float)d, x1.v[i]);
                    x2.v[i] = fmaf(dt, sqrtf(vs.v[i]) / sqrtf((float)d), x2.v[i]);
                    if (gr < B && lw && h1) traj[at + c1] = x1.v[i];
                    if (gr < B && lw && h2) traj[at + c2] = x2.v[i];
                    xe.v[i] = fmaf(dt, vs.v[i], xe.v[i]);
                    if (gr < B && lw && he) traj[at + ce] = xe.v[i];
                } else if constexpr (REG & 1) {
                    xe.v[i] = fmaf(dt, vs.v[i], xe.v[i]);
                    if (gr < B && lw) traj[at + ce] = xe.v[i];
                }
                if constexpr (REG & 2) {
                    xf.v[i] = fmaf(dt, sqrtf(js.v[i]) / (float)d, xf.v[i]);
                    if (gr < B && lw) {
                        traj[at + cf] = xf.v[i];
                        jsq[(size_t)k * B + gr] = js.v[i];
                    }
                }
            }
        }
    }
}

template <int MODE, int REG, bool NV = false>
static int cnf_reg_solve(const SmArgs& A, int B, int d, const float* t_span, int n_t, float* traj, float* tspan_dev,
                         const float* eps, float* jsq, int mask, hipStream_t s) {
    const int grid = small_grid<ode_small_euler_reg<MODE, REG, NV>, 128 * 1024>(B);
    if (grid < 0) return CFM_EINVAL;
    int rc = cfm_hip(hipMemcpyAsync(tspan_dev, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    const size_t lds = !NV ? cr_lds_bytes : MODE == AUG_NONE ? cr_lds_bytes_notrace : cr_lds_bytes_nv;
    hipLaunchKernelGGL((ode_small_euler_reg<MODE, REG, NV>), dim3(grid), dim3(256), lds, s, A, B, d, tspan_dev, n_t, traj, eps,
                       jsq, mask);
    return cfm_status();
}

// Eight instantiations: the four of masks 1 to 3 as they were, and four NV ones (no trace; exact with and without the
// Jacobian bit; Hutchinson) that take bits 0, 2 and 3 at run time.  Masks 1 to 3 with a trace never reach an NV kernel.
extern "C" int cfm_cnf_reg_solve_internal(const SmArgs* A, int B, int d, const float* t_span, int n_t, float* traj,
                                          float* tspan_dev, const float* eps, float* jsq, int mode, int reg_mask,
                                          hipStream_t s) {
    if (mode == 2) return cnf_reg_solve<AUG_NONE, 0, true>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
    if (reg_mask & 12) {
        if (mode == 1) return cnf_reg_solve<AUG_HUTCH, 0, true>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
        if (reg_mask & 2) return cnf_reg_solve<AUG_EXACT, 2, true>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
        return cnf_reg_solve<AUG_EXACT, 0, true>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
    }
    if (mode == 1) return cnf_reg_solve<AUG_HUTCH, 1>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
    if (reg_mask == 1) return cnf_reg_solve<AUG_EXACT, 1>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
    if (reg_mask == 2) return cnf_reg_solve<AUG_EXACT, 2>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
    return cnf_reg_solve<AUG_EXACT, 3>(*A, B, d, t_span, n_t, traj, tspan_dev, eps, jsq, reg_mask, s);
}
