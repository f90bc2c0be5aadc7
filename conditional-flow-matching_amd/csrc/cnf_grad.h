// cnf_grad.h — gradient of the Euler solve of the augmented CNF state (included by small_grad.hip, whose host tail and
// reduce launch it ends on; the tile engine it runs on comes from small_field.h: SmTile, sm_gemm, cg_gemm_t,
// sm_stage_weights, selu_f, selu_slope; cnf_check, cnf_reg_check and cg_reg_cols from ode_envelope.h).
//
// Forward (ode_small_fixed<CFM_ODE_EULER, MODE>):  y_{n+1} = y_n + h_n v(y_n, t_n),  l_{n+1} = l_n - h_n div(y_n, t_n).
// Given G = dL/d[l_N, y_N]:  c = G[:, 0] never changes (l enters linearly), a_N = G[:, 1:], and for n = N-1 .. 0
//   g_n(y, theta) = a_{n+1} . v - c div        a_n = a_{n+1} + h_n grad_y g_n(y_n)        theta_bar += h_n sum_rows grad_theta g_n
// h_n is folded into the seeds: the step runs the reverse pass of g with (h a, h c) in place of (a, c).
//
// One reverse step on a 16-row tile (z_l pre-activations, s_l = selu'(z_l), q_l = selu''(z_l), U_l^k = W_{l-1} T_{l-1}^k,
// T_l^k = s_l * U_l^k, div = sum_k w_k^T W_3 T_3^k; exact: (T_0^k, w_k) = (e_k, e_k), k < d; Hutchinson: one pair (eps, eps)):
//   primal forward from y_n (the forward pass's code: same z bits, so the same side of every kink): s_l, q_l, h_l in registers
//   per direction k:   T_1..T_3 forward;   Tb_3 = -c w_k^T W_3;   for l = 3..1:  sb_l += Tb_l * U_l,  Ub_l = s_l * Tb_l,
//                      dW_{l-1} += Ub_l^T T_{l-1},  Tb_{l-1} = Ub_l W_{l-1};   dW_3 += w_k^T (-c T_3)
//   primal reverse:    hb_3 = a W_3, dW_3 += a^T h_3, db_3 += a;   for l = 3..1:  zb_l = hb_l * s_l + sb_l * q_l,
//                      dW_{l-1} += zb_l^T h_{l-1}, db_{l-1} += zb_l, hb_{l-1} = zb_l W_{l-1};   a += hb_0[:, :d];
//                      the time column of W_0 gets t_n zb_1 (the tangents have no time component)
// Products with W_l run through sm_gemm on the staged weights; products with W_l^T (the pull-backs) run through sm_gemm on
// TRANSPOSED copies of the two 64 x 64 layers (same conflict-free fragment reads), and through cg_gemm_t, which reads the
// staged matrix by columns, for the two thin layers (once per step each).  Weight gradients are MFMA accumulators with
// K = the 16 rows of the tile (cg_outer), kept across all steps and tiles of the workgroup; every workgroup writes one
// partial gradient and ode_small_grad_reduce adds the partials in workgroup order: the same bits run to run.
// Rows are independent: no cross-workgroup wait of any kind.
//
// REG (bit 0: squared_L2, bit 1: jacobian_frobenius) is the regularised solve of cnf_reg.hip: the state is
// [l, (e), (f), y], e += h |v|^2, f += h sqrt(S) / d with S = sum_k |J e_k|^2, J e_k = W_3 T_3^k.  With ce, cf the upstream
// columns of e and f (constant along the solve, as c is):
//   g_n = a . v - c div + ce |v|^2 + cf sqrt(S) / d
//   bit 0: the primal output cotangent is h (a + 2 ce v) in place of h a: the last layer is evaluated for v
//   bit 1: the cotangent of direction k's column J e_k is Jb_k = -h c e_k + (h cf / (d sqrt(S))) J e_k (no second term
//          where S = 0, as torch.norm's backward has it), so Tb_3 = Jb_k W_3 and dW_3 += Jb_k^T T_3^k: one sm_gemm for
//          J e_k, one cg_gemm_t and one cg_outer on a sixth tile buffer JB; S is read from the forward's side buffer
//          jsq [n_t - 1, B].  Below Tb_3 the sweep is the one above.
// REG = 0 is the kernel as it was: every REG branch is an `if constexpr`.
//
// NV (reg_mask bits 2 and 3): the state is [l, (L1), (L2), (e), (f), y], L1 += h (sum_j |v_j|) / d,
// L2 += h |v| / sqrt(d).  With c1, c2 their upstream columns g_n gains c1 (sum_j |v_j|) / d + c2 |v| / sqrt(d), so the primal
// output cotangent is h (a + 2 ce v + c1 sign(v) / d + c2 v / (sqrt(d) |v|)), sign(0) = 0 and no c2 term where |v| = 0
// (torch.abs's and torch.norm's backward).  |v|^2 per row is one sm_rowsum over v (a scratch region behind the tile
// buffers); nothing else changes.  As in the forward, the Jacobian bit stays compile-time (REG is 0 or 2) and which of
// e, L1, L2 are carried is read from `mask` at run time: a column that is absent has cotangent 0.
#pragma once

// W1^T, W2^T -> LDS, zero padded to [2][64][SM_LD]: WT[l - 1][k][r] = W_l[r][k]
__device__ __forceinline__ void cg_stage_transposed(const SmArgs& A, float* WT, int tid) {
#pragma unroll
    for (int l = 1; l <= 2; ++l) {
        const int in_l = A.dims[l], out_l = A.dims[l + 1];
        for (int e = tid; e < SM_W * SM_LD; e += 256) {
            const int k = e / SM_LD, r = e % SM_LD;
            WT[(l - 1) * SM_W * SM_LD + e] = (r < out_l && k < in_l) ? A.W[l][(size_t)r * in_l + k] : 0.f;
        }
    }
}

// A workgroup's partial gradient Pw in the order W0, b0, W1, b1, W2, b2, W3, b3 (each as the caller's tensor is laid
// out) from its accumulators: dWa in cg_outer's layout, dba / dwt per lane (bias and time-column sums of the lane's rows)
__device__ __forceinline__ void cg_store_partial(const SmArgs& A, int d, float* __restrict__ Pw, const f32x4 (&dWa)[4][4],
                                                 const float (&dba)[4], float dwt, int lane, int col) {
    int off = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int in_l = A.dims[l], out_l = A.dims[l + 1];
        const int K = (l == 0) ? d : in_l;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * mb + 4 * (lane >> 4) + i;
                if (r < out_l && col < K) Pw[off + r * in_l + col] = dWa[l][mb][i];
            }
        }
        float bsum = dba[l];
        bsum += __shfl_xor(bsum, 16, 64);
        bsum += __shfl_xor(bsum, 32, 64);
        if (l == 0) {
            float tsum = dwt;
            tsum += __shfl_xor(tsum, 16, 64);
            tsum += __shfl_xor(tsum, 32, 64);
            if (lane < 16 && col < out_l) Pw[off + col * in_l + d] = tsum;
        }
        off += out_l * in_l;
        if (lane < 16 && col < out_l) Pw[off + col] = bsum;
        off += out_l;
    }
}

// one staged net, the transposed copies of its two 64 x 64 layers, five tile buffers
constexpr size_t cg_lds_bytes = small_lds_bytes(1, 5, false) + sizeof(float) * 2 * SM_W * SM_LD;
static_assert(cg_lds_bytes == 127488, "the gradient kernel");
// the sixth tile buffer (JB) of the jacobian_frobenius sweep: above 128 KB, inside the CU's 160 KB
constexpr size_t cg_lds_bytes_jac = cg_lds_bytes + sizeof(float) * SM_ROWS * SM_LD;
static_assert(cg_lds_bytes_jac == 131840 && cg_lds_bytes_jac <= 160 * 1024, "the gradient kernel with the Jacobian penalty");
// NV: sm_rowsum's scratch behind the last tile buffer
constexpr size_t cg_lds_bytes_red = sizeof(float) * 4 * SM_ROWS;
static_assert(cg_lds_bytes + cg_lds_bytes_red <= 128 * 1024 && cg_lds_bytes_jac + cg_lds_bytes_red <= 160 * 1024, "the |v| row sum");

// traj [n_t, B, D]: the forward solve (y_n is read), D = 1 + cg_reg_cols(REG) + d (NV: cg_aug_cols(0, mask) + d);
// G [B, D]; g0 [B, D] or null;
// part [gridDim.x][P]: the workgroup's partial gradient in the order W0, b0, W1, b1, W2, b2, W3, b3 (each as the caller's
// tensor is laid out); jsq [n_t - 1, B]: S per (step, row) as the forward wrote it (read with REG bit 1 only); mask:
// reg_mask, read by the NV kernels only
template <int MODE, int REG = 0, bool NV = false>
__global__ __launch_bounds__(256) void ode_small_euler_grad(SmArgs A, int B, int d, const float* __restrict__ tspan, int n_t,
                                                         const float* __restrict__ traj, const float* __restrict__ eps,
                                                         const float* __restrict__ G, float* __restrict__ g0,
                                                         float* __restrict__ part, int P,
                                                         const float* __restrict__ jsq, int mask) {
    static_assert(REG >= 0 && REG <= 3 && (MODE == AUG_EXACT || !(REG & 2)), "the Jacobian penalty needs the exact directions");
    static_assert(!NV || !(REG & 1), "NV: bit 0 is read from mask");
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    constexpr int TS = SM_ROWS * SM_LD, WS = SM_W * SM_LD;
    float* Wl = small_lds;
    float* WT = Wl + 4 * WS;                  // W1^T, W2^T
    float* bl = WT + 2 * WS;
    float* wt = bl + 4 * SM_W;
    float* E = wt + SM_W;
    float* X1 = E + TS;
    float* X2 = X1 + TS;
    float* X3 = X2 + TS;
    float* Y3 = X3 + TS;
    float* JB = Y3 + TS;                      // REG bit 1 only (cg_lds_bytes_jac)
    float* red = (REG & 2) ? JB + TS : JB;    // NV only (cg_lds_bytes_red)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    sm_stage_weights(A, d, Wl, bl, wt, tid);
    cg_stage_transposed(A, WT, tid);
    // the columns of L1, L2, e, f and y_0 in a state row [l, (L1), (L2), (e), (f), y]
    const bool h1 = NV && (mask & 4), h2 = NV && (mask & 8), he = NV ? (mask & 1) != 0 : (REG & 1) != 0;
    const int k1 = 1, k2 = k1 + (h1 ? 1 : 0);
    const int ke = NV ? k2 + (h2 ? 1 : 0) : 1, kf = NV ? ke + (he ? 1 : 0) : 1 + (REG & 1);
    const int c0 = NV ? kf + ((REG >> 1) & 1) : 1 + cg_reg_cols(REG);
    const int D = d + c0;
    const size_t n = (size_t)B * D;
    const int col = wv * 16 + (lane & 15);
    const bool lw = wv == 0 && (lane & 15) == 0;
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
        SmTile a, cv, ep, yn, ce, cf, cl1, cl2;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const int gr = row0 + sm_row(i, lane);
            const bool ok = gr < B && col < d;
            a.v[i] = ok ? G[(size_t)gr * D + c0 + col] : 0.f;
            cv.v[i] = gr < B ? G[(size_t)gr * D] : 0.f;
            if constexpr (REG & 1) ce.v[i] = gr < B ? G[(size_t)gr * D + 1] : 0.f;
            if constexpr (REG & 2) cf.v[i] = gr < B ? G[(size_t)gr * D + kf] : 0.f;
            if constexpr (NV) {
                ce.v[i] = (he && gr < B) ? G[(size_t)gr * D + ke] : 0.f;
                cl1.v[i] = (h1 && gr < B) ? G[(size_t)gr * D + k1] : 0.f;
                cl2.v[i] = (h2 && gr < B) ? G[(size_t)gr * D + k2] : 0.f;
            }
            ep.v[i] = (MODE == AUG_HUTCH && ok) ? eps[(size_t)gr * d + col] : 0.f;
            yn.v[i] = (ok && n_t >= 2) ? traj[(size_t)(n_t - 2) * n + (size_t)gr * D + c0 + col] : 0.f;
        }
        __syncthreads();
        for (int st = n_t - 2; st >= 0; --st) {
            const float t = tspan[st], h = tspan[st + 1] - tspan[st];
            const SmTile y = yn;
            if (st > 0) {
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const int gr = row0 + sm_row(i, lane);
                    yn.v[i] = (gr < B && col < d) ? traj[(size_t)(st - 1) * n + (size_t)gr * D + c0 + col] : 0.f;
                }
            }
            SmTile ap, cp;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) { ap.v[i] = h * a.v[i]; cp.v[i] = -(h * cv.v[i]); }    // cp = -h c
            SmTile rs;                                    // h cf / (d sqrt(S)) per row; 0 where S = 0
            if constexpr (REG & 2) {
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const int gr = row0 + sm_row(i, lane);
                    const float S = gr < B ? jsq[(size_t)st * B + gr] : 0.f;
                    rs.v[i] = S > 0.f ? (h * cf.v[i]) / ((float)d * sqrtf(S)) : 0.f;
                }
            }

            // ---- primal forward: s_l, q_l, h_l (the arithmetic of sm_field_aug) ----
            SmTile s[3], q[3], hh[3];
            f32x4 c[SM_MB];
            cg_put(X1, y, lane, col);
            sm_lds_barrier();
            {
                float* src = X1; float* dst = X2;
#pragma unroll
                for (int l = 0; l < 3; ++l) {
                    const int N = A.dims[l + 1];
                    sm_gemm(src, Wl + l * WS, wv, lane, c);
                    const float bv = (col < N) ? bl[l * SM_W + col] : 0.f;
                    const float wtc = (l == 0 && col < N) ? wt[col] : 0.f;
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        float z = c[0][i] + bv;
                        if (l == 0) z = fmaf(t, wtc, z);
                        const float sl = (col < N && sm_row(i, lane) < nrows) ? selu_slope(z) : 0.f;
                        s[l].v[i] = sl;
                        q[l].v[i] = z > 0.f ? 0.f : sl;
                        hh[l].v[i] = (col < N) ? selu_f(z) : 0.f;
                    }
                    if (l < 2) {
                        cg_put(dst, hh[l], lane, col);
                        sm_lds_barrier();
                        float* tmp = src; src = dst; dst = tmp;
                    }
                }
                if constexpr (REG & 1) {                  // v = W3 h3 + b3: the seed of the output is h (a + 2 ce v)
                    cg_put(dst, hh[2], lane, col);        // dst = X2: last read by layer 1, a barrier ago
                    sm_lds_barrier();
                    sm_gemm(dst, W3, wv, lane, c);
                    const float bv = (col < d) ? bl[3 * SM_W + col] : 0.f;
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        const float v = (col < d) ? c[0][i] + bv : 0.f;
                        ap.v[i] = h * (a.v[i] + 2.f * ce.v[i] * v);
                    }
                }
                if constexpr (NV) {                       // the same v; the seed gains the L1 and L2 terms
                    cg_put(dst, hh[2], lane, col);
                    sm_lds_barrier();
                    sm_gemm(dst, W3, wv, lane, c);
                    const float bv = (col < d) ? bl[3 * SM_W + col] : 0.f;
                    SmTile vv, p;
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        vv.v[i] = (col < d) ? c[0][i] + bv : 0.f;
                        p.v[i] = vv.v[i] * vv.v[i];
                    }
                    const SmTile vs = sm_rowsum(p, red, wv, lane);         // |v|^2 per row
                    const float rd = 1.f / (float)d, rsd = 1.f / sqrtf((float)d);
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        const float v = vv.v[i];
                        const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
                        const float rn = vs.v[i] > 0.f ? rsd / sqrtf(vs.v[i]) : 0.f;
                        ap.v[i] = h * (((a.v[i] + 2.f * ce.v[i] * v) + cl1.v[i] * sg * rd) + cl2.v[i] * v * rn);
                    }
                }
            }
            sm_lds_barrier();       // layer 2 read X1: an exact direction writes T1 there with no barrier of its own before

            // ---- the directions: tangents forward, their cotangents back ----
            SmTile sb[3];
#pragma unroll
            for (int l = 0; l < 3; ++l) {
#pragma unroll
                for (int i = 0; i < SM_V; ++i) sb[l].v[i] = 0.f;
            }
            const int nk = (MODE == AUG_HUTCH) ? 1 : d;
            for (int k = 0; k < nk; ++k) {
                SmTile U1, U2, U3, tv;
                if constexpr (MODE == AUG_HUTCH) {
                    cg_put(E, ep, lane, col);
                    sm_lds_barrier();
                    sm_gemm(E, Wl, wv, lane, c);
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) U1.v[i] = c[0][i];
                } else {
                    const float w0 = Wl[col * SM_LD + k];                                   // W0[col][k]
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        tv.v[i] = (col == k && sm_row(i, lane) < nrows) ? 1.f : 0.f;
                        U1.v[i] = w0;
                    }
                    cg_put(E, tv, lane, col);
                }
#pragma unroll
                for (int i = 0; i < SM_V; ++i) tv.v[i] = s[0].v[i] * U1.v[i];
                cg_put(X1, tv, lane, col);                                                  // T1
                sm_lds_barrier();
                sm_gemm(X1, Wl + 1 * WS, wv, lane, c);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) { U2.v[i] = c[0][i]; tv.v[i] = s[1].v[i] * U2.v[i]; }
                cg_put(X2, tv, lane, col);                                                  // T2
                sm_lds_barrier();
                sm_gemm(X2, Wl + 2 * WS, wv, lane, c);
                if constexpr (REG & 2) {
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) { U3.v[i] = c[0][i]; tv.v[i] = s[2].v[i] * U3.v[i]; }
                    cg_put(X3, tv, lane, col);                                              // T3
                    sm_lds_barrier();
                    sm_gemm(X3, W3, wv, lane, c);                                           // J e_k (columns >= d are 0)
#pragma unroll
                    for (int i = 0; i < SM_V; ++i)
                        tv.v[i] = fmaf(rs.v[i], c[0][i], (col == k && sm_row(i, lane) < nrows) ? cp.v[i] : 0.f);
                    cg_put(JB, tv, lane, col);                                              // Jb_k
                    sm_lds_barrier();
                    cg_outer(JB, X3, wv, lane, dWa[3]);
                    cg_gemm_t(JB, W3, wv, lane, c[0]);                                      // Tb3 = Jb_k W3
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) {
                        const float tb = c[0][i];
                        sb[2].v[i] = fmaf(tb, U3.v[i], sb[2].v[i]);
                        tv.v[i] = s[2].v[i] * tb;
                    }
                } else {                  // the sweep without the Jacobian penalty: its lines as they were, indentation included
#pragma unroll
                for (int i = 0; i < SM_V; ++i) { U3.v[i] = c[0][i]; tv.v[i] = cp.v[i] * (s[2].v[i] * U3.v[i]); }
                cg_put(X3, tv, lane, col);                                                  // -h c T3
                sm_lds_barrier();
                cg_outer(E, X3, wv, lane, dWa[3]);
                if constexpr (MODE == AUG_HUTCH) {
                    cg_gemm_t(E, W3, wv, lane, c[0]);                                       // eps W3
                } else {
                    const float w3 = W3[k * SM_LD + col];                                   // W3[k][col]
                    c[0] = f32x4{w3, w3, w3, w3};
                }
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const float tb = cp.v[i] * c[0][i];
                    sb[2].v[i] = fmaf(tb, U3.v[i], sb[2].v[i]);
                    tv.v[i] = s[2].v[i] * tb;
                }
                }
                cg_put(Y3, tv, lane, col);                                                  // Ub3
                sm_lds_barrier();
                cg_outer(Y3, X2, wv, lane, dWa[2]);
                sm_gemm(Y3, W2T, wv, lane, c);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    sb[1].v[i] = fmaf(c[0][i], U2.v[i], sb[1].v[i]);
                    tv.v[i] = s[1].v[i] * c[0][i];
                }
                cg_put(X3, tv, lane, col);                                                  // Ub2
                sm_lds_barrier();
                cg_outer(X3, X1, wv, lane, dWa[1]);
                sm_gemm(X3, W1T, wv, lane, c);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    sb[0].v[i] = fmaf(c[0][i], U1.v[i], sb[0].v[i]);
                    tv.v[i] = s[0].v[i] * c[0][i];
                }
                cg_put(Y3, tv, lane, col);                                                  // Ub1
                sm_lds_barrier();
                cg_outer(Y3, E, wv, lane, dWa[0]);
                sm_lds_barrier();
            }

            // ---- primal reverse ----
            SmTile zb;
            cg_put(E, ap, lane, col);
            cg_put(X1, hh[2], lane, col);
            sm_lds_barrier();
            dba[3] += cg_sum4(ap);
            cg_outer(E, X1, wv, lane, dWa[3]);
            cg_gemm_t(E, W3, wv, lane, c[0]);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[2].v[i] + sb[2].v[i] * q[2].v[i];
            dba[2] += cg_sum4(zb);
            cg_put(X2, zb, lane, col);
            cg_put(X3, hh[1], lane, col);
            sm_lds_barrier();
            cg_outer(X2, X3, wv, lane, dWa[2]);
            sm_gemm(X2, W2T, wv, lane, c);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[1].v[i] + sb[1].v[i] * q[1].v[i];
            dba[1] += cg_sum4(zb);
            cg_put(E, zb, lane, col);
            cg_put(X1, hh[0], lane, col);
            sm_lds_barrier();
            cg_outer(E, X1, wv, lane, dWa[1]);
            sm_gemm(E, W1T, wv, lane, c);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[0].v[i] + sb[0].v[i] * q[0].v[i];
            {
                const float zs = cg_sum4(zb);
                dba[0] += zs;
                dwt = fmaf(t, zs, dwt);
            }
            cg_put(X2, zb, lane, col);
            cg_put(X3, y, lane, col);
            sm_lds_barrier();
            cg_outer(X2, X3, wv, lane, dWa[0]);
            cg_gemm_t(X2, Wl, wv, lane, c[0]);                                              // zb1 W0[:, :d]
#pragma unroll
            for (int i = 0; i < SM_V; ++i) a.v[i] += c[0][i];
            sm_lds_barrier();
        }
        if (g0) {
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const int gr = row0 + sm_row(i, lane);
                if (gr < B && col < d) g0[(size_t)gr * D + c0 + col] = a.v[i];
                if (gr < B && lw) g0[(size_t)gr * D] = cv.v[i];
                if constexpr (REG & 1) { if (gr < B && lw) g0[(size_t)gr * D + 1] = ce.v[i]; }
                if constexpr (REG & 2) { if (gr < B && lw) g0[(size_t)gr * D + kf] = cf.v[i]; }
                if constexpr (NV) {
                    if (gr < B && lw && he) g0[(size_t)gr * D + ke] = ce.v[i];
                    if (gr < B && lw && h1) g0[(size_t)gr * D + k1] = cl1.v[i];
                    if (gr < B && lw && h2) g0[(size_t)gr * D + k2] = cl2.v[i];
                }
            }
        }
    }

    cg_store_partial(A, d, part + (size_t)blockIdx.x * P, dWa, dba, dwt, lane, col);
}

template <int MODE, int REG = 0, bool NV = false>
static int cnf_grad_launch(const SmArgs& A, int B, int d, const float* tspan_dev, int n_t, const float* traj,
                           const float* eps, const float* G, float* g0, float* part, int P, const CgOut& O, hipStream_t s,
                           const float* jsq = nullptr, int mask = 0) {
    return cg_launch<ode_small_euler_grad<MODE, REG, NV>, ((REG & 2) ? 160 : 128) * 1024>(
        ((REG & 2) ? cg_lds_bytes_jac : cg_lds_bytes) + (NV ? cg_lds_bytes_red : 0), s, B, part, P, A, O, 1.f, nullptr, A, B, d,
        tspan_dev, n_t, traj, eps, G, g0, part, P, jsq, mask);
}

extern "C" int cfm_cnf_euler_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                      const float* traj, int B, const float* t_span, int n_t, int mode, const float* eps,
                                      const float* g_final, float* const* dW, float* const* db, float* g_initial, void* ws,
                                      void* stream) {
    int d; SmArgs A;
    if (!traj || !t_span || !g_final || !dW || !db || !ws || n_t < 1) return CFM_EINVAL;
    int rc = cnf_check(W, b, dims, n_layers, B, mode, eps, &d, &A);
    if (rc) return rc;
    CgOut O;
    const int P = cg_out(dims, dW, db, &O);
    if (P < 0) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const CgWs w = cg_carve(ws, n_t);
    rc = cfm_hip(hipMemcpyAsync(w.tspan, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    return mode == 0 ? cnf_grad_launch<AUG_EXACT>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s)
                     : cnf_grad_launch<AUG_HUTCH>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s);
}

// the gradient of the regularised solve (cfm_ode_euler_cnf_reg_mlp_f32, cnf_reg.h): traj, g_final, g_initial [., B, D] with
// D = cg_aug_cols(mode, reg_mask) + d; jac_sq: the forward's side buffer (reg_mask bit 1); mode 2 (no trace) has no gradient:
// cnf_check refuses it
extern "C" int cfm_cnf_reg_euler_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                          const float* traj, int B, const float* t_span, int n_t, int mode, const float* eps,
                                          int reg_mask, const float* jac_sq, const float* g_final, float* const* dW,
                                          float* const* db, float* g_initial, void* ws, void* stream) {
    int d; SmArgs A;
    if (!traj || !t_span || !g_final || !dW || !db || !ws || n_t < 1 || cnf_reg_check(mode, reg_mask, jac_sq)) return CFM_EINVAL;
    int rc = cnf_check(W, b, dims, n_layers, B, mode, eps, &d, &A);
    if (rc) return rc;
    CgOut O;
    const int P = cg_out(dims, dW, db, &O);
    if (P < 0) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const CgWs w = cg_carve(ws, n_t);
    rc = cfm_hip(hipMemcpyAsync(w.tspan, t_span, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    if (rc) return rc;
    if (reg_mask & 12) {        // three NV instantiations: bits 0, 2 and 3 at run time
        if (mode == 1) return cnf_grad_launch<AUG_HUTCH, 0, true>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s, jac_sq, reg_mask);
        if (reg_mask & 2) return cnf_grad_launch<AUG_EXACT, 2, true>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s, jac_sq, reg_mask);
        return cnf_grad_launch<AUG_EXACT, 0, true>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s, jac_sq, reg_mask);
    }
    if (mode == 1) return cnf_grad_launch<AUG_HUTCH, 1>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s, jac_sq);
    if (reg_mask == 1) return cnf_grad_launch<AUG_EXACT, 1>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s, jac_sq);
    if (reg_mask == 2) return cnf_grad_launch<AUG_EXACT, 2>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s, jac_sq);
    return cnf_grad_launch<AUG_EXACT, 3>(A, B, d, w.tspan, n_t, traj, eps, g_final, g_initial, w.part, P, O, s, jac_sq);
}
