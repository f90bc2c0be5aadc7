// action_grad.h — the action-matching loss and its parameter gradient in one launch (included by small_grad.hip after
// cnf_grad.h; SmTile, sm_gemm, cg_gemm_t, cg_put, cg_outer, cg_sum4, selu_f, selu_slope come from small_field.h,
// the host tail and the reduce launch from small_grad.hip, grad_check from ode_envelope.h).
//
// Counterpart of ActionMatchingLitModule.step (runner/src/models/cfm_module.py:670-694) and the loss.backward() that
// follows it: per row  l = s(x0, 0) - s(x1, 1) + 1/2 |grad_x s(xt, t)|^2 + d/dt s(xt, t),  loss = mean l, for the action net
// s = MLP([x, t]) with dims [d + 1, n1, n2, n3, 1].  z_l pre-activations, h_l = selu(z_l), s_l = selu'(z_l),
// q_l = selu''(z_l) (= s_l for z <= 0, else 0: grad_field.h's convention).  Per 16-row tile, three passes:
//   endpoint (x0, 0) with c = +1, endpoint (x1, 1) with c = -1: a plain backward
//       loss += c W3 . h3 (b3 cancels between the two),  dW3 += c h3,  zb3 = c W3 * s3,
//       for l = 3..1:  dW_{l-1} += zb_l^T h_{l-1},  db_{l-1} += zb_l,  zb_{l-1} = s_{l-1} * (zb_l W_{l-1})
//   interior u = [xt, t], t per row: the primal forward and reverse sweep of gf_field,
//       g3 = s3 * W3,  hb2 = g3 W2,  g2 = s2 * hb2,  hb1 = g2 W1,  g1 = s1 * hb1,  g = g1 W0  (all d + 1 columns)
//       loss += 1/2 |g[:, :d]|^2 + g[:, d];   its gradient is that of the derivative of s along the fixed w = (g_x, 1):
//       dz1 = W0 w, dh1 = s1 * dz1, dz2 = W1 dh1, dh2 = s2 * dz2, dz3 = W2 dh2;   dW3 += s3 * dz3
//       zeta3 = W3 * q3 * dz3                          dW2 += g3^T dh2 + zeta3^T h2,  db2 += zeta3
//       zeta2 = s2 * (zeta3 W2) + hb2 * q2 * dz2       dW1 += g2^T dh1 + zeta2^T h1,  db1 += zeta2
//       zeta1 = s1 * (zeta2 W1) + hb1 * q1 * dz1       dW0 += g1^T w   + zeta1^T u,   db0 += zeta1
// db3 is identically zero (the loss does not depend on b3) and is written as an exact 0.  1 / B is applied once, by the
// reduce launch, to sums of O(1) terms.
//
// Layout decisions:
//  * Layer 0 is staged with all d + 1 columns and the time sits in column d of the input tile, so the time column of W0
//    needs no code of its own: g_t is column d of g1 W0 and the time column of dW0 is column d of the MFMA accumulator.
//  * Pull-backs read the staged matrices by columns (cg_gemm_t), no transposed copies: both reads are two-way bank
//    conflicted (grad_field.h), and the copies would cost 34 KiB of LDS and their staging per launch.
//  * W3 is one row, so dW3 is a per-lane column sum like the biases; three MFMA accumulator sets (dW0..dW2, 48 VGPRs).
//  * Every tile of a pass has a buffer of its own (twelve): a buffer is written once per pass, every write is followed
//    by a barrier before its first read, and one barrier closes the pass.  No buffer is recycled inside a pass, so there
//    is no write-after-read order to get wrong; the LDS is there because the grid is at most CG_MAXGRID = one workgroup
//    per CU whatever the image size, so a second workgroup per CU would have nothing to run.
// Weight gradients, bias sums and the loss are kept across the workgroup's tiles; every workgroup writes one partial
// (gradient, then its loss term) and ode_small_grad_reduce adds the partials in workgroup order and scales by 1 / B:
// the same bits run to run, no float atomics, no cross-workgroup wait.
#pragma once

#define AM_TILES 12
constexpr size_t am_lds_bytes = sizeof(float) * (3 * SM_W * SM_LD + 4 * SM_W + AM_TILES * SM_ROWS * SM_LD + 4);
static_assert(am_lds_bytes == 105488, "the action-matching gradient kernel");

extern "C" size_t cfm_action_grad_ws_bytes_internal(int B) {
    if (B <= 0) return 0;
    const size_t tiles = ((size_t)B + SM_ROWS - 1) / SM_ROWS;
    const size_t g = tiles < CG_MAXGRID ? tiles : CG_MAXGRID;
    return sizeof(float) * g * CG_PMAX;
}

struct AmAcc {
    f32x4 dW[3][4];        // dW0, dW1, dW2 in cg_outer's layout
    float db[3], dw3, loss;
};

// the forward chain of one pass: U holds [x, t]; h1, h2 are left in H1, H2 for the outer products; s_l, q_l and h3 in registers
__device__ __forceinline__ void am_forward(const SmArgs& A, const float* Wl, const float* bl, const float* U, float* H1,
                                           float* H2, int nrows, int wv, int lane, int col, SmTile (&s)[3], SmTile (&q)[3],
                                           SmTile& h3) {
    constexpr int WS = SM_W * SM_LD;
    f32x4 c[SM_MB];
    const float* src = U;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int N = A.dims[l + 1];
        sm_gemm(src, Wl + l * WS, wv, lane, c);
        const float bv = (col < N) ? bl[l * SM_W + col] : 0.f;
        SmTile hv;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const float z = c[0][i] + bv;
            const float sl = (col < N && sm_row(i, lane) < nrows) ? selu_slope(z) : 0.f;
            s[l].v[i] = sl;
            q[l].v[i] = z > 0.f ? 0.f : sl;
            hv.v[i] = (col < N) ? selu_f(z) : 0.f;
        }
        if (l < 2) {
            float* dst = l == 0 ? H1 : H2;
            cg_put(dst, hv, lane, col);
            sm_lds_barrier();
            src = dst;
        } else {
            h3 = hv;
        }
    }
}

// x [B, d] rows row0.. and the time into U (column d); rows beyond B are zero.  x null: the reference's interpolant
// t * x1 + (1 - t) * x0 in its eager operation order (four roundings, no contraction: the bits torch's ops give)
__device__ __forceinline__ void am_load(float* U, const float* __restrict__ x, const float* __restrict__ t, float tconst,
                                        const float* __restrict__ x0, const float* __restrict__ x1, int row0, int B, int d,
                                        int lane, int col) {
#pragma unroll
    for (int i = 0; i < SM_V; ++i) {
        const int r = sm_row(i, lane), gr = row0 + r;
        float v = 0.f;
        if (gr < B) {
            const float tr = t ? t[gr] : tconst;
            const size_t e = (size_t)gr * d + col;
            if (col < d) v = x ? x[e] : tr * x1[e] + (1.f - tr) * x0[e];
            else if (col == d) v = tr;
        }
        U[r * SM_LD + col] = v;
    }
    sm_lds_barrier();
}

// one endpoint: the value with cotangent cs (+1 at (x0, 0), -1 at (x1, 1)) and its plain backward
__device__ __forceinline__ void am_endpoint(const SmArgs& A, const float* Wl, const float* bl, const float* w3l, float* T,
                                            const float* __restrict__ x, float tconst, float cs, int row0, int B, int d,
                                            int wv, int lane, int col, AmAcc& acc) {
    constexpr int TS = SM_ROWS * SM_LD, WS = SM_W * SM_LD;
    float* U = T; float* H1 = T + TS; float* H2 = T + 2 * TS; float* Z3 = T + 3 * TS; float* Z2 = T + 4 * TS; float* Z1 = T + 5 * TS;
    const int nrows = B - row0;
    SmTile s[3], q[3], h3, zb;
    f32x4 c;
    am_load(U, x, nullptr, tconst, nullptr, nullptr, row0, B, d, lane, col);
    am_forward(A, Wl, bl, U, H1, H2, nrows, wv, lane, col, s, q, h3);
    (void)q;
    const float w3 = cs * w3l[col];                                     // c W3[0][col] (0 beyond n3)
    float hs = 0.f;
#pragma unroll
    for (int i = 0; i < SM_V; ++i) {
        hs += (sm_row(i, lane) < nrows) ? h3.v[i] : 0.f;
        zb.v[i] = w3 * s[2].v[i];                                       // zb3
    }
    acc.loss = fmaf(w3, hs, acc.loss);
    acc.dw3 = fmaf(cs, hs, acc.dw3);
    acc.db[2] += cg_sum4(zb);
    cg_put(Z3, zb, lane, col);
    sm_lds_barrier();
    cg_outer(Z3, H2, wv, lane, acc.dW[2]);
    cg_gemm_t(Z3, Wl + 2 * WS, wv, lane, c);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) zb.v[i] = s[1].v[i] * c[i];          // zb2
    acc.db[1] += cg_sum4(zb);
    cg_put(Z2, zb, lane, col);
    sm_lds_barrier();
    cg_outer(Z2, H1, wv, lane, acc.dW[1]);
    cg_gemm_t(Z2, Wl + 1 * WS, wv, lane, c);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) zb.v[i] = s[0].v[i] * c[i];          // zb1
    acc.db[0] += cg_sum4(zb);
    cg_put(Z1, zb, lane, col);
    sm_lds_barrier();
    cg_outer(Z1, U, wv, lane, acc.dW[0]);
    sm_lds_barrier();                                                   // the pass is over: its buffers may be rewritten
}

// the interior point [xt, t]: 1/2 |g_x|^2 + g_t and its parameter gradient
__device__ __forceinline__ void am_interior(const SmArgs& A, const float* Wl, const float* bl, const float* w3l, float* T,
                                            const float* __restrict__ xt, const float* __restrict__ t,
                                            const float* __restrict__ x0, const float* __restrict__ x1, int row0, int B, int d,
                                            int wv, int lane, int col, AmAcc& acc) {
    constexpr int TS = SM_ROWS * SM_LD, WS = SM_W * SM_LD;
    float* U = T; float* H1 = T + TS; float* H2 = T + 2 * TS; float* Z3 = T + 3 * TS; float* Z2 = T + 4 * TS; float* Z1 = T + 5 * TS;
    float* G3 = T + 6 * TS; float* G2 = T + 7 * TS; float* G1 = T + 8 * TS; float* WD = T + 9 * TS; float* D1 = T + 10 * TS;
    float* D2 = T + 11 * TS;
    const int nrows = B - row0;
    SmTile s[3], q[3], h3, hb1, hb2, dz1, dz2, tv;
    f32x4 c, cm[SM_MB];
    am_load(U, xt, t, 0.f, x0, x1, row0, B, d, lane, col);
    am_forward(A, Wl, bl, U, H1, H2, nrows, wv, lane, col, s, q, h3);
    (void)h3;
    const float w3 = w3l[col];
    // ---- the reverse sweep: g = grad_u s ----
#pragma unroll
    for (int i = 0; i < SM_V; ++i) tv.v[i] = s[2].v[i] * w3;                                 // g3
    cg_put(G3, tv, lane, col);
    sm_lds_barrier();
    cg_gemm_t(G3, Wl + 2 * WS, wv, lane, c);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) { hb2.v[i] = c[i]; tv.v[i] = s[1].v[i] * c[i]; }          // g2
    cg_put(G2, tv, lane, col);
    sm_lds_barrier();
    cg_gemm_t(G2, Wl + 1 * WS, wv, lane, c);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) { hb1.v[i] = c[i]; tv.v[i] = s[0].v[i] * c[i]; }          // g1
    cg_put(G1, tv, lane, col);
    sm_lds_barrier();
    cg_gemm_t(G1, Wl, wv, lane, c);                                                          // g = g1 W0: [g_x, g_t]
    {
        float ls = 0.f;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const float g = c[i];                                                            // 0 in rows beyond B (s_l = 0)
            ls += (col < d) ? 0.5f * g * g : (col == d ? g : 0.f);
            tv.v[i] = (col < d) ? g : ((col == d && sm_row(i, lane) < nrows) ? 1.f : 0.f);   // w = (g_x, 1)
        }
        acc.loss += ls;
    }
    cg_put(WD, tv, lane, col);
    sm_lds_barrier();
    // ---- the tangent of the chain along w ----
    sm_gemm(WD, Wl, wv, lane, cm);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) { dz1.v[i] = cm[0][i]; tv.v[i] = s[0].v[i] * cm[0][i]; }  // dh1
    cg_put(D1, tv, lane, col);
    sm_lds_barrier();
    sm_gemm(D1, Wl + 1 * WS, wv, lane, cm);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) { dz2.v[i] = cm[0][i]; tv.v[i] = s[1].v[i] * cm[0][i]; }  // dh2
    cg_put(D2, tv, lane, col);
    sm_lds_barrier();
    sm_gemm(D2, Wl + 2 * WS, wv, lane, cm);
    {
        float ds = 0.f;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            ds += s[2].v[i] * cm[0][i];                                                      // dh3
            tv.v[i] = w3 * q[2].v[i] * cm[0][i];                                             // zeta3
        }
        acc.dw3 += ds;
    }
    acc.db[2] += cg_sum4(tv);
    cg_put(Z3, tv, lane, col);
    sm_lds_barrier();
    cg_outer(G3, D2, wv, lane, acc.dW[2]);
    cg_outer(Z3, H2, wv, lane, acc.dW[2]);
    cg_gemm_t(Z3, Wl + 2 * WS, wv, lane, c);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) tv.v[i] = s[1].v[i] * c[i] + hb2.v[i] * q[1].v[i] * dz2.v[i];   // zeta2
    acc.db[1] += cg_sum4(tv);
    cg_put(Z2, tv, lane, col);
    sm_lds_barrier();
    cg_outer(G2, D1, wv, lane, acc.dW[1]);
    cg_outer(Z2, H1, wv, lane, acc.dW[1]);
    cg_gemm_t(Z2, Wl + 1 * WS, wv, lane, c);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) tv.v[i] = s[0].v[i] * c[i] + hb1.v[i] * q[0].v[i] * dz1.v[i];   // zeta1
    acc.db[0] += cg_sum4(tv);
    cg_put(Z1, tv, lane, col);
    sm_lds_barrier();
    cg_outer(G1, WD, wv, lane, acc.dW[0]);
    cg_outer(Z1, U, wv, lane, acc.dW[0]);
    sm_lds_barrier();                                                   // the pass is over
}

// x0, x1, xt [B, d] (xt null: the interpolant), t [B]; part [gridDim.x][P]: W0, b0, W1, b1, W2, b2, W3, b3 (as the caller's tensors), then the
// workgroup's share of sum_rows l
__global__ __launch_bounds__(256) void action_matching_grad(SmArgs A, int B, int d, const float* __restrict__ x0,
                                                         const float* __restrict__ x1, const float* __restrict__ xt,
                                                         const float* __restrict__ t, float* __restrict__ part, int P) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    constexpr int WS = SM_W * SM_LD;
    float* Wl = small_lds;                    // W0 (all d + 1 columns), W1, W2
    float* bl = Wl + 3 * WS;                  // b0, b1, b2
    float* w3l = bl + 3 * SM_W;               // W3[0][:]
    float* T = w3l + SM_W;                    // AM_TILES tile buffers
    float* red = T + AM_TILES * SM_ROWS * SM_LD;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int l = 0; l < 3; ++l) {
        const int in_l = A.dims[l], out_l = A.dims[l + 1];
        for (int e = tid; e < WS; e += 256) {
            const int r = e / SM_LD, k = e % SM_LD;
            Wl[l * WS + e] = (r < out_l && k < in_l) ? A.W[l][(size_t)r * in_l + k] : 0.f;
        }
        if (tid < SM_W) bl[l * SM_W + tid] = (tid < out_l) ? A.b[l][tid] : 0.f;
    }
    if (tid < SM_W) w3l[tid] = (tid < A.dims[3]) ? A.W[3][tid] : 0.f;
    __syncthreads();
    const int col = wv * 16 + (lane & 15);

    AmAcc acc;
    acc.dw3 = 0.f; acc.loss = 0.f;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        acc.db[l] = 0.f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc.dW[l][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int row0 = blockIdx.x * SM_ROWS; row0 < B; row0 += gridDim.x * SM_ROWS) {
        am_endpoint(A, Wl, bl, w3l, T, x0, 0.f, 1.f, row0, B, d, wv, lane, col, acc);
        am_endpoint(A, Wl, bl, w3l, T, x1, 1.f, -1.f, row0, B, d, wv, lane, col, acc);
        am_interior(A, Wl, bl, w3l, T, xt, t, x0, x1, row0, B, d, wv, lane, col, acc);
    }

    // ---- this workgroup's partial ----
    float* Pw = part + (size_t)blockIdx.x * P;
    int off = 0;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int in_l = A.dims[l], out_l = A.dims[l + 1];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * mb + 4 * (lane >> 4) + i;
                if (r < out_l && col < in_l) Pw[off + r * in_l + col] = acc.dW[l][mb][i];
            }
        }
        off += out_l * in_l;
        float bsum = acc.db[l];
        bsum += __shfl_xor(bsum, 16, 64);
        bsum += __shfl_xor(bsum, 32, 64);
        if (lane < 16 && col < out_l) Pw[off + col] = bsum;
        off += out_l;
    }
    {
        float wsum = acc.dw3;
        wsum += __shfl_xor(wsum, 16, 64);
        wsum += __shfl_xor(wsum, 32, 64);
        if (lane < 16 && col < A.dims[3]) Pw[off + col] = wsum;
        off += A.dims[3];
        float ls = acc.loss;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) ls += __shfl_xor(ls, o, 64);
        if (lane == 0) red[wv] = ls;
        __syncthreads();
        if (tid == 0) {
            Pw[off] = 0.f;                                              // db3
            Pw[off + 1] = ((red[0] + red[1]) + red[2]) + red[3];
        }
    }
}

extern "C" int cfm_action_matching_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                            const float* x0, const float* x1, const float* xt, const float* t, int B,
                                            float* loss, float* const* dW, float* const* db, void* ws, void* stream) {
    int d; SmArgs A;
    if (!x0 || !x1 || !t || !loss || !dW || !db || !ws) return CFM_EINVAL;
    int rc = grad_check(W, b, dims, n_layers, B, &d, &A);
    if (rc) return rc;
    for (int l = 0; l < 4; ++l) if (!W[l] || !b[l]) return CFM_EINVAL;
    CgOut O;
    const int P = cg_out(dims, dW, db, &O) + 1;                         // the loss term behind the gradient
    if (P < 1) return CFM_EINVAL;
    return cg_launch<action_matching_grad, 128 * 1024>(am_lds_bytes, (hipStream_t)stream, B, (float*)ws, P, A, O, 1.f / (float)B, loss,
                                                       A, B, d, x0, x1, xt, t, (float*)ws, P);
}
