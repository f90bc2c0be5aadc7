// grad_field.h — the action-matching field v = grad_x s(x, t) of a 4-layer SELU potential on the 16-row tile engine
// (included by ode.hip; SmTile, sm_gemm, cg_gemm_t, sm_rowsum, selu_f, selu_slope come from small_field.h).
//
// Counterpart of GradModel (torchcfm/models/models.py:24-32) over MLP(dim, out_dim=1, time_varying=True): the action net
// has dims [d + 1, n1, n2, n3, 1].  With z_l the pre-activations, s_l = selu'(z_l), q_l = selu''(z_l) (= s_l for
// z <= 0, else 0: PyTorch's double backward of elu_backward):
//   forward   z1 = W0[:, :d] x + t W0[:, d] + b0,  h1 = selu(z1),  z2 = W1 h1 + b1,  h2 = selu(z2),  z3 = W2 h2 + b2
//             (sm_field's code: the same ascending-k MFMA chain, the same bias / time-column epilogue, so every z sits
//             on the side of every kink that MLP.forward_hip of the action net puts it on)
//   reverse   g3 = s3 * W3[0, :] (no product),  hb2 = g3 W2,  g2 = s2 * hb2,  hb1 = g2 W1,  g1 = s1 * hb1,
//             v = g1 W0[:, :d]                  (b3 and the value s are never needed)
//   Laplacian per direction k < d (tangents of the whole chain; hb1, hb2 kept from the primal):
//             dz1 = W0[:, k],  dh1 = s1 * dz1,  dz2 = W1 dh1,  dh2 = s2 * dz2,  dz3 = W2 dh2,
//             dg3 = W3[0, :] * q3 * dz3,  dg2 = s2 * (dg3 W2) + hb2 * q2 * dz2,  dg1 = s1 * (dg2 W1) + hb1 * q1 * dz1,
//             lap += dg1 . W0[:, k]             (two forward and two pull-back products; one sm_rowsum at the end)
// Six dependent product rounds per evaluation against sm_field's four.
//
// The pull-backs (products with W_l, not W_l^T) read the staged matrices BY COLUMNS (cg_gemm_t); no transposed copies
// are staged.  ds_read_b32 is served in two groups of 32 lanes over 32 banks: the row-fragment read of sm_gemm
// (address 68 fr + fk + 4 j, fr = lane & 15, fk = lane >> 4) puts fr and fr + 8 on one bank, the column read
// (68 (fk + 4 j) + 16 wave + fr) puts 12 of a group's 16 columns on a bank of the other k row: both are two-way, two LDS
// cycles per group, so a transposed copy buys no read cycles.  It would cost 34 KiB of LDS (112 KiB per workgroup: one
// workgroup per CU instead of the two whose MFMA and SELU phases overlap) and half as much staging traffic again per
// launch.  The LDS image is therefore exactly the plain field's (small_lds_bytes(1, 2, rowsum)).
//
// Padding: columns beyond a layer's width and rows of a partial tile beyond B carry s_l = q_l = 0, so every cotangent
// and tangent tile is zero there and the Laplacian's row sums see nothing of them (as in sm_field_aug).
#pragma once

enum { FIELD_MLP = 0, FIELD_GRAD = 1 };      // field kind of the small-field kernels: MLP([x, t]) / grad_x of a potential

constexpr size_t gf_lds_bytes = small_lds_bytes(1, 2, true);
static_assert(gf_lds_bytes == 79872, "the gradient-field kernels: the plain field's image, two workgroups per CU");

__device__ __forceinline__ void gf_put(float* __restrict__ buf, const SmTile& v, int lane, int col) {
#pragma unroll
    for (int i = 0; i < SM_V; ++i) buf[sm_row(i, lane) * SM_LD + col] = v.v[i];
}

// v(t, y) for the tile (C layout in, C layout out, columns >= d are 0); LAP: lap = sum_k d v_k / d y_k per row, in every
// lane that holds the row.  nrows: rows of the tile below B.  The primal is the same code for both LAP: the same v bits.
template <bool LAP>
__device__ __forceinline__ SmTile gf_field(const SmTile& y, float t, const SmArgs& A, int d, float* Abuf0, float* Abuf1,
                                           const float* Wl, const float* bl, const float* wt, int nrows, float* red,
                                           int wv, int lane, SmTile& lap) {
    constexpr int WS = SM_W * SM_LD;
    const int col = wv * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) Abuf0[sm_row(i, lane) * SM_LD + col] = (col < d) ? y.v[i] : 0.f;
    sm_lds_barrier();
    SmTile s[3], q[3], tv;
    f32x4 c[SM_MB];
    float* src = Abuf0; float* dst = Abuf1;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int N = A.dims[l + 1];
        sm_gemm(src, Wl + l * WS, wv, lane, c);
        const float bv = (col < N) ? bl[l * SM_W + col] : 0.f;
        const float wtc = (l == 0 && col < N) ? wt[col] : 0.f;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            float z = c[i >> 2][i & 3] + bv;
            if (l == 0) z = fmaf(t, wtc, z);
            const float sl = (col < N && sm_row(i, lane) < nrows) ? selu_slope(z) : 0.f;
            s[l].v[i] = sl;
            q[l].v[i] = z > 0.f ? 0.f : sl;
            tv.v[i] = (col < N) ? selu_f(z) : 0.f;
        }
        if (l < 2) {
            gf_put(dst, tv, lane, col);
            sm_lds_barrier();
            float* tmp = src; src = dst; dst = tmp;
        }
    }
    // the reverse sweep: Abuf1 (read last by layer 1), Abuf0 (by layer 2), Abuf1 again; a barrier after every write
    const float w3 = (col < A.dims[3]) ? Wl[3 * WS + col] : 0.f;                            // W3[0][col]
    SmTile hb1, hb2, out;
#pragma unroll
    for (int i = 0; i < SM_V; ++i) tv.v[i] = s[2].v[i] * w3;                                // g3
    gf_put(Abuf1, tv, lane, col);
    sm_lds_barrier();
    cg_gemm_t(Abuf1, Wl + 2 * WS, wv, lane, c[0]);                                          // g3 W2
#pragma unroll
    for (int i = 0; i < SM_V; ++i) { hb2.v[i] = c[0][i]; tv.v[i] = s[1].v[i] * c[0][i]; }   // g2
    gf_put(Abuf0, tv, lane, col);
    sm_lds_barrier();
    cg_gemm_t(Abuf0, Wl + 1 * WS, wv, lane, c[0]);                                          // g2 W1
#pragma unroll
    for (int i = 0; i < SM_V; ++i) { hb1.v[i] = c[0][i]; tv.v[i] = s[0].v[i] * c[0][i]; }   // g1
    gf_put(Abuf1, tv, lane, col);
    sm_lds_barrier();
    cg_gemm_t(Abuf1, Wl, wv, lane, c[0]);                                                   // g1 W0[:, :d]
#pragma unroll
    for (int i = 0; i < SM_V; ++i) out.v[i] = (col < d) ? c[0][i] : 0.f;
    if constexpr (LAP) {
        SmTile acc;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) acc.v[i] = 0.f;
        for (int k = 0; k < d; ++k) {
            // (the first write of a direction goes to Abuf0: its last readers, g2 W1 of the primal or dg3 W2 of the
            // direction before, sit behind a barrier; Abuf1's readers are behind the barrier that follows this write)
            const float w0 = (col < A.dims[1]) ? Wl[col * SM_LD + k] : 0.f;                 // W0[col][k] = dz1
            SmTile dz2;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) tv.v[i] = s[0].v[i] * w0;                        // dh1
            gf_put(Abuf0, tv, lane, col);
            sm_lds_barrier();
            sm_gemm(Abuf0, Wl + 1 * WS, wv, lane, c);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) { dz2.v[i] = c[0][i]; tv.v[i] = s[1].v[i] * c[0][i]; }   // dh2
            gf_put(Abuf1, tv, lane, col);
            sm_lds_barrier();
            sm_gemm(Abuf1, Wl + 2 * WS, wv, lane, c);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) tv.v[i] = w3 * q[2].v[i] * c[0][i];              // dg3
            gf_put(Abuf0, tv, lane, col);
            sm_lds_barrier();
            cg_gemm_t(Abuf0, Wl + 2 * WS, wv, lane, c[0]);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) tv.v[i] = s[1].v[i] * c[0][i] + hb2.v[i] * q[1].v[i] * dz2.v[i];   // dg2
            gf_put(Abuf1, tv, lane, col);
            sm_lds_barrier();
            cg_gemm_t(Abuf1, Wl + 1 * WS, wv, lane, c[0]);
#pragma unroll
            for (int i = 0; i < SM_V; ++i)
                acc.v[i] = fmaf(w0, s[0].v[i] * c[0][i] + hb1.v[i] * q[0].v[i] * w0, acc.v[i]);               // dg1 . W0[:, k]
        }
        lap = sm_rowsum(acc, red, wv, lane);
    } else {
        (void)red; (void)lap; (void)q; (void)hb1; (void)hb2;
    }
    return out;
}
