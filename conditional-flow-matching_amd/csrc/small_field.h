// small_field.h — the 16-row tile engine of the fused small-field kernels of ode.hip, sde_small.h, cnf_grad.h and action_grad.h
// and icnn.hip (SmTile, sm_gemm, cg_gemm_t, cg_put, cg_outer, sm_field, sm_field_aug, weights staged in LDS), its LDS byte count, envelope check, launch helper.
#pragma once
#include "cfm_common.h"

// =====================================================================================
// Fused Dormand-Prince step for SMALL vector fields (4 linear layers, every width <= 64:
// the reference's 2-D tutorials and single-cell models, MLP(dim, w=64)).
//
// The layer-per-kernel driver of ode.hip spends ~31 launches and one host read-back per step
// attempt: 266 us per step at B = 8192, d = 50, w = 64 where the arithmetic is ~20 us.
// Rows are independent inside a step (only the error norm couples them), so here ONE persistent
// kernel does the whole adaptive solve: a workgroup keeps the four weight matrices in LDS (68 KB)
// and owns a 16-row tile (SM_MB = 1: B = 8192 -> 512 workgroups, two per CU, so one workgroup's
// MFMA phase overlaps the other's SELU epilogue; measured 3.46 ms against 3.87 ms for 32-row tiles
// with two accumulator chains per wave and one workgroup per CU), holds x and k1..k7 of its tile
// in MFMA accumulator layout in registers, and runs the six stage evaluations back to back.  Wave w
// owns output columns 16w..16w+15: a v_mfma_f32_16x16x4_f32 accumulator chain with the same
// ascending-k fp32 fma chain and epilogue as mlp_layer: bitwise the same field values.  The
// accept / reject decision and the next step size are taken ON THE DEVICE by every workgroup from
// the same all-reduced error norm (same fp32 controller as ode.hip's host loop); the host launches
// once and reads the step counters back.
// =====================================================================================
#define SM_W 64
#define SM_LD 68     // row stride = 4 (mod 64): fragment reads (row = lane & 15, k = lane >> 4) hit 64 distinct banks
#define SM_MB 1      // 16-row blocks per tile = independent MFMA accumulator chains per wave
#define SM_ROWS (16 * SM_MB)
#define SM_V (4 * SM_MB)   // tile floats per lane: element i -> row sm_row(i, lane), column 16 * wave + (lane & 15)

typedef float f32x4 __attribute__((ext_vector_type(4)));
struct SmTile { float v[SM_V]; };
__device__ __forceinline__ int sm_row(int i, int lane) { return 16 * (i >> 2) + 4 * (lane >> 4) + (i & 3); }

// same SELU as mlp.hip (bitwise)
__device__ __forceinline__ float selu_f(float x) {
    return x > 0.f ? 1.0507009873554805f * x : (1.0507009873554805f * 1.6732632423543772f) * expm1f(x);
}
struct SmArgs { const float* W[4]; const float* b[4]; int dims[5]; };

// Workgroup barrier that orders LDS traffic only: global stores of the tile (trajectory rows) stay in
// flight across it instead of being drained (s_waitcnt vmcnt(0)) the way __syncthreads() would
__device__ __forceinline__ void sm_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// one layer on the tile: out(C layout) = A[SM_ROWS x 64] * W_l[64 x 64]^T, this wave's 16 columns
__device__ __forceinline__ void sm_gemm(const float* __restrict__ Abuf, const float* __restrict__ Wl, int wv, int lane,
                                        f32x4 (&c)[SM_MB]) {
#pragma unroll
    for (int m = 0; m < SM_MB; ++m) c[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fk = lane >> 4;
    const float* ap = Abuf + fr * SM_LD + fk;
    const float* bp = Wl + (wv * 16 + fr) * SM_LD + fk;
    // every layer runs the full 16 k-steps (rows / columns beyond the layer's width are zero in both operands,
    // and fma(0, 0, acc) leaves acc alone), fully unrolled: all operand reads are in flight before the
    // first MFMA issues, then the accumulator chain(s) run back to back in ascending k
    float a[SM_MB][SM_W / 4], b[SM_W / 4];
#pragma unroll
    for (int j = 0; j < SM_W / 4; ++j) {
#pragma unroll
        for (int m = 0; m < SM_MB; ++m) a[m][j] = ap[16 * m * SM_LD + 4 * j];
        b[j] = bp[4 * j];
    }
#pragma unroll
    for (int j = 0; j < SM_W / 4; ++j) {
#pragma unroll
        for (int m = 0; m < SM_MB; ++m) c[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][j], b[j], c[m], 0, 0, 0);
    }
}

// out(C layout) = A[16 x 64] * M, M = the staged [64][SM_LD] matrix read by columns: out[r][n] = sum_k A[r][k] M[k][n]
__device__ __forceinline__ void cg_gemm_t(const float* __restrict__ Abuf, const float* __restrict__ M, int wv, int lane,
                                          f32x4& c) {
    c = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fk = lane >> 4;
    const float* ap = Abuf + fr * SM_LD + fk;
    const float* bp = M + fk * SM_LD + wv * 16 + fr;
    float a[SM_W / 4], b[SM_W / 4];
#pragma unroll
    for (int j = 0; j < SM_W / 4; ++j) { a[j] = ap[4 * j]; b[j] = bp[4 * j * SM_LD]; }
#pragma unroll
    for (int j = 0; j < SM_W / 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
}

// ---- what the gradient kernels (small_grad.hip, icnn.hip) add to the engine: a C-layout tile into a buffer, the
// weight-gradient product over the 16 rows of a tile, a lane's column sum; and their grid cap ----
#define CG_MAXGRID 256                                 // workgroups (= partial gradients) at most
static_assert(SM_MB == 1, "the gradient kernel is written for one 16-row block per tile");
__device__ __forceinline__ void cg_put(float* __restrict__ buf, const SmTile& v, int lane, int col) {
#pragma unroll
    for (int i = 0; i < SM_V; ++i) buf[sm_row(i, lane) * SM_LD + col] = v.v[i];
}

// acc[mb](C layout of block mb) += Z^T H over the 16 rows of the tile: element i of lane -> dW[16 mb + 4 (lane >> 4) + i]
// [16 wave + (lane & 15)], dW[n][k] = sum_r Z[r][n] H[r][k]
__device__ __forceinline__ void cg_outer(const float* __restrict__ Zbuf, const float* __restrict__ Hbuf, int wv, int lane,
                                         f32x4 (&acc)[4]) {
    const int fr = lane & 15, fk = lane >> 4;
    const float* zp = Zbuf + fk * SM_LD + fr;
    const float* hp = Hbuf + fk * SM_LD + wv * 16 + fr;
    float a[4][SM_ROWS / 4], b[SM_ROWS / 4];
#pragma unroll
    for (int j = 0; j < SM_ROWS / 4; ++j) {
        b[j] = hp[4 * j * SM_LD];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) a[mb][j] = zp[4 * j * SM_LD + 16 * mb];
    }
#pragma unroll
    for (int j = 0; j < SM_ROWS / 4; ++j) {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mb][j], b[j], acc[mb], 0, 0, 0);
    }
}

__device__ __forceinline__ float cg_sum4(const SmTile& v) { return (v.v[0] + v.v[1]) + (v.v[2] + v.v[3]); }

// f(t, y) for the tile; y arrives in C layout, the result leaves in C layout (columns >= d are 0)
__device__ __forceinline__ SmTile sm_field(const SmTile& y, float t, const SmArgs& A, int d, float* Abuf0,
                                           float* Abuf1, const float* Wl, const float* bl, const float* wt,
                                           int wv, int lane) {
    const int col = wv * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < SM_V; ++i) Abuf0[sm_row(i, lane) * SM_LD + col] = (col < d) ? y.v[i] : 0.f;
    sm_lds_barrier();
    SmTile acc;
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
            if (l < 3) v = selu_f(v);
            acc.v[i] = (col < N) ? v : 0.f;
        }
        if (l < 3) {
#pragma unroll
            for (int i = 0; i < SM_V; ++i) dst[sm_row(i, lane) * SM_LD + col] = acc.v[i];
            sm_lds_barrier();
            float* tmp = src; src = dst; dst = tmp;
        }
    }
    return acc;
}

// ---- CNF augmentation: v = f(t, x) and its divergence on the tile ----------------------------------------------
// J = W3 diag(s3) W2 diag(s2) W1 diag(s1) W0[:, :d],  s_l = selu'(z_l) at the layer's pre-activation.
//   AUG_EXACT: tr J = sum_k (J e_k)_k.  T1 = s1 * W0[:, k] needs no product; T2 = s2 * (W1 T1), T3 = s3 * (W2 T2);
//              only row k of W3 is needed, so the last product is a dot product: 2 GEMMs per direction.
//   AUG_HUTCH: eps^T J eps (eps fixed per solve): T1 = s1 * (W0 eps), T2, T3, Ju = W3 T3: 4 GEMMs.
// The lane that owns (row, col) of z_l owns (row, col) of every tangent tile, so s_l stays in its registers; the
// tangent tiles take the primal's LDS staging buffers in the same strict alternation (a barrier after every write).
enum { AUG_NONE = 0, AUG_EXACT = 1, AUG_HUTCH = 2 };

// selu'(z) as PyTorch's elu_backward takes it: scale for z > 0, scale * alpha * exp(z) otherwise (z = 0 included)
__device__ __forceinline__ float selu_slope(float z) {
    return z > 0.f ? 1.0507009873554805f : (1.0507009873554805f * 1.6732632423543772f) * expf(z);
}

// per-row sum of a C-layout tile over its 64 columns: 16 lanes of a wave (butterfly: every lane gets the same bits),
// then the 4 waves in a fixed order through red[4][SM_ROWS]; every lane gets the sums of its SM_V rows
__device__ __forceinline__ SmTile sm_rowsum(SmTile p, float* red, int wv, int lane) {
#pragma unroll
    for (int i = 0; i < SM_V; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) p.v[i] += __shfl_xor(p.v[i], o, 64);
    }
    if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < SM_V; ++i) red[wv * SM_ROWS + sm_row(i, lane)] = p.v[i];
    }
    sm_lds_barrier();
    SmTile r;
#pragma unroll
    for (int i = 0; i < SM_V; ++i) {
        const int row = sm_row(i, lane);
        r.v[i] = ((red[row] + red[SM_ROWS + row]) + red[2 * SM_ROWS + row]) + red[3 * SM_ROWS + row];
    }
    return r;
}

// f(t, y) exactly as sm_field (bitwise the same v), plus div (per row, in every lane holding the row).
// eps: the probe tile (C layout, zero outside [rows, d]); nrows: rows of the tile below B (the rest stay zero in
// every tangent tile).
template <int MODE>
__device__ __forceinline__ SmTile sm_field_aug(const SmTile& y, float t, const SmArgs& A, int d, float* Abuf0,
                                               float* Abuf1, const float* Wl, const float* bl, const float* wt,
                                               const SmTile& eps, int nrows, float* red, int wv, int lane,
                                               SmTile& div) {
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
    SmTile q;
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
#pragma unroll
            for (int i = 0; i < SM_V; ++i) q.v[i] = fmaf(w3, (col < N3) ? sl[2].v[i] * c[i >> 2][i & 3] : 0.f, q.v[i]);
        }
    }
    div = sm_rowsum(q, red, wv, lane);
    return acc;
}

// weights -> LDS, zero padded to [4][64][SM_LD]; biases; the time column of layer 0
__device__ __forceinline__ void sm_stage_weights(const SmArgs& A, int d, float* Wl, float* bl, float* wt, int tid) {
    for (int l = 0; l < 4; ++l) {
        const int in_l = A.dims[l], out_l = A.dims[l + 1];
        const int K = (l == 0) ? d : in_l;
        for (int e = tid; e < SM_W * SM_LD; e += 256) {
            const int r = e / SM_LD, k = e % SM_LD;
            Wl[l * SM_W * SM_LD + e] = (r < out_l && k < K) ? A.W[l][(size_t)r * in_l + k] : 0.f;
        }
        if (tid < SM_W) bl[l * SM_W + tid] = (tid < out_l) ? A.b[l][tid] : 0.f;
    }
    if (tid < SM_W) wt[tid] = (tid < A.dims[1]) ? A.W[0][(size_t)tid * A.dims[0] + d] : 0.f;
}

// ---- host side ----  Dynamic LDS of a kernel that stages `nets` fields (weights, biases, time column each) and
// carves `tiles` tile buffers behind them, plus sm_rowsum's scratch: the one place the layout's size is written down.
constexpr size_t small_lds_bytes(int nets, int tiles, bool rowsum) {
    return sizeof(float) * ((size_t)nets * (4 * SM_W * SM_LD + 4 * SM_W + SM_W) + (size_t)tiles * SM_ROWS * SM_LD +
                            (rowsum ? 4 * SM_ROWS : 0));
}
static_assert(small_lds_bytes(1, 2, false) == 79616, "plain one-net kernels");
static_assert(small_lds_bytes(1, 2, true) == 79872, "augmented one-net kernels");
static_assert(small_lds_bytes(2, 2, false) == 150528, "the two-net SDE kernels");

// What the tile engine needs of a field: 4 layers, [x, t] -> dx, no width above SM_W.  0, or CFM_EINVAL.  The entry
// points add what is theirs alone: the ODE / CNF entries d + 1 <= SM_W, and each its lower bounds.  d_out may be null.
static inline int small_envelope(const int* dims, int n_layers, int* d_out) {
    if (!dims || n_layers != 4) return CFM_EINVAL;
    const int d = dims[4];
    if (dims[0] != d + 1 || d > SM_W) return CFM_EINVAL;
    for (int l = 1; l <= 3; ++l) if (dims[l] > SM_W) return CFM_EINVAL;
    if (d_out) *d_out = d;
    return 0;
}

static inline SmArgs small_args(const float* const* W, const float* const* b, const int* dims) {
    SmArgs A;
    for (int l = 0; l < 4; ++l) { A.W[l] = W[l]; A.b[l] = b[l]; }
    for (int l = 0; l < 5; ++l) A.dims[l] = dims[l];
    return A;
}

// Grid of a tile kernel over B rows (<= cap workgroups); raises KERNEL's dynamic-LDS limit once per device (-1: failed)
template <auto KERNEL, int LIMIT>
static inline int small_grid(int B, int cap = 4096) {
    const int raised = cfm_once_per_device([] {
        return hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LIMIT) == hipSuccess ? 1 : -1;
    });
    if (raised < 0) return -1;
    const int tiles = (B + SM_ROWS - 1) / SM_ROWS;
    return tiles < cap ? tiles : cap;
}
