// icnn.hip — input-convex networks for optimal transport (Makkuva et al. 2020): the transport map of an ICNN, the three
// means of compute_w2 and the two training steps of the minimax objective (cfm_icnn_f32).
//
// Counterpart of runner/src/models/components/icnn_model.py and of ICNNLitModule.training_step / compute_w2
// (runner/src/models/icnn_module.py:98-135, 229-245).  A net of L hidden layers of width H on d inputs, written by levels
// l = 1 .. L (sp = Softplus(beta 1, threshold 20), s_l = sp'(a_l), q_l = sp''(a_l) = s_l (1 - s_l)):
//     a_1 = IN_0 x + b_0,   a_l = HZ_{l-2} h_{l-1} + IN_{l-1} x + b_{l-1},   h_l = sp(a_l),   out = wz . h_L + wx . x
// with IN_0 = Wzs[0], IN_j = Wxs[j-1] ([H, d], each with its bias), HZ_j = Wzs[j+1] ([H, H], bias-free), wz = Wzs[L],
// wx = Wxs[L-1].  Four kernels of one tile engine (small_field.h: 16-row tiles, wave w owns columns 16w .. 16w+15):
//   icnn_transport  p = grad net(x): forward, then the reverse sweep  hb_L = wz, ab_l = s_l * hb_l, hb_{l-1} = ab_l HZ_{l-2},
//                   grad = (((ab_L IN_{L-1}) + ab_{L-1} IN_{L-2}) + .. + ab_1 IN_0) + wx
//   icnn_values     net f: the row sums of f(x), f(p), y.p, |x|^2, |y|^2 (W2), or f(p), y.p and w = grad f(p) - y (the g-step)
//   icnn_f_grad     net f: two plain backwards, at x with cotangent +1 and at p with cotangent -1
//                       dwz += c h_L, dwx += c x, and per level  dIN_{l-1} += ab_l^T x, db_{l-1} += ab_l, dHZ_{l-2} += ab_l^T h_{l-1}
//   icnn_g_grad     net g: the parameter gradient of the derivative of g along the fixed w at y.  Tangent forward
//                       da_1 = IN_0 w, dh_l = s_l * da_l, da_l = HZ_{l-2} dh_{l-1} + IN_{l-1} w;   dwz += dh_L, dwx += w
//                   then, from l = L down, the reverse sweep (ab_l, hb_l as above) together with the second-order one
//                       zeta_l = s_l * ht_l + q_l * da_l * hb_l   (ht_L = 0),   ht_{l-1} = zeta_l HZ_{l-2}
//                       dIN_{l-1} += ab_l^T w + zeta_l^T y,  db_{l-1} += zeta_l,  dHZ_{l-2} += ab_l^T dh_{l-1} + zeta_l^T h_{l-1}
// Launches per operation, whatever B and d:  TRANSPORT 1 (icnn_transport);  W2 3 (transport of g at y, values, reduce);
// F_STEP 3 (transport of g at y, f_grad, reduce);  G_STEP 4 (transport of g at y, values, g_grad, reduce).  p and w travel
// between the launches through the caller's p and w outputs, so only ONE net's weights are ever LDS-resident.
//
// Layout decisions:
//  * All seven matrices are staged as [64][SM_LD] with zero fill, the skip matrices too (K = d is zero-filled to the
//    full 16 k-steps of sm_gemm): one GEMM, one column-read pull-back (cg_gemm_t) and one outer product (cg_outer) serve
//    every product of the unit, and x may be as wide as a whole tile (ICNN_MAX_DIM = 64; there is no time column).
//  * Nine tile buffers: X, W, H1..H3, D0, D1, A, Z.  The g-step keeps q_l * da_l in registers and only two dh tiles: dh_l
//    sits in D[(l-1) & 1], and the one tile that a later one overwrote (dh_1 when L = 4, by dh_3) is kept in registers
//    and put again when its level comes.  A and Z are rewritten at every level, behind a barrier of their own.
//  * Weight gradients, bias sums and loss terms are kept across the workgroup's tiles; every workgroup writes one partial
//    (8 loss terms, then the gradient) and icnn_reduce adds the partials in workgroup order, scales by 1 / B once and adds
//    the penalty reg sum_W |relu(-W)|^2 / 2 over the Wzs with its gradient -reg relu(-W): the same bits run to run, no
//    float atomics.
#include "cfm_common.h"
#include "small_field.h"
#include "ode_envelope.h"

#define ICNN_MAX_DIM 64
#define IC_MAXL 4
#define IC_TILES 9
#define IC_TERMS 8                                      // loss terms in front of a partial: f(x), f(p), y.p, |x|^2, |y|^2, 3 spare
#define IC_PMAX (IC_TERMS + IC_MAXL * SM_W * ICNN_MAX_DIM + IC_MAXL * SM_W + (IC_MAXL - 1) * SM_W * SM_W + SM_W + ICNN_MAX_DIM)
#define IC_NSEG (3 * IC_MAXL + 1)

static_assert(ICNN_MAX_DIM == CFM_ICNN_MAX_DIM && ICNN_MAX_DIM <= SM_W, "x occupies one tile");
constexpr int IC_WS = SM_W * SM_LD, IC_TS = SM_ROWS * SM_LD;
constexpr size_t ic_lds_bytes = sizeof(float) * ((2 * IC_MAXL - 1) * IC_WS + (IC_MAXL + 2) * SM_W + IC_TILES * IC_TS + 4 * IC_TERMS);
static_assert(ic_lds_bytes == 162688, "the ICNN kernels: seven matrices, six vectors, nine tiles, the term scratch");
static_assert(ic_lds_bytes <= 160 * 1024, "the LDS of one gfx950 compute unit");

extern "C" size_t cfm_icnn_ws_bytes_internal(int B) {
    if (B <= 0) return 0;
    const size_t tiles = ((size_t)B + SM_ROWS - 1) / SM_ROWS;
    const size_t g = tiles < CG_MAXGRID ? tiles : CG_MAXGRID;
    return sizeof(float) * g * IC_PMAX;
}

struct IcNet { const float* IN[IC_MAXL]; const float* b[IC_MAXL]; const float* HZ[IC_MAXL - 1]; const float* wz; const float* wx; };
struct IcDims { int d, H, L, B; };
struct IcLds { float* IN; float* HZ; float* bl; float* wz; float* wx; float* T; float* red; };
struct IcFw { SmTile s[IC_MAXL], q[IC_MAXL], hL; };
struct IcAcc {
    f32x4 dIN[IC_MAXL][4], dHZ[IC_MAXL - 1][4];        // cg_outer's layout
    float db[IC_MAXL], dwz, dwx;
};
// the gradient's segments in a partial's order (IN, b, HZ, wz, wx): where each goes, its length, and the weight whose
// penalty it carries (null: none)
struct IcSeg { float* out[IC_NSEG]; const float* pen[IC_NSEG]; int n[IC_NSEG]; int nseg; };

__device__ __forceinline__ IcLds ic_carve(float* lds) {
    IcLds S;
    S.IN = lds; S.HZ = S.IN + IC_MAXL * IC_WS; S.bl = S.HZ + (IC_MAXL - 1) * IC_WS; S.wz = S.bl + IC_MAXL * SM_W;
    S.wx = S.wz + SM_W; S.T = S.wx + SM_W; S.red = S.T + IC_TILES * IC_TS;
    return S;
}

// one net -> LDS, zero padded; levels beyond L are not staged and never read
__device__ __forceinline__ void ic_stage(const IcNet& N, const IcDims& D, const IcLds& S, int tid) {
    for (int l = 0; l < D.L; ++l) {
        for (int e = tid; e < IC_WS; e += 256) {
            const int r = e / SM_LD, k = e % SM_LD;
            S.IN[l * IC_WS + e] = (r < D.H && k < D.d) ? N.IN[l][(size_t)r * D.d + k] : 0.f;
            if (l < D.L - 1) S.HZ[l * IC_WS + e] = (r < D.H && k < D.H) ? N.HZ[l][(size_t)r * D.H + k] : 0.f;
        }
        if (tid < SM_W) S.bl[l * SM_W + tid] = (tid < D.H) ? N.b[l][tid] : 0.f;
    }
    if (tid < SM_W) {
        S.wz[tid] = (tid < D.H) ? N.wz[tid] : 0.f;
        S.wx[tid] = (tid < D.d) ? N.wx[tid] : 0.f;
    }
    __syncthreads();
}

// rows row0.. of src [B, d] into a tile buffer; columns beyond d and rows beyond B are zero.  No barrier.
__device__ __forceinline__ void ic_load(float* buf, const float* __restrict__ src, int row0, const IcDims& D, int lane, int col) {
#pragma unroll
    for (int i = 0; i < SM_V; ++i) {
        const int r = sm_row(i, lane), gr = row0 + r;
        buf[r * SM_LD + col] = (gr < D.B && col < D.d) ? src[(size_t)gr * D.d + col] : 0.f;
    }
}

// sp, sp', sp'' of torch's Softplus(beta 1, threshold 20) without overflow: e = exp(-|z|) <= 1, r = 1 / (1 + e);
// sigma(|z|) = r and sigma(-|z|) = e r, so 1 - sigma is never formed by a subtraction
__device__ __forceinline__ void ic_softplus(float z, float& h, float& s, float& q) {
    const float e = expf(-fabsf(z)), r = 1.f / (1.f + e), er = e * r;
    const bool big = z > 20.f;
    h = big ? z : fmaxf(z, 0.f) + log1pf(e);
    s = big ? 1.f : (z >= 0.f ? r : er);
    q = big ? 0.f : r * er;
}

// the forward of one tile from X (T0 or any buffer): h_1 .. h_{L-1} into T2 .. T4, s_l, q_l and h_L in registers.
// s_l, q_l are zero outside [rows below B, H columns], so every derivative tile is zero there.
template <int NL>
__device__ __forceinline__ void ic_forward(const IcLds& S, const IcDims& D, const float* X, int nrows, int wv, int lane, int col,
                                           IcFw& fw) {
#pragma unroll
    for (int l = 0; l < IC_MAXL; ++l) {
        if (l < NL) {
            f32x4 c[SM_MB], c2[SM_MB];
            sm_gemm(X, S.IN + l * IC_WS, wv, lane, c);
            if (l > 0) sm_gemm(S.T + (1 + l) * IC_TS, S.HZ + (l - 1) * IC_WS, wv, lane, c2);
            const float bv = S.bl[l * SM_W + col];
            SmTile hv;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                const float zx = c[0][i] + bv;
                const float z = l > 0 ? c2[0][i] + zx : zx;
                float h, s, q;
                ic_softplus(z, h, s, q);
                const bool live = col < D.H && sm_row(i, lane) < nrows;
                fw.s[l].v[i] = live ? s : 0.f;
                fw.q[l].v[i] = live ? q : 0.f;
                hv.v[i] = live ? h : 0.f;
            }
            if (l < NL - 1) {
                cg_put(S.T + (2 + l) * IC_TS, hv, lane, col);
                sm_lds_barrier();
            } else {
                fw.hL = hv;
            }
        }
    }
}

// this lane's share of sum_rows out: wz . h_L + wx . x over its elements (h_L and X are zero in dead rows and columns)
__device__ __forceinline__ float ic_value(const IcLds& S, const float* X, const IcFw& fw, int lane, int col) {
    const float wz = S.wz[col], wx = S.wx[col];
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < SM_V; ++i) v += wz * fw.hL.v[i] + wx * X[sm_row(i, lane) * SM_LD + col];
    return v;
}

// the reverse sweep with cotangent cs: grad (C layout, columns = inputs) = cs grad_x out; GRAD: the plain backward's
// parameter sums as well.  ab_l alternates between T7 and T8: a buffer is rewritten two barriers after its last read.
// Ends without a barrier: the caller closes the pass.
template <bool GRAD, int NL>
__device__ __forceinline__ void ic_reverse(const IcLds& S, const IcDims& D, const float* X, const IcFw& fw, float cs, int wv,
                                           int lane, int col, SmTile& grad, IcAcc* acc) {
    SmTile hb;
    const float wz = cs * S.wz[col];
#pragma unroll
    for (int i = 0; i < SM_V; ++i) hb.v[i] = wz;
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = IC_MAXL - 1; l >= 0; --l) {
        if (l < NL) {
            SmTile ab;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) ab.v[i] = fw.s[l].v[i] * hb.v[i];
            float* AB = S.T + (7 + (l & 1)) * IC_TS;
            cg_put(AB, ab, lane, col);
            sm_lds_barrier();
            if constexpr (GRAD) {
                acc->db[l] += cg_sum4(ab);
                cg_outer(AB, X, wv, lane, acc->dIN[l]);
                if (l > 0) cg_outer(AB, S.T + (1 + l) * IC_TS, wv, lane, acc->dHZ[l - 1]);
            }
            f32x4 c;
            cg_gemm_t(AB, S.IN + l * IC_WS, wv, lane, c);
            g += c;
            if (l > 0) {
                cg_gemm_t(AB, S.HZ + (l - 1) * IC_WS, wv, lane, c);
#pragma unroll
                for (int i = 0; i < SM_V; ++i) hb.v[i] = c[i];
            }
        }
    }
    const float wx = cs * S.wx[col];
#pragma unroll
    for (int i = 0; i < SM_V; ++i) grad.v[i] = g[i] + wx;
    if constexpr (GRAD) {
        float hs = 0.f, xs = 0.f;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) { hs += fw.hL.v[i]; xs += X[sm_row(i, lane) * SM_LD + col]; }
        acc->dwz = fmaf(cs, hs, acc->dwz);
        acc->dwx = fmaf(cs, xs, acc->dwx);
    }
}

__device__ __forceinline__ void ic_store(float* __restrict__ dst, const SmTile& v, int row0, const IcDims& D, int lane, int col) {
#pragma unroll
    for (int i = 0; i < SM_V; ++i) {
        const int gr = row0 + sm_row(i, lane);
        if (gr < D.B && col < D.d) dst[(size_t)gr * D.d + col] = v.v[i];
    }
}

// the workgroup's loss terms, each added over lanes then waves in a fixed order, into Pw[0 .. IC_TERMS)
__device__ __forceinline__ void ic_write_terms(const IcLds& S, float (&t)[IC_TERMS], float* Pw, int tid, int lane, int wv) {
#pragma unroll
    for (int k = 0; k < IC_TERMS; ++k) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) t[k] += __shfl_xor(t[k], o, 64);
        if (lane == 0) S.red[wv * IC_TERMS + k] = t[k];
    }
    __syncthreads();
    if (tid < IC_TERMS) Pw[tid] = ((S.red[tid] + S.red[IC_TERMS + tid]) + S.red[2 * IC_TERMS + tid]) + S.red[3 * IC_TERMS + tid];
}

__device__ __forceinline__ void ic_zero(IcAcc& acc) {
    acc.dwz = 0.f; acc.dwx = 0.f;
#pragma unroll
    for (int l = 0; l < IC_MAXL; ++l) {
        acc.db[l] = 0.f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            acc.dIN[l][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (l < IC_MAXL - 1) acc.dHZ[l][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// the workgroup's gradient behind the terms, in IcSeg's order
__device__ __forceinline__ void ic_write_grad(const IcAcc& acc, const IcDims& D, float* Pw, int lane, int col) {
    int off = IC_TERMS;
#pragma unroll
    for (int l = 0; l < IC_MAXL; ++l) {
        if (l < D.L) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 16 * mb + 4 * (lane >> 4) + i;
                    if (r < D.H && col < D.d) Pw[off + r * D.d + col] = acc.dIN[l][mb][i];
                }
            }
            off += D.H * D.d;
        }
    }
#pragma unroll
    for (int l = 0; l < IC_MAXL; ++l) {
        if (l < D.L) {
            float bsum = acc.db[l];
            bsum += __shfl_xor(bsum, 16, 64);
            bsum += __shfl_xor(bsum, 32, 64);
            if (lane < 16 && col < D.H) Pw[off + col] = bsum;
            off += D.H;
        }
    }
#pragma unroll
    for (int l = 0; l < IC_MAXL - 1; ++l) {
        if (l < D.L - 1) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 16 * mb + 4 * (lane >> 4) + i;
                    if (r < D.H && col < D.H) Pw[off + r * D.H + col] = acc.dHZ[l][mb][i];
                }
            }
            off += D.H * D.H;
        }
    }
    float zs = acc.dwz, xs = acc.dwx;
    zs += __shfl_xor(zs, 16, 64); zs += __shfl_xor(zs, 32, 64);
    xs += __shfl_xor(xs, 16, 64); xs += __shfl_xor(xs, 32, 64);
    if (lane < 16 && col < D.H) Pw[off + col] = zs;
    off += D.H;
    if (lane < 16 && col < D.d) Pw[off + col] = xs;
}

// p [B, d] = grad net(x)
template <int NL>
__global__ __launch_bounds__(256) void icnn_transport(IcNet N, IcDims D, const float* __restrict__ x, float* __restrict__ p) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    const IcLds S = ic_carve(small_lds);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = wv * 16 + (lane & 15);
    ic_stage(N, D, S, tid);
    for (int row0 = blockIdx.x * SM_ROWS; row0 < D.B; row0 += gridDim.x * SM_ROWS) {
        IcFw fw; SmTile g;
        ic_load(S.T, x, row0, D, lane, col);
        sm_lds_barrier();
        ic_forward<NL>(S, D, S.T, D.B - row0, wv, lane, col, fw);
        ic_reverse<false, NL>(S, D, S.T, fw, 1.f, wv, lane, col, g, nullptr);
        ic_store(p, g, row0, D, lane, col);
        sm_lds_barrier();                                               // the pass is over: its buffers may be rewritten
    }
}

// net f.  x given (W2): terms f(x), f(p), y.p, |x|^2, |y|^2.  x null (the g-step): terms f(p), y.p, and w = grad f(p) - y
template <int NL>
__global__ __launch_bounds__(256) void icnn_values(IcNet N, IcDims D, const float* __restrict__ x, const float* __restrict__ y,
                                                const float* __restrict__ p, float* __restrict__ w, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    const IcLds S = ic_carve(small_lds);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = wv * 16 + (lane & 15);
    ic_stage(N, D, S, tid);
    float t[IC_TERMS];
#pragma unroll
    for (int k = 0; k < IC_TERMS; ++k) t[k] = 0.f;
    float* Y = S.T + IC_TS;
    for (int row0 = blockIdx.x * SM_ROWS; row0 < D.B; row0 += gridDim.x * SM_ROWS) {
        IcFw fw;
        if (x) {
            ic_load(S.T, x, row0, D, lane, col);
            sm_lds_barrier();
            ic_forward<NL>(S, D, S.T, D.B - row0, wv, lane, col, fw);
            t[0] += ic_value(S, S.T, fw, lane, col);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) { const float v = S.T[sm_row(i, lane) * SM_LD + col]; t[3] += v * v; }
            sm_lds_barrier();
        }
        ic_load(S.T, p, row0, D, lane, col);
        ic_load(Y, y, row0, D, lane, col);
        sm_lds_barrier();
        ic_forward<NL>(S, D, S.T, D.B - row0, wv, lane, col, fw);
        t[1] += ic_value(S, S.T, fw, lane, col);
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            const float yv = Y[sm_row(i, lane) * SM_LD + col];
            t[2] += yv * S.T[sm_row(i, lane) * SM_LD + col];
            t[4] += yv * yv;
        }
        if (w) {
            SmTile g;
            ic_reverse<false, NL>(S, D, S.T, fw, 1.f, wv, lane, col, g, nullptr);
#pragma unroll
            for (int i = 0; i < SM_V; ++i) g.v[i] -= Y[sm_row(i, lane) * SM_LD + col];
            ic_store(w, g, row0, D, lane, col);
        }
        sm_lds_barrier();
    }
    ic_write_terms(S, t, part + (size_t)blockIdx.x * IC_PMAX, tid, lane, wv);
}

// net f: the terms f(x), f(p) and the gradient of sum_rows f(x) - f(p)
template <int NL>
__global__ __launch_bounds__(256) void icnn_f_grad(IcNet N, IcDims D, const float* __restrict__ x, const float* __restrict__ p,
                                                float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    const IcLds S = ic_carve(small_lds);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = wv * 16 + (lane & 15);
    ic_stage(N, D, S, tid);
    float t[IC_TERMS];
#pragma unroll
    for (int k = 0; k < IC_TERMS; ++k) t[k] = 0.f;
    IcAcc acc;
    ic_zero(acc);
    for (int row0 = blockIdx.x * SM_ROWS; row0 < D.B; row0 += gridDim.x * SM_ROWS) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            IcFw fw; SmTile g;
            ic_load(S.T, pass == 0 ? x : p, row0, D, lane, col);
            sm_lds_barrier();
            ic_forward<NL>(S, D, S.T, D.B - row0, wv, lane, col, fw);
            t[pass] += ic_value(S, S.T, fw, lane, col);
            ic_reverse<true, NL>(S, D, S.T, fw, pass == 0 ? 1.f : -1.f, wv, lane, col, g, &acc);
            sm_lds_barrier();
        }
    }
    float* Pw = part + (size_t)blockIdx.x * IC_PMAX;
    ic_write_terms(S, t, Pw, tid, lane, wv);
    ic_write_grad(acc, D, Pw, lane, col);
}

// net g: the gradient of sum_rows w . grad_y g(y), w fixed
template <int NL>
__global__ __launch_bounds__(256) void icnn_g_grad(IcNet N, IcDims D, const float* __restrict__ y, const float* __restrict__ w,
                                                float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    const IcLds S = ic_carve(small_lds);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = wv * 16 + (lane & 15);
    ic_stage(N, D, S, tid);
    IcAcc acc;
    ic_zero(acc);
    float* Y = S.T; float* Wd = S.T + IC_TS; float* A = S.T + 7 * IC_TS; float* Z = S.T + 8 * IC_TS;
    for (int row0 = blockIdx.x * SM_ROWS; row0 < D.B; row0 += gridDim.x * SM_ROWS) {
        IcFw fw;
        SmTile qd[IC_MAXL], dh0, hb, ht;                                // qd_l = q_l * da_l
        ic_load(Y, y, row0, D, lane, col);
        ic_load(Wd, w, row0, D, lane, col);
        sm_lds_barrier();
        ic_forward<NL>(S, D, Y, D.B - row0, wv, lane, col, fw);
        // ---- the tangent of the chain along w: dh_l into D[(l-1) & 1] = T5, T6 ----
#pragma unroll
        for (int l = 0; l < IC_MAXL; ++l) {
            if (l < NL) {
                f32x4 c[SM_MB], c2[SM_MB];
                sm_gemm(Wd, S.IN + l * IC_WS, wv, lane, c);
                if (l > 0) sm_gemm(S.T + (5 + ((l - 1) & 1)) * IC_TS, S.HZ + (l - 1) * IC_WS, wv, lane, c2);
                SmTile dh;
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    const float dal = l > 0 ? c2[0][i] + c[0][i] : c[0][i];
                    qd[l].v[i] = fw.q[l].v[i] * dal;
                    dh.v[i] = fw.s[l].v[i] * dal;
                }
                if (l == 0) dh0 = dh;
                if (l < NL - 1) {
                    cg_put(S.T + (5 + (l & 1)) * IC_TS, dh, lane, col);
                    sm_lds_barrier();
                } else {
                    acc.dwz += cg_sum4(dh);
                }
            }
        }
        {
            float xs = 0.f;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) xs += Wd[sm_row(i, lane) * SM_LD + col];
            acc.dwx += xs;
        }
        // ---- the reverse sweep and the second-order reverse, level by level ----
        const float wz = S.wz[col];
#pragma unroll
        for (int i = 0; i < SM_V; ++i) { hb.v[i] = wz; ht.v[i] = 0.f; }
#pragma unroll
        for (int l = IC_MAXL - 1; l >= 0; --l) {
            if (l < NL) {
                SmTile ab, zt;
#pragma unroll
                for (int i = 0; i < SM_V; ++i) {
                    ab.v[i] = fw.s[l].v[i] * hb.v[i];
                    zt.v[i] = fw.s[l].v[i] * ht.v[i] + qd[l].v[i] * hb.v[i];
                }
                cg_put(A, ab, lane, col);
                cg_put(Z, zt, lane, col);
                if (l == 1 && NL == IC_MAXL) cg_put(S.T + 5 * IC_TS, dh0, lane, col);   // dh_1, which dh_3 overwrote
                sm_lds_barrier();
                acc.db[l] += cg_sum4(zt);
                cg_outer(A, Wd, wv, lane, acc.dIN[l]);
                cg_outer(Z, Y, wv, lane, acc.dIN[l]);
                if (l > 0) {
                    f32x4 c;
                    cg_outer(A, S.T + (5 + ((l - 1) & 1)) * IC_TS, wv, lane, acc.dHZ[l - 1]);
                    cg_outer(Z, S.T + (1 + l) * IC_TS, wv, lane, acc.dHZ[l - 1]);
                    cg_gemm_t(A, S.HZ + (l - 1) * IC_WS, wv, lane, c);
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) hb.v[i] = c[i];
                    cg_gemm_t(Z, S.HZ + (l - 1) * IC_WS, wv, lane, c);
#pragma unroll
                    for (int i = 0; i < SM_V; ++i) ht.v[i] = c[i];
                }
                sm_lds_barrier();                                       // A, Z (and at l = 0 the pass's buffers) may be rewritten
            }
        }
    }
    ic_write_grad(acc, D, part + (size_t)blockIdx.x * IC_PMAX, lane, col);
}

// losses[3] and the gradient from the partials, added in workgroup order.  op 1: W2 (w2, f_loss, g_loss); 2, 3: the step's
// (loss, its data term, its penalty).  P = IC_TERMS for W2, IC_TERMS + the gradient's length for a step.
__global__ __launch_bounds__(256) void icnn_reduce(const float* __restrict__ part, int nparts, int P, IcSeg G, float scale, float reg,
                                                int op, float* __restrict__ losses) {
    __shared__ float term[IC_TERMS];
    __shared__ float pen[256];
    const int tid = threadIdx.x;
    int p = blockIdx.x * 256 + tid;
    float sum = 0.f;
    if (p < P) {
        for (int g = 0; g < nparts; ++g) sum += part[(size_t)g * IC_PMAX + p];
    }
    if (p >= IC_TERMS && p < P) {
        int e = p - IC_TERMS;
        for (int k = 0; k < G.nseg; ++k) {
            if (e >= 0 && e < G.n[k]) {
                float v = sum * scale;
                if (G.pen[k] && reg > 0.f) v -= reg * fmaxf(-G.pen[k][e], 0.f);
                G.out[k][e] = v;
            }
            e -= G.n[k];
        }
    }
    if (blockIdx.x != 0) return;
    if (tid < IC_TERMS) term[tid] = sum;
    float ps = 0.f;
    if (reg > 0.f) {
        for (int k = 0; k < G.nseg; ++k) {
            if (G.pen[k]) {
                for (int e = tid; e < G.n[k]; e += 256) { const float r = fmaxf(-G.pen[k][e], 0.f); ps += r * r; }
            }
        }
    }
    pen[tid] = ps;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) pen[tid] += pen[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float fx = term[0], fp = term[1], yp = term[2];
        if (op == CFM_ICNN_W2) {
            losses[0] = ((((fp - fx) - yp) + 0.5f * term[3]) + 0.5f * term[4]) * scale;
            losses[1] = (fx - fp) * scale;
            losses[2] = (fp - yp) * scale;
        } else {
            const float data = (op == CFM_ICNN_F_STEP ? fx - fp : fp - yp) * scale;
            const float penalty = reg > 0.f ? reg * (0.5f * pen[0]) : 0.f;
            losses[0] = data + penalty;
            losses[1] = data;
            losses[2] = penalty;
        }
    }
}

// ---- host side ----
static bool ic_net(const cfm_icnn_net& n, int L, IcNet* N) {
    if (!n.bz0) return false;
    for (int l = 0; l <= L; ++l) if (!n.Wz[l]) return false;
    for (int l = 0; l < L; ++l) if (!n.Wx[l]) return false;
    for (int l = 0; l < L - 1; ++l) if (!n.bx[l]) return false;
    N->IN[0] = n.Wz[0]; N->b[0] = n.bz0;
    for (int l = 1; l < IC_MAXL; ++l) { N->IN[l] = l < L ? n.Wx[l - 1] : nullptr; N->b[l] = l < L ? n.bx[l - 1] : nullptr; }
    for (int l = 0; l < IC_MAXL - 1; ++l) N->HZ[l] = l < L - 1 ? n.Wz[l + 1] : nullptr;
    N->wz = n.Wz[L]; N->wx = n.Wx[L - 1];
    return true;
}

// the gradient outputs of a net in a partial's order; the number of floats, or -1 when one is missing
static int ic_seg(const cfm_icnn_net& n, int d, int H, int L, IcSeg* G) {
    if (!n.dbz0) return -1;
    for (int l = 0; l <= L; ++l) if (!n.dWz[l]) return -1;
    for (int l = 0; l < L; ++l) if (!n.dWx[l]) return -1;
    for (int l = 0; l < L - 1; ++l) if (!n.dbx[l]) return -1;
    int k = 0, total = 0;
    auto add = [&](float* out, const float* pen, int len) { G->out[k] = out; G->pen[k] = pen; G->n[k] = len; ++k; total += len; };
    add(n.dWz[0], n.Wz[0], H * d);
    for (int l = 1; l < L; ++l) add(n.dWx[l - 1], nullptr, H * d);
    add(n.dbz0, nullptr, H);
    for (int l = 1; l < L; ++l) add(n.dbx[l - 1], nullptr, H);
    for (int l = 1; l < L; ++l) add(n.dWz[l], n.Wz[l], H * H);
    add(n.dWz[L], n.Wz[L], H);
    add(n.dWx[L - 1], nullptr, d);
    G->nseg = k;
    for (; k < IC_NSEG; ++k) { G->out[k] = nullptr; G->pen[k] = nullptr; G->n[k] = 0; }
    return total;
}

// the tile launches of one operation, the depth compile-time: no branch stands between an MFMA chain and its reader
template <int NL>
static int ic_launch(const cfm_icnn_call& c, const IcDims& D, const IcNet& F, const IcNet& Gn) {
    hipStream_t s = (hipStream_t)c.stream;
    constexpr int LIM = 160 * 1024;
    float* part = (float*)c.ws;
    int rc;
    const int grid = small_grid<icnn_transport<NL>, LIM>(c.B, CG_MAXGRID);
    if (grid < 0) return CFM_EINVAL;
    if (c.op == CFM_ICNN_TRANSPORT) {
        hipLaunchKernelGGL(icnn_transport<NL>, dim3(grid), dim3(256), ic_lds_bytes, s, F, D, c.x, c.p);
        return cfm_status();
    }
    // the dynamic-LDS limit of the kernels this operation launches, and of no other
    if (c.op != CFM_ICNN_F_STEP && small_grid<icnn_values<NL>, LIM>(c.B, CG_MAXGRID) < 0) return CFM_EINVAL;
    if (c.op == CFM_ICNN_F_STEP && small_grid<icnn_f_grad<NL>, LIM>(c.B, CG_MAXGRID) < 0) return CFM_EINVAL;
    if (c.op == CFM_ICNN_G_STEP && small_grid<icnn_g_grad<NL>, LIM>(c.B, CG_MAXGRID) < 0) return CFM_EINVAL;
    hipLaunchKernelGGL(icnn_transport<NL>, dim3(grid), dim3(256), ic_lds_bytes, s, Gn, D, c.y, c.p);
    if ((rc = cfm_status())) return rc;
    if (c.op == CFM_ICNN_W2) {
        hipLaunchKernelGGL(icnn_values<NL>, dim3(grid), dim3(256), ic_lds_bytes, s, F, D, c.x, c.y, (const float*)c.p, (float*)nullptr, part);
    } else if (c.op == CFM_ICNN_F_STEP) {
        hipLaunchKernelGGL(icnn_f_grad<NL>, dim3(grid), dim3(256), ic_lds_bytes, s, F, D, c.x, (const float*)c.p, part);
    } else {
        hipLaunchKernelGGL(icnn_values<NL>, dim3(grid), dim3(256), ic_lds_bytes, s, F, D, (const float*)nullptr, c.y, (const float*)c.p, c.w, part);
        if ((rc = cfm_status())) return rc;
        hipLaunchKernelGGL(icnn_g_grad<NL>, dim3(grid), dim3(256), ic_lds_bytes, s, Gn, D, c.y, (const float*)c.w, part);
    }
    return cfm_status();
}

extern "C" int cfm_icnn_f32(const cfm_icnn_call* call) {
    if (!call || call->size != sizeof(cfm_icnn_call)) return CFM_EINVAL;
    const cfm_icnn_call& c = *call;
    if (c.op < CFM_ICNN_TRANSPORT || c.op > CFM_ICNN_G_STEP) return CFM_EINVAL;
    if (c.L < 2 || c.L > IC_MAXL || c.dimh < 1 || c.dimh > SM_W || c.d < 1 || c.d > ICNN_MAX_DIM || c.B < 1) return CFM_EINVAL;
    if (!(c.reg >= 0.f) || !cfm_ode_fused_internal()) return CFM_EINVAL;
    const IcDims D{c.d, c.dimh, c.L, c.B};
    IcNet F, Gn;
    IcSeg seg;
    seg.nseg = 0;
    for (int k = 0; k < IC_NSEG; ++k) { seg.out[k] = nullptr; seg.pen[k] = nullptr; seg.n[k] = 0; }
    int P = IC_TERMS;
    if (!ic_net(c.f, c.L, &F) || !c.p) return CFM_EINVAL;
    if (c.op == CFM_ICNN_TRANSPORT) {
        if (!c.x) return CFM_EINVAL;
    } else {
        if (!ic_net(c.g, c.L, &Gn) || !c.y || !c.losses || !c.ws) return CFM_EINVAL;
        if (c.op != CFM_ICNN_G_STEP && !c.x) return CFM_EINVAL;
        if (c.op == CFM_ICNN_G_STEP && !c.w) return CFM_EINVAL;
        if (c.op != CFM_ICNN_W2) {
            const int n = ic_seg(c.op == CFM_ICNN_F_STEP ? c.f : c.g, c.d, c.dimh, c.L, &seg);
            if (n < 0) return CFM_EINVAL;
            P += n;
        }
    }
    // ---- everything above is host arithmetic: a declining call has made no HIP call ----
    int rc = c.L == 2 ? ic_launch<2>(c, D, F, Gn) : c.L == 3 ? ic_launch<3>(c, D, F, Gn) : ic_launch<4>(c, D, F, Gn);
    if (rc || c.op == CFM_ICNN_TRANSPORT) return rc;
    const int tiles = (c.B + SM_ROWS - 1) / SM_ROWS, grid = tiles < CG_MAXGRID ? tiles : CG_MAXGRID;
    hipStream_t s = (hipStream_t)c.stream;
    float* part = (float*)c.ws;
    hipLaunchKernelGGL(icnn_reduce, dim3((P + 255) / 256), dim3(256), 0, s, (const float*)part, grid, P, seg, 1.f / (float)c.B, c.reg, c.op,
                       c.losses);
    return cfm_status();
}
