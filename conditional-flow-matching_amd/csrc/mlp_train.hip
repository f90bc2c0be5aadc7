// mlp_train.hip — training step of the MLP vector field on fp32 MFMA (gfx950): backward GEMMs with
// fused SELU' epilogue, bias gradients, fused multi-tensor Adam.
//
// Replaces, for torchcfm.models.MLP (torchcfm/models/models.py:10-21), what autograd + torch.optim.Adam
// execute in the reference's training loop (examples/images/cifar10/train_cifar10.py:141-151:
// vt = net(...); loss = mean((vt - ut)^2); loss.backward(); optim.step()):
//
//   forward (training)   the same mlp_layer kernels as inference (mlp.hip), keeping h_l = selu(z_l) (the
//                        next wgrad's operand) and z_l (selu'(z) = scale * alpha * exp(z): recovering it from
//                        h as h + scale * alpha cancels catastrophically for saturated units — measured
//                        1.7e-3 relative error on the first layer's gradient at d = 784)
//   dgrad                dz_{l-1} = (dz_l . W_l) * selu'(z_{l-1})     [B,N] x [N,K]  ("NN")
//   wgrad                dW_l = dz_l^T . h_{l-1}                      [N,B] x [B,K]  ("TN"), the
//                        contraction runs over the batch: split over S batch chunks so that a 512 x 512
//                        gradient still fills the chip, partial sums reduced in a fixed order
//                        (deterministic, no atomics)
//   bias grad            db_l = column sums of dz_l, accumulated by the wgrad workgroups of the first tile column
//                        from the dz tile they stage anyway; every split-K partial of the pass (weights and
//                        biases of all layers) is reduced by ONE table-driven launch
//   Adam                 one launch for every parameter tensor of the model (pointer table), torch.optim.Adam
//                        arithmetic (lerp / addcmul / addcdiv order, bias corrections as Python doubles)
//
// All GEMMs are v_mfma_f32_32x32x2_f32 (exact fp32, 157 TFLOP/s peak) on the shared tile engine of gemm_core.h:
// K-major LDS tiles whatever the operand's storage order (k-contiguous operands are transposed on the way in),
// two stages, ds_read_b64 fragments.
//
// Host side: ONE driver for the regression step (one net) and the SF2M step (two nets of equal sizes per launch) —
// mlp_train_forward, mlp_backward_impl, launch_gemm (one product) and launch_gemm_pair (dgrad + wgrad of a layer) all take
// `nets`; carve_train_ws is the one statement of the CFM_OP_MLP_TRAIN workspace layout.
#include "cfm_common.h"
#include "gemm_core.h"

#define SELU_SCALE 1.0507009873554805f
#define SELU_ALPHA 1.6732632423543772f

// selu'(z)
__device__ __forceinline__ float selu_grad(float z) {
    return z > 0.f ? SELU_SCALE : (SELU_SCALE * SELU_ALPHA) * expf(z);
}

enum { EPI_PLAIN = 0, EPI_SELU_GRAD = 1 };

// C[M,N] (+ epilogue) = A[M,Kc] . B[Kc,N], contraction over [k_begin, k_end) of this workgroup's split, on the
// shared tile engine (gemm_core.h).
//   A_KMAJOR = false: A(i,k) = A[i * lda + k]      true: A(i,k) = A[k * lda + i]
//   B_KMAJOR = false: B(k,j) = Bm[j * ldb + k]     true: B(k,j) = Bm[k * ldb + j]
// grid: x = tiles_m * tiles_n (XCD-remapped), y = split index s; split s writes C + s * split_stride.
// the arguments of one product (a kernel argument of the single and of the paired launch)
struct GemmArgs {
    const float* A; int lda; const float* Bm; int ldb; float* C; int ldc; size_t split_stride;
    const float* H;            // EPI_SELU_GRAD: pre-activations [M, ldc]
    int M, N, Kc, k_chunk, tiles_n;
    float* colsum;             // A_KMAJOR: sum_k A(i, k) per split -> colsum[s * M + i]
    const float* tvec;         // A_KMAJOR: weights t[k] of a second column sum
    float* tsum;               //   sum_k A(i, k) t[k] per split -> tsum[s * M + i]
};

template <int BM, int BN, int BK, bool A_KMAJOR, bool B_KMAJOR, int EPI, bool VECA, bool VECB>
__device__ __forceinline__ void gemm_tile(float* __restrict__ lds, unsigned lid, int split, const GemmArgs& G) {
    using Core = GemmCore<BM, BN, BK, A_KMAJOR, B_KMAJOR, VECA, VECB>;
    const float* __restrict__ A = G.A; const float* __restrict__ Bm = G.Bm; float* __restrict__ C = G.C;
    const float* __restrict__ H = G.H; float* __restrict__ colsum = G.colsum; const float* __restrict__ tvec = G.tvec;
    float* __restrict__ tsum = G.tsum;
    const int lda = G.lda, ldb = G.ldb, ldc = G.ldc, M = G.M, N = G.N, Kc = G.Kc, k_chunk = G.k_chunk, tiles_n = G.tiles_n;
    const size_t split_stride = G.split_stride;
    const int tm = lid / tiles_n, tn = lid % tiles_n;
    const int row0 = tm * BM, col0 = tn * BN;
    const int tid = threadIdx.x;
    const int k_begin = split * k_chunk;
    const int k_end = (k_begin + k_chunk < Kc) ? k_begin + k_chunk : Kc;

    // bias gradient rides along: the workgroups of the first tile column add up their A tile (dz) over k, from the
    // K-major LDS stage every step (same ascending-k order as before)
    // (the time column of a time-varying first layer is not part of the GEMM operand: its gradient
    //  dW[:, d] = sum_b dz[b, :] t[b] is a second, weighted column sum of the same tile)
    const bool do_colsum = A_KMAJOR && colsum != nullptr && tn == 0 && tid < BM;
    const bool do_tsum = do_colsum && tvec != nullptr && tsum != nullptr;
    float csum = 0.f, wsum = 0.f;
    auto post = [&](const float* As, int k0) {
        if (A_KMAJOR && do_colsum) {
            if (do_tsum) {
#pragma unroll
                for (int kk = 0; kk < BK; ++kk) {
                    const float a = As[kk * Core::LDA + tid];
                    csum += a;
                    wsum = fmaf(a, (k0 + kk < k_end) ? tvec[k0 + kk] : 0.f, wsum);
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < BK; ++kk) csum += As[kk * Core::LDA + tid];
            }
        }
    };
    Core g;
    g.zero();
    g.run(lds, A, lda, row0, M, Bm, ldb, col0, N, k_begin, k_end, post);
    if (A_KMAJOR && do_colsum && row0 + tid < M) {
        colsum[(size_t)split * M + row0 + tid] = csum;
        if (do_tsum) tsum[(size_t)split * M + row0 + tid] = wsum;
    }

    constexpr int EU = Core::EU, EM = Core::EM, ER = Core::ER;
    float* Cs = C + (size_t)split * split_stride;
    const int gc = col0 + Core::col_lo();
    const bool pair = EU == 2 && (ldc & 1) == 0 && gc + 1 < N;
#pragma unroll
    for (int m = 0; m < EM; ++m) {
#pragma unroll
        for (int r = 0; r < ER; ++r) {
            const int gr = row0 + Core::row_of(m, r);
            if (gr >= M || gc >= N) continue;
            float v[2];
#pragma unroll
            for (int u = 0; u < EU; ++u) v[u] = g.at(m, u, r);
            if (EPI == EPI_SELU_GRAD) {
                if (pair) {
                    const float2 h = *reinterpret_cast<const float2*>(H + (size_t)gr * ldc + gc);
                    v[0] *= selu_grad(h.x); v[EU - 1] *= selu_grad(h.y);
                } else {
#pragma unroll
                    for (int u = 0; u < EU; ++u) if (gc + u < N) v[u] *= selu_grad(H[(size_t)gr * ldc + gc + u]);
                }
            }
            float* po = Cs + (size_t)gr * ldc + gc;
            if (pair) *reinterpret_cast<float2*>(po) = make_float2(v[0], v[EU - 1]);
            else {
#pragma unroll
                for (int u = 0; u < EU; ++u) if (gc + u < N) po[u] = v[u];
            }
        }
    }
}


// grid: x = tiles_m * tiles_n (XCD-remapped), y = split index s; split s writes C + s * split_stride.
template <int BM, int BN, int BK, bool A_KMAJOR, bool B_KMAJOR, int EPI, bool VECA, bool VECB>
__global__ __launch_bounds__(256) void gemm_f32_mfma(GemmArgs G) {
    using Core = GemmCore<BM, BN, BK, A_KMAJOR, B_KMAJOR, VECA, VECB>;
    __shared__ __attribute__((aligned(16))) float lds[Core::LDS_FLOATS];
    gemm_tile<BM, BN, BK, A_KMAJOR, B_KMAJOR, EPI, VECA, VECB>(lds, cfm_xcd_remap(blockIdx.x, gridDim.x), (int)blockIdx.y, G);
}

// dgrad and wgrad of ONE layer in one launch (round 6): both read dz_l and nothing of each other.  A 1-D grid: the
// dgrad tiles first (their contraction is the long one: 512 - 784 against 256 per wgrad split), then tiles x splits of
// wgrad; 64 x 64 x 32 tiles and 16-byte loads on both (the launcher falls back to two launches otherwise).  Same tile
// routine, same bits.  14 -> 11 launches per C3 model step.
__global__ __launch_bounds__(256) void gemm_pair_f32_mfma(GemmArgs D, int tiles_d, GemmArgs Wg, int tiles_w, int splits_w) {
    using CoreD = GemmCore<64, 64, 32, false, true, true, true>;
    using CoreW = GemmCore<64, 64, 32, true, true, true, true>;
    constexpr int LDSF = CoreD::LDS_FLOATS > CoreW::LDS_FLOATS ? CoreD::LDS_FLOATS : CoreW::LDS_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    const int b = (int)blockIdx.x;
    if (b < tiles_d) {
        gemm_tile<64, 64, 32, false, true, EPI_SELU_GRAD, true, true>(lds, cfm_xcd_remap((unsigned)b, (unsigned)tiles_d), 0, D);
    } else {
        const int q = b - tiles_d;
        gemm_tile<64, 64, 32, true, true, EPI_PLAIN, true, true>(lds, cfm_xcd_remap((unsigned)(q % tiles_w), (unsigned)tiles_w), q / tiles_w, Wg);
    }
}

// The same launches for TWO nets of equal sizes (the flow and the score net of cfm_mlp_sf2m_step_f32): x-blocks
// [0, per_net) are net 0's grid, [per_net, 2 per_net) net 1's, each net's workgroups in the order, on the tile and
// with the split they have when that net runs alone — the same tile routine, the same bits as one launch per net.
struct GemmArgs2 { GemmArgs net[2]; };
template <int BM, int BN, int BK, bool A_KMAJOR, bool B_KMAJOR, int EPI, bool VECA, bool VECB>
__global__ __launch_bounds__(256) void gemm_f32_mfma_two(GemmArgs2 T, unsigned per_net) {
    using Core = GemmCore<BM, BN, BK, A_KMAJOR, B_KMAJOR, VECA, VECB>;
    __shared__ __attribute__((aligned(16))) float lds[Core::LDS_FLOATS];
    const unsigned second = blockIdx.x >= per_net ? 1u : 0u;
    const GemmArgs G = T.net[second];
    gemm_tile<BM, BN, BK, A_KMAJOR, B_KMAJOR, EPI, VECA, VECB>(lds, cfm_xcd_remap(blockIdx.x - second * per_net, per_net), (int)blockIdx.y, G);
}
__global__ __launch_bounds__(256) void gemm_pair_f32_mfma_two(GemmArgs2 D, int tiles_d, GemmArgs2 Wg, int tiles_w, int splits_w) {
    using CoreD = GemmCore<64, 64, 32, false, true, true, true>;
    using CoreW = GemmCore<64, 64, 32, true, true, true, true>;
    constexpr int LDSF = CoreD::LDS_FLOATS > CoreW::LDS_FLOATS ? CoreD::LDS_FLOATS : CoreW::LDS_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    const int per_net = tiles_d + tiles_w * splits_w;
    const int second = (int)blockIdx.x >= per_net ? 1 : 0;
    const int b = (int)blockIdx.x - second * per_net;
    if (b < tiles_d) {
        const GemmArgs G = D.net[second];
        gemm_tile<64, 64, 32, false, true, EPI_SELU_GRAD, true, true>(lds, cfm_xcd_remap((unsigned)b, (unsigned)tiles_d), 0, G);
    } else {
        const int q = b - tiles_d;
        const GemmArgs G = Wg.net[second];
        gemm_tile<64, 64, 32, true, true, EPI_PLAIN, true, true>(lds, cfm_xcd_remap((unsigned)(q % tiles_w), (unsigned)tiles_w), q / tiles_w, G);
    }
}

// out[e] = sum_s partial[s * stride + e] in split order (deterministic), for every tensor of the table
// (all weight and bias gradients of a backward pass in ONE launch)
struct ReduceJob { const float* partial; float* out; unsigned long long stride, n; int S, cols, ld_out, pad; };   // cols > 0: out[(e / cols) * ld_out + e % cols]
#define MLP_MAX_LAYERS 16
struct ReduceTable { ReduceJob job[2 * MLP_MAX_LAYERS + 2]; int count; };

__global__ __launch_bounds__(256) void reduce_splits_multi(ReduceTable T) {
    for (int q = blockIdx.y; q < T.count; q += gridDim.y) {
        const ReduceJob J = T.job[q];
        if (J.pad == 1) {
            // ONE number out of S partials (the loss: one partial per workgroup of the last layer, ~ 800 of them): lane l
            // adds partials l, l + 64, ... in order, then a fixed tree over the wave — deterministic, and not 800
            // dependent loads in one thread
            if (blockIdx.x == 0 && threadIdx.x < 64) {
                float v = 0.f;
                for (int s2 = threadIdx.x; s2 < J.S; s2 += 64) v += J.partial[s2];
                v = wave_sum_f(v);
                if (threadIdx.x == 0) J.out[0] = v;
            }
            continue;
        }
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < J.n; e += (size_t)gridDim.x * 256) {
            float v = J.partial[e];
            // (8 partials in flight per thread, added in split order: the same sums as one load at a time)
            for (int s0 = 1; s0 < J.S; s0 += 8) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = (s0 + u < J.S) ? J.partial[(size_t)(s0 + u) * J.stride + e] : 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) if (s0 + u < J.S) v += t[u];
            }
            if (J.cols > 0) J.out[(e / (unsigned)J.cols) * (size_t)J.ld_out + (e % (unsigned)J.cols)] = v;
            else J.out[e] = v;
        }
    }
}

#define MLP_MAX_SPLITS 32
#define MLP_LOSS_PARTIALS 4096
extern "C" size_t cfm_mlp_train_ws_bytes_internal(int B, int maxw, int max_params) {
    // two [B, maxw] gradient buffers + a pool of split-K partials (weights, biases, the time column) that holds FOUR
    // layers of the largest size at MLP_MAX_SPLITS splits (callers pass the largest dims[l] * dims[l+1]): every layer of
    // a net of up to four, so such a net is reduced by one launch at the end.  A deeper net at a batch that splits every
    // layer 32 ways fills it: the backward then reduces what it has collected and reuses the pool from its start
    // (one more small launch per refill, the same bits).
    // (+ MLP_LOSS_PARTIALS loss partials for cfm_mlp_regression_step_f32: one per workgroup of the last layer)
    return sizeof(float) * ((size_t)2 * B * maxw + (size_t)MLP_MAX_SPLITS * ((size_t)max_params + maxw) * 4) + 4 * MLP_LOSS_PARTIALS;
}

// the widest layer and the largest weight matrix of a net: the sizes of its CFM_OP_MLP_TRAIN workspace
static void mlp_widest(const int* dims, int n_layers, int* maxw, size_t* maxp) {
    *maxw = 0; *maxp = 0;
    for (int l = 0; l <= n_layers; ++l) *maxw = dims[l] > *maxw ? dims[l] : *maxw;
    for (int l = 0; l < n_layers; ++l) { const size_t p = (size_t)dims[l] * dims[l + 1]; *maxp = p > *maxp ? p : *maxp; }
}

// a CFM_OP_MLP_TRAIN workspace (cfm_mlp_train_ws_bytes_internal), carved: two [B, maxw] gradient buffers, the pool of
// split-K partials, the loss partials at its end
struct TrainWs { float* gbuf[2]; float* pool; size_t pool_floats; float* lpart; };
static TrainWs carve_train_ws(void* ws, int B, int maxw, size_t maxp) {
    TrainWs w;
    w.gbuf[0] = (float*)ws; w.gbuf[1] = w.gbuf[0] + (size_t)B * maxw;
    w.pool = w.gbuf[1] + (size_t)B * maxw;
    w.pool_floats = (size_t)MLP_MAX_SPLITS * (maxp + maxw) * 4;
    w.lpart = w.pool + w.pool_floats;
    return w;
}

// mlp.hip
int cfm_gemm_pick_tile(long M, long N, long splits);
int cfm_mlp_launch_layer(const MlpNetLayer* net, int nets, int lda, int ldw, const float* t, int t_per_row, int tcol, int B,
                         int K, int N, bool act, float inv_n, hipStream_t s, int* n_partials);

// one product of each net of a launch: per-net operands (the sizes, pitches and tvec are shared)
struct GemmOps { const float* A; const float* Bm; float* C; const float* H; float* colsum; float* tsum; };

static GemmArgs gemm_args(const GemmOps& o, int lda, int ldb, int ldc, size_t split_stride, int M, int N, int Kc, int k_chunk,
                          int tiles_n, const float* tvec) {
    GemmArgs G;
    G.A = o.A; G.lda = lda; G.Bm = o.Bm; G.ldb = ldb; G.C = o.C; G.ldc = ldc; G.split_stride = split_stride; G.H = o.H;
    G.M = M; G.N = N; G.Kc = Kc; G.k_chunk = k_chunk; G.tiles_n = tiles_n; G.colsum = o.colsum; G.tvec = tvec; G.tsum = o.tsum;
    return G;
}

// nets == 1: gemm_f32_mfma; nets == 2: gemm_f32_mfma_two on twice the grid (MAXNETS == 1: a product no two-net caller has,
// for which no two-net kernel is built)
template <bool AK, bool BK_, int EPI, int MAXNETS, bool VA, bool VB>
static void launch_gemm_t(int tile, const GemmOps* op, int nets, int lda, int ldb, int ldc, size_t split_stride, int M, int N,
                          int Kc, int k_chunk, int S, hipStream_t s, const float* tvec) {
    const int bm = tile == 0 ? 128 : 64;
    const int tm = (M + bm - 1) / bm, tn = (N + bm - 1) / bm;
    GemmArgs2 T;
    for (int q = 0; q < nets; ++q) T.net[q] = gemm_args(op[q], lda, ldb, ldc, split_stride, M, N, Kc, k_chunk, tn, tvec);
    const dim3 grid(nets * tm * tn, S);
    if (MAXNETS == 1 || nets == 1) {
        if (tile == 0) hipLaunchKernelGGL((gemm_f32_mfma<128, 128, 16, AK, BK_, EPI, VA, VB>), grid, dim3(256), 0, s, T.net[0]);
        else hipLaunchKernelGGL((gemm_f32_mfma<64, 64, 32, AK, BK_, EPI, VA, VB>), grid, dim3(256), 0, s, T.net[0]);
    } else if constexpr (MAXNETS == 2) {
        if (tile == 0) hipLaunchKernelGGL((gemm_f32_mfma_two<128, 128, 16, AK, BK_, EPI, VA, VB>), grid, dim3(256), 0, s, T, (unsigned)(tm * tn));
        else hipLaunchKernelGGL((gemm_f32_mfma_two<64, 64, 32, AK, BK_, EPI, VA, VB>), grid, dim3(256), 0, s, T, (unsigned)(tm * tn));
    }
}

static bool gemm_vec_ok(const float* p, int ld, int extent) { return (ld % 4 == 0) && ((uintptr_t)p & 15) == 0 && (extent % 4 == 0); }

// One product of one net or of two nets of equal sizes: tile and split from the sizes, 16-byte loads per net from its own
// operands.  Two nets whose choices are equal share one launch; unequal ones (an operand of one net off the 16-byte grid)
// take this launcher once each, as one net.
template <bool AK, bool BK_, int EPI, int MAXNETS = 2>
static int launch_gemm(const GemmOps* op, int nets, int lda, int ldb, int ldc, size_t split_stride, int M, int N, int Kc, int S,
                       hipStream_t s, const float* tvec = nullptr) {
    // 16-byte loads per operand: K-contiguous needs Kc % 4 == 0 (k_chunk is a multiple of 32), K-major needs the row
    // extent % 4 == 0; both need the pitch % 4 == 0 and an aligned base
    bool va[2], vb[2];
    for (int q = 0; q < nets; ++q) { va[q] = gemm_vec_ok(op[q].A, lda, AK ? M : Kc); vb[q] = gemm_vec_ok(op[q].Bm, ldb, BK_ ? N : Kc); }
    if (nets == 2 && (va[0] != va[1] || vb[0] != vb[1])) {
        for (int q = 0; q < 2; ++q) {
            const int rc = launch_gemm<AK, BK_, EPI, MAXNETS>(op + q, 1, lda, ldb, ldc, split_stride, M, N, Kc, S, s, tvec);
            if (rc) return rc;
        }
        return 0;
    }
    int k_chunk = (Kc + S - 1) / S;
    k_chunk = (k_chunk + 31) / 32 * 32;
    const int tile = cfm_gemm_pick_tile(M, N, S);
#define CFM_LG(VA_, VB_) launch_gemm_t<AK, BK_, EPI, MAXNETS, VA_, VB_>(tile, op, nets, lda, ldb, ldc, split_stride, M, N, Kc, k_chunk, S, s, tvec)
    if (va[0]) { if (vb[0]) CFM_LG(true, true); else CFM_LG(true, false); }
    else       { if (vb[0]) CFM_LG(false, true); else CFM_LG(false, false); }
#undef CFM_LG
    return cfm_status();
}

// dgrad (dop: dz . W, SELU' of the pre-activations H) and wgrad (wop: dz^T . h, bias column sums riding along) of one
// layer [N, K] in ONE launch, gemm_pair_f32_mfma (one net) or gemm_pair_f32_mfma_two (two nets): when both products run
// on 64 x 64 tiles with 16-byte loads (every hidden layer at C3), in every net.  false: nothing launched, the caller takes
// two launches.
static bool launch_gemm_pair(const GemmOps* dop, const GemmOps* wop, int nets, int B, int K, int N, int S, hipStream_t s) {
    if (cfm_gemm_pick_tile(N, K, S) != 2 || cfm_gemm_pick_tile(B, K, 1) != 2) return false;
    for (int q = 0; q < nets; ++q)
        if (!(gemm_vec_ok(dop[q].A, N, N) && gemm_vec_ok(wop[q].Bm, K, K) && gemm_vec_ok(dop[q].Bm, K, K))) return false;
    int k_chunk_w = (B + S - 1) / S; k_chunk_w = (k_chunk_w + 31) / 32 * 32;
    const int k_chunk_d = (N + 31) / 32 * 32;
    const int tn = (K + 63) / 64, tiles_w = ((N + 63) / 64) * tn, tiles_d = ((B + 63) / 64) * tn;
    GemmArgs2 Ga, Gw;
    for (int q = 0; q < nets; ++q) {
        Ga.net[q] = gemm_args(dop[q], N, K, K, 0, B, K, N, k_chunk_d, tn, nullptr);
        Gw.net[q] = gemm_args(wop[q], N, K, K, (size_t)N * K, N, K, B, k_chunk_w, tn, nullptr);
    }
    const dim3 grid(nets * (tiles_d + tiles_w * S));
    if (nets == 1) hipLaunchKernelGGL(gemm_pair_f32_mfma, grid, dim3(256), 0, s, Ga.net[0], tiles_d, Gw.net[0], tiles_w, S);
    else hipLaunchKernelGGL(gemm_pair_f32_mfma_two, grid, dim3(256), 0, s, Ga, tiles_d, Gw, tiles_w, S);
    return true;
}

// batch splits of a weight gradient dW[N, K]: enough workgroups to fill the chip, at least 64 rows per split
// (round 6, forced split counts at C3: S = 4 / 8 / 16 (this rule) / 32: forward + MSE + backward 444 / 413 / 410 / 477 us —
//  profiles/r6_experiments.txt)
static int wgrad_splits(int N, int K, int B) {
    const long tiles = (long)((N + 127) / 128) * ((K + 127) / 128);
    int S = 1;
    while (S < MLP_MAX_SPLITS && tiles * S < 256 && B / (2 * S) >= 64) S *= 2;
    return S;
}

// What the backward needs of one net.  acts[l] = h_l (l = 0: the network input [B, dims[0]]; l = 1 .. n-1: the saved
// hidden activations), zs[l] = z_l for l = 1 .. n-1 (zs[0] unused); dout [B, dims[n]]; dW[l] ([dims[l+1], dims[l]]) and
// db[l] receive the gradients.  has_loss: `loss` is one more job for the final reduction (the loss partials of a fused step).
struct NetBackward {
    const float* acts[MLP_MAX_LAYERS]; const float* zs[MLP_MAX_LAYERS]; const float* const* W; float* const* dW; float* const* db;
    const float* dout; TrainWs ws; ReduceJob loss; bool has_loss;
};

// Backward through all layers of one net, or of two nets of equal sizes (the flow and the score net of the SF2M step): layer
// by layer the same launches, for two nets each on twice the grid, with tile, split and pairing decided per net.
// Launches: per layer ONE launch for wgrad (bias column sums ride along) + dgrad (round 6; two where the shapes do not allow
// the pair), then ONE reduction of every split-K partial (weights and biases of all layers and nets, and their loss
// partials).  A workspace's pool holds four layers' partials at 32 splits: deeper nets that fill it get one more reduction
// per refill (see the loop).
// tvec != NULL: the network input is [acts[0] (B x dims[0] - 1, pitch dims[0] - 1), tvec (B)] — the time column is
// kept apart (the fused steps never concatenate it); its weight gradient is the weighted column sum.
// nets == 1 only (the SF2M step has neither): dx, if not NULL, receives the input gradient [B, dims[0]]; layer_done, if not
// NULL, asks for the bucketed form (one reduction per layer, see the loop).
// The caller bounds n_layers by what ONE ReduceTable holds: MLP_MAX_LAYERS - 1 for one net, SF2M_MAX_LAYERS for two.
static int mlp_backward_impl(const NetBackward* nb, int nets, const int* dims, int n_layers, int B, hipStream_t s,
                             const float* tvec, float* dx, void* const* layer_done) {
    const size_t pool_floats = nb[0].ws.pool_floats;
    size_t used = 0;
    ReduceTable T; T.count = 0;
    const float* dz[2];
    for (int q = 0; q < nets; ++q) dz[q] = nb[q].dout;
    for (int l = n_layers - 1; l >= 0; --l) {
        const bool split_t = (l == 0 && tvec != nullptr);
        const int Kfull = dims[l], N = dims[l + 1];
        const int K = split_t ? Kfull - 1 : Kfull;            // columns of the GEMM operand
        // wgrad: dW[N,K] = dz^T[N,B] . h[B,K], contraction over the batch, S splits; db partials ride along
        const int S = wgrad_splits(N, K, B);
        const size_t np = (size_t)N * K;
        const size_t need = (size_t)S * (np + (size_t)N * (split_t ? 2 : 1));
        // (cannot happen with a workspace of cfm_mlp_train_ws_bytes_internal: np + 2 N <= maxp + maxw even with the time
        //  column apart and S <= MLP_MAX_SPLITS, a quarter of the pool — kept for a caller that passes other dims there)
        if (need > pool_floats) return CFM_EINVAL;
        if (used + need > pool_floats) {
            // the pool is full (a fifth layer at S = 32): reduce what has been collected and start it again at offset zero.
            // Stream order puts the reduction in front of the next product, so no slot is rewritten before it is read;
            // every job keeps its partials and its split order: bit-equal to an unbounded pool.  (The loss jobs stay in
            // the final launch.)
            if (T.count) { hipLaunchKernelGGL(reduce_splits_multi, dim3(256, T.count), dim3(256), 0, s, T); T.count = 0; }
            used = 0;
        }
        const size_t o_part = used; used += (size_t)S * np;
        const size_t o_bpart = used; used += (size_t)S * N;
        const size_t o_tpart = used; if (split_t) used += (size_t)S * N;
        // dgrad of the same layer: dz_prev[B,K] = (dz[B,N] . W[N,K]) * selu'(z_prev) — reads dz_l like wgrad and nothing of it
        GemmOps wop[2], dop[2];
        for (int q = 0; q < nets; ++q) {
            float* pool = nb[q].ws.pool;
            wop[q] = GemmOps{dz[q], nb[q].acts[l], pool + o_part, nullptr, pool + o_bpart, split_t ? pool + o_tpart : nullptr};
            dop[q] = GemmOps{dz[q], nb[q].W[l], l > 0 ? nb[q].ws.gbuf[l & 1] : nullptr, nb[q].zs[l], nullptr, nullptr};
        }
        const bool paired = l > 0 && launch_gemm_pair(dop, wop, nets, B, K, N, S, s);
        int rc = paired ? cfm_status()
                        : launch_gemm<true, true, EPI_PLAIN>(wop, nets, N, K, K, np, N, K, B, S, s, split_t ? tvec : nullptr);
        if (rc) return rc;
        for (int q = 0; q < nets; ++q) {
            T.job[T.count++] = ReduceJob{wop[q].C, nb[q].dW[l], np, np, S, split_t ? K : 0, Kfull, 0};
            T.job[T.count++] = ReduceJob{wop[q].colsum, nb[q].db[l], (unsigned long long)N, (unsigned long long)N, S, 0, 0, 0};
            if (split_t) T.job[T.count++] = ReduceJob{wop[q].tsum, nb[q].dW[l] + K, (unsigned long long)N, (unsigned long long)N, S, 1, Kfull, 0};
        }
        if (layer_done) {
            // bucketed form (data parallel): this layer's gradients are final as soon as its own reduction has run —
            // the caller's communication stream waits for layer_done[l] and all-reduces them while the remaining
            // layers' products run.  Same jobs, same order of the partial sums: bit-equal to the one-reduction form.
            if (l == 0 && nb[0].has_loss) T.job[T.count++] = nb[0].loss;
            hipLaunchKernelGGL(reduce_splits_multi, dim3(256, T.count), dim3(256), 0, s, T);
            T.count = 0; used = 0;      // (the next layer's partials go where these were: its product runs behind this reduction)
            if (layer_done[l]) { const hipError_t e = hipEventRecord((hipEvent_t)layer_done[l], s); if (e != hipSuccess) return (int)e; }
        }
        if (l > 0) {
            if (!paired) {
                rc = launch_gemm<false, true, EPI_SELU_GRAD>(dop, nets, N, K, K, 0, B, K, N, 1, s);
                if (rc) return rc;
            }
            for (int q = 0; q < nets; ++q) dz[q] = dop[q].C;
        } else if (dx) {
            const GemmOps xop = {dz[0], nb[0].W[0], dx, nullptr, nullptr, nullptr};
            rc = launch_gemm<false, true, EPI_PLAIN, 1>(&xop, 1, N, Kfull, Kfull, 0, B, Kfull, N, 1, s);
            if (rc) return rc;
        }
    }
    if (layer_done) return cfm_status();
    for (int q = 0; q < nets; ++q) if (nb[q].has_loss) T.job[T.count++] = nb[q].loss;
    hipLaunchKernelGGL(reduce_splits_multi, dim3(256, T.count), dim3(256), 0, s, T);
    return cfm_status();
}

extern "C" int cfm_mlp_backward_f32(const float* const* acts, const float* const* preact, const float* const* W,
                                    const int* dims, int n_layers, int B, const float* dout, float* const* dW,
                                    float* const* db, float* dx, void* ws, void* stream) {
    if (!acts || !W || !dims || !dout || !dW || !db || n_layers < 1 || n_layers > MLP_MAX_LAYERS - 1 || B < 0 || !ws) return CFM_EINVAL;
    if (n_layers > 1 && !preact) return CFM_EINVAL;
    if (B == 0) return 0;
    int maxw; size_t maxp;
    mlp_widest(dims, n_layers, &maxw, &maxp);
    NetBackward nb;
    nb.acts[0] = acts[0]; nb.zs[0] = nullptr;
    for (int l = 1; l < n_layers; ++l) { nb.acts[l] = acts[l]; nb.zs[l] = preact[l]; }
    nb.W = W; nb.dW = dW; nb.db = db; nb.dout = dout; nb.ws = carve_train_ws(ws, B, maxw, maxp); nb.has_loss = false;
    return mlp_backward_impl(&nb, 1, dims, n_layers, B, (hipStream_t)stream, nullptr, dx, nullptr);
}

// ------------------------------------------------------- fused regression step ----
// g = (2 / n) (v - u) in place of v, and the partial sums of (v - u)^2 (one per workgroup, summed in block order by
// the backward's final reduction: deterministic)
#define MSE_BLOCKS 256
__global__ __launch_bounds__(256) void mse_grad(float* __restrict__ v, const float* __restrict__ u, size_t n, float scale,
                                                float inv_n, float* __restrict__ partial) {
    __shared__ float sh[4];
    float acc = 0.f;
    const size_t n4 = n / 4;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (size_t)gridDim.x * 256) {
        float4 a = reinterpret_cast<float4*>(v)[e];
        const float4 b = reinterpret_cast<const float4*>(u)[e];
        a.x -= b.x; a.y -= b.y; a.z -= b.z; a.w -= b.w;
        acc = fmaf(a.x, a.x, acc); acc = fmaf(a.y, a.y, acc); acc = fmaf(a.z, a.z, acc); acc = fmaf(a.w, a.w, acc);
        a.x *= scale; a.y *= scale; a.z *= scale; a.w *= scale;
        reinterpret_cast<float4*>(v)[e] = a;
    }
    if (blockIdx.x == 0)
        for (size_t e = n4 * 4 + threadIdx.x; e < n; e += 256) { const float d = v[e] - u[e]; acc = fmaf(d, d, acc); v[e] = d * scale; }
    acc = wave_sum_f(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + (sh[2] + sh[3])) * inv_n;
}

// What the training forward needs of one net: parameters, the buffers that keep h_l and z_l (hidden[l], preact[l]: [B, dims[l + 1]],
// l = 0 .. n - 2), the output g [B, dims[n]], and its loss: target, row weights (or NULL), seed scale, loss partials.
struct NetForward {
    const float* const* W; const float* const* b; float* const* hidden; float* const* preact; float* g;
    const float* target; const float* lam; float scale; float* lpart;
    int lam_mode;      // what the row weights do (cfm_common.h): LAM_RESIDUAL, or LAM_ROW_WEIGHT for the DSBM step
};

// one loss partial per workgroup of the last layer (an upper bound: the 128 x 128 form has fewer)
static bool loss_partials_fit(int B, int N) { return (long)((B + 63) / 64) * ((N + 63) / 64) <= MLP_LOSS_PARTIALS; }

// Training forward of one net or of two nets of equal sizes on the same input [xt, t], keeping h_l and z_l.  fuse_loss: the
// LAST layer's epilogue forms each net's loss gradient seed in place of its output and one loss partial per workgroup,
// *n_lpart of them (round 6: the MSE was a launch of its own and a second pass over v); otherwise g receives the output.
static int mlp_train_forward(const NetForward* nf, int nets, const float* xt, const float* t, const int* dims, int n_layers, int B,
                             float inv_n, bool fuse_loss, hipStream_t s, int* n_lpart) {
    const float* cur[2] = {xt, xt};
    for (int l = 0; l < n_layers; ++l) {
        const bool last = (l == n_layers - 1);
        const bool first_t = (l == 0 && t != nullptr);
        const int K = first_t ? dims[0] - 1 : dims[l];
        MlpNetLayer net[2];
        for (int q = 0; q < nets; ++q) {
            float* dst = last ? nf[q].g : nf[q].hidden[l];
            net[q] = MlpNetLayer{cur[q], nf[q].W[l], nf[q].b[l], dst, last ? nullptr : nf[q].preact[l], nullptr, nullptr, 0.f, nullptr};
            if (last && fuse_loss) { net[q].target = nf[q].target; net[q].lam = nf[q].lam; net[q].scale = nf[q].scale; net[q].partial = nf[q].lpart; net[q].lam_mode = nf[q].lam_mode; }
            cur[q] = dst;
        }
        const int rc = cfm_mlp_launch_layer(net, nets, K, dims[l], first_t ? t : nullptr, first_t ? 1 : 0, first_t ? K : -1, B, K,
                                            dims[l + 1], !last, inv_n, s, (last && fuse_loss) ? n_lpart : nullptr);
        if (rc) return rc;
    }
    return 0;
}

// the backward's view of a net the training forward has run: input, saved activations, seed, and its loss job
static void net_backward_of(NetBackward* nb, const NetForward& nf, const float* xt, int n_layers, float* const* dW, float* const* db,
                            const TrainWs& ws, float* loss, int n_lpart) {
    nb->acts[0] = xt; nb->zs[0] = nullptr;
    for (int l = 1; l < n_layers; ++l) { nb->acts[l] = nf.hidden[l - 1]; nb->zs[l] = nf.preact[l - 1]; }
    nb->W = nf.W; nb->dW = dW; nb->db = db; nb->dout = nf.g; nb->ws = ws;
    nb->loss = ReduceJob{nf.lpart, loss, 1ull, 1ull, n_lpart, 0, 0, 1};      // (pad = 1: one number out of n_lpart partials)
    nb->has_loss = true;
}

// One regression step of the vector field on a coupled batch, everything but the optimizer update:
//     v = net([xt, t]);  loss = mean((v - ut)^2);  dW, db = d loss / d parameters
// — what `vt = model(torch.cat([xt, t[:, None]], -1)); loss = torch.mean((vt - ut) ** 2); loss.backward()` does in the
// reference's loops (examples/images/cifar10/train_cifar10.py:147-149, every 2D tutorial).  t == NULL: the net is
// not time varying (dims[0] = columns of xt); otherwise dims[0] = columns of xt + 1 and the time column is never
// materialised: forward adds its rank-1 term in the first layer's epilogue, backward takes its weight gradient
// as a weighted column sum.  g [B, dims[n]] receives d loss / d v (the caller may ignore it); *loss a device float.
// 10 launches for the 4-layer field (round 6: dgrad + wgrad of a layer share one, the MSE rides in the last layer's
// epilogue), all kernels of this library (no eager elementwise ops in between).
extern "C" int cfm_mlp_regression_step_f32(const float* xt, const float* t, const float* ut,
                                           const float* const* W, const float* const* b, const int* dims, int n_layers,
                                           int B, float* const* hidden, float* const* preact, float* g,
                                           float* const* dW, float* const* db, float* loss, void* const* layer_done,
                                           void* ws, void* stream) {
    if (!xt || !ut || !W || !b || !dims || !g || !dW || !db || !loss || !ws || n_layers < 1 || n_layers > MLP_MAX_LAYERS - 1 || B < 1)
        return CFM_EINVAL;
    if (n_layers > 1 && (!hidden || !preact)) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (t && dims[0] < 2) return CFM_EINVAL;
    int maxw; size_t maxp;
    mlp_widest(dims, n_layers, &maxw, &maxp);
    const TrainWs tw = carve_train_ws(ws, B, maxw, maxp);
    const size_t nel = (size_t)B * dims[n_layers];
    const float inv_n = 1.0f / (float)nel;
    const NetForward nf = {W, b, hidden, preact, g, ut, nullptr, 2.0f * inv_n, tw.lpart};
    // a last layer of more workgroups than loss partials: the loss is a launch of its own behind the forward
    const bool fused = loss_partials_fit(B, dims[n_layers]);
    int n_lpart = MSE_BLOCKS;
    int rc = mlp_train_forward(&nf, 1, xt, t, dims, n_layers, B, inv_n, fused, s, &n_lpart);
    if (rc) return rc;
    if (!fused) {
        hipLaunchKernelGGL(mse_grad, dim3(MSE_BLOCKS), dim3(256), 0, s, g, ut, nel, 2.0f * inv_n, inv_n, tw.lpart);
        rc = cfm_status();
        if (rc) return rc;
    }
    // backward (+ the loss partials in its final reduction)
    NetBackward nb;
    net_backward_of(&nb, nf, xt, n_layers, dW, db, tw, loss, n_lpart);
    return mlp_backward_impl(&nb, 1, dims, n_layers, B, s, t, nullptr, layer_done);
}

// ------------------------------------------------------------ the SF2M step: two nets ----
// the deepest pair of nets whose reduction jobs fit ONE ReduceTable: 2 nets x (2 per layer + the time column + the loss)
#define SF2M_MAX_LAYERS ((2 * MLP_MAX_LAYERS + 2 - 4) / 4)

// One [SF]2M training step for a flow net and a score net of equal layer sizes, everything but the optimizer update:
//     v = flow([xt, t]);  s = score([xt, t]);  losses = {mean((v - ut)^2), mean((lam[:, None] * s + eps)^2)}
//     dW, db of both nets = d (losses[0] + score_weight * losses[1]) / d parameters
// — examples/2D_tutorials/SF2M_tutorial.ipynb cell 3, runner/src/models/cfm_module.py:896-909.  Every launch of
// cfm_mlp_regression_step_f32 serves both nets (see gemm_f32_mfma_two), so the step has the launch count of ONE
// regression step; the kernel choices are made per net, so each net's gradients are the bits that step gives it alone
// (the flow net on ut; the score net, with lam = 1, on -eps).
extern "C" int cfm_mlp_sf2m_step_f32(const float* xt, const float* t, const float* ut, const float* eps, const float* lam,
                                     const float* const* W, const float* const* b, float* const* hidden,
                                     float* const* preact, float* const* dW, float* const* db, const int* dims,
                                     int n_layers, int B, float* g_flow, float* g_score, float* losses,
                                     float score_weight, void* ws, void* stream) {
    if (!xt || !ut || !eps || !lam || !W || !b || !dims || !g_flow || !g_score || !dW || !db || !losses || !ws || n_layers < 1 || B < 1)
        return CFM_EINVAL;
    if (n_layers > SF2M_MAX_LAYERS) return CFM_EINVAL;      // the one reduction's table is full at two nets of 7 layers
    if (n_layers > 1 && (!hidden || !preact)) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (t && dims[0] < 2) return CFM_EINVAL;
    // one loss partial per workgroup of the last layer (this step has no separate loss launch to fall back on)
    if (!loss_partials_fit(B, dims[n_layers])) return CFM_EINVAL;
    int maxw; size_t maxp;
    mlp_widest(dims, n_layers, &maxw, &maxp);
    // two CFM_OP_MLP_TRAIN workspaces back to back: the flow net's, then the score net's
    const size_t ws_pitch = cfm_align_up(cfm_mlp_train_ws_bytes_internal(B, maxw, (int)maxp), 256);
    const size_t nel = (size_t)B * dims[n_layers];
    const float inv_n = 1.0f / (float)nel;
    TrainWs tw[2]; NetForward nf[2];
    for (int q = 0; q < 2; ++q) {
        tw[q] = carve_train_ws((char*)ws + q * ws_pitch, B, maxw, maxp);
        nf[q] = NetForward{W + q * n_layers, b + q * n_layers, hidden + q * (n_layers - 1), preact + q * (n_layers - 1), q ? g_score : g_flow,
                           q ? eps : ut, q ? lam : nullptr, q ? (2.0f * inv_n) * score_weight : 2.0f * inv_n, tw[q].lpart};
    }
    int n_lpart = 0;
    const int rc = mlp_train_forward(nf, 2, xt, t, dims, n_layers, B, inv_n, true, s, &n_lpart);
    if (rc) return rc;
    NetBackward nb[2];
    for (int q = 0; q < 2; ++q) net_backward_of(&nb[q], nf[q], xt, n_layers, dW + q * n_layers, db + q * n_layers, tw[q], losses + q, n_lpart);
    return mlp_backward_impl(nb, 2, dims, n_layers, B, s, t, nullptr, nullptr);
}

// ------------------------------------------------------------ the DSBM step: two nets ----
// One DSBM (diffusion Schrodinger bridge matching) training step for a forward and a backward drift net of equal layer sizes,
// everything but the optimizer update:
//     f = fwd([xt, t]);  b = bwd([xt, t])
//     losses = {mean(wf[:, None] * (f - ft)^2), mean(wb[:, None] * (b - bt)^2)};  dW, db of both nets = d (losses[0] + losses[1]) / d parameters
// — runner/src/models/cfm_module.py:1203-1227 (DSBMLitModule.step: the two row-scaled MSEs and their sum).  The two-net driver
// of cfm_mlp_sf2m_step_f32 with the row-weighted loss epilogue (LAM_ROW_WEIGHT) on both nets: the launch count of ONE
// regression step, and with wf = wb = 1 each net's loss and gradients are the bits cfm_mlp_regression_step_f32 gives it alone.
extern "C" int cfm_mlp_dsbm_step_f32(const float* xt, const float* t, const float* ft, const float* bt, const float* wf,
                                     const float* wb, const float* const* W, const float* const* b, float* const* hidden,
                                     float* const* preact, float* const* dW, float* const* db, const int* dims,
                                     int n_layers, int B, float* g_fwd, float* g_bwd, float* losses, void* ws, void* stream) {
    if (!xt || !ft || !bt || !wf || !wb || !W || !b || !dims || !g_fwd || !g_bwd || !dW || !db || !losses || !ws || n_layers < 1 || B < 1)
        return CFM_EINVAL;
    if (n_layers > SF2M_MAX_LAYERS) return CFM_EINVAL;      // the one reduction's table is full at two nets of 7 layers
    if (n_layers > 1 && (!hidden || !preact)) return CFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (t && dims[0] < 2) return CFM_EINVAL;
    if (!loss_partials_fit(B, dims[n_layers])) return CFM_EINVAL;
    int maxw; size_t maxp;
    mlp_widest(dims, n_layers, &maxw, &maxp);
    // two CFM_OP_MLP_TRAIN workspaces back to back: the forward net's, then the backward net's
    const size_t ws_pitch = cfm_align_up(cfm_mlp_train_ws_bytes_internal(B, maxw, (int)maxp), 256);
    const size_t nel = (size_t)B * dims[n_layers];
    const float inv_n = 1.0f / (float)nel;
    TrainWs tw[2]; NetForward nf[2];
    for (int q = 0; q < 2; ++q) {
        tw[q] = carve_train_ws((char*)ws + q * ws_pitch, B, maxw, maxp);
        nf[q] = NetForward{W + q * n_layers, b + q * n_layers, hidden + q * (n_layers - 1), preact + q * (n_layers - 1), q ? g_bwd : g_fwd,
                           q ? bt : ft, q ? wb : wf, 2.0f * inv_n, tw[q].lpart, LAM_ROW_WEIGHT};
    }
    int n_lpart = 0;
    const int rc = mlp_train_forward(nf, 2, xt, t, dims, n_layers, B, inv_n, true, s, &n_lpart);
    if (rc) return rc;
    NetBackward nb[2];
    for (int q = 0; q < 2; ++q) net_backward_of(&nb[q], nf[q], xt, n_layers, dW + q * n_layers, db + q * n_layers, tw[q], losses + q, n_lpart);
    return mlp_backward_impl(nb, 2, dims, n_layers, B, s, t, nullptr, nullptr);
}

// ------------------------------------------------------------------- Adam ----
// torch.optim.Adam (amsgrad = False, maximize = False), single step on every tensor of the table:
//   g      = grad (+ weight_decay * p)
//   m      = lerp(m, g, w = 1 - beta1)        = m + w * (g - m)          for |w| <  0.5
//                                             = g - (g - m) * (1 - w)    for |w| >= 0.5   (ATen/native/Lerp.h)
//   v      = v * beta2 + (1 - beta2) * g * g
//   denom  = sqrt(v) / sqrt(bias_correction2) + eps
//   p      = p - (lr / bias_correction1) * m / denom
// The scalar factors arrive as the fp32 roundings of the Python doubles torch computes them with.
struct AdamTable { float* p; const float* g; float* m; float* v; unsigned long long n; };

// (the contraction pattern below is the one that is bit-equal to torch's foreach kernels on ROCm 7 /
//  torch 2.10, found by probing the alternatives: tools/probe/adam_probe.py)
__global__ __launch_bounds__(256) void adam_multi(const AdamTable* __restrict__ tab, int n_tensors,
                                                  float w1, float omw1, int w1_small, float beta2, float w2,
                                                  float bc2_sqrt, float eps, float step_size, float weight_decay,
                                                  float grad_scale) {
    for (int q = blockIdx.y; q < n_tensors; q += gridDim.y) {
        const AdamTable T = tab[q];
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < T.n; e += (size_t)gridDim.x * 256) {
            float g = T.g[e];
            if (grad_scale != 1.f) {              // data parallel: the all-reduced SUM -> the mean (`grad.mul_(1 / world)`),
                g = __fmul_rn(g, grad_scale);     // folded into this launch; .grad is left holding the mean, as DDP leaves it
                const_cast<float*>(T.g)[e] = g;
            }
            const float p = T.p[e];
            if (weight_decay != 0.f) g = fmaf(weight_decay, p, g);
            float m = T.m[e], v = T.v[e];
            const float gm = g - m;                                   // lerp: the form is uniform over the launch
            m = w1_small ? fmaf(w1, gm, m) : fmaf(-gm, omw1, g);
            v = fmaf(w2, __fmul_rn(g, g), __fmul_rn(v, beta2));       // mul_, then addcmul_
            const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), eps);
            T.m[e] = m; T.v[e] = v;
            T.p[e] = fmaf(-step_size, __fdiv_rn(m, denom), p);        // addcdiv_
        }
    }
}

// table: device array of n_tensors AdamTable records {param, grad, exp_avg, exp_avg_sq, numel}
extern "C" int cfm_adam_step_f32(const void* table, int n_tensors, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, int step, double grad_scale, void* stream) {
    if (!table || n_tensors < 0 || step < 1 || !(grad_scale > 0.0)) return CFM_EINVAL;
    if (n_tensors == 0) return 0;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const double step_size = lr / bc1, bc2_sqrt = sqrt(bc2);
    const float w1 = (float)(1.0 - beta1);       // ATen switches forms on the fp32 weight and takes 1 - w in fp32
    hipLaunchKernelGGL(adam_multi, dim3(256, n_tensors < 16 ? n_tensors : 16), dim3(256), 0, (hipStream_t)stream,
                       (const AdamTable*)table, n_tensors, w1, 1.0f - w1, fabsf(w1) < 0.5f ? 1 : 0, (float)beta2,
                       (float)(1.0 - beta2),
                       (float)bc2_sqrt, (float)eps, (float)step_size, (float)weight_decay, (float)grad_scale);
    return cfm_status();
}
