// ode_reverse.h — what ode_small_fixed_grad (ode_grad.h) and ode_small_adaptive_grad (ode_adaptive_grad.h) share: the
// kernel prologue and one reverse step of an explicit Runge-Kutta step on a 16-row tile (ode_grad.h's header says what it
// computes and how its LDS buffers alternate).  The scheme enters as a compile-time coefficient source T only:
//   T::NS        the stage count
//   T::a(s, q)   stage s + 2 is Y = fmaf(h, sum_{q <= s} a(s, q) k_{q+1}, y_n)     (fp64; every use casts to float)
//   T::b(s)      y_{n+1} = fmaf(h, sum_s b(s) k_{s+1}, y_n)
// The caller supplies y_n, lam_{n+1}, the signed step h, the stage times tsg (the field's arguments) and the accumulators.
// Runs on cg_stage_transposed of cnf_grad.h and on the tile engine of small_field.h (cg_put, cg_outer, cg_sum4 among it).
#pragma once

// one staged net, the transposed copies of its two 64 x 64 layers, four tile buffers
constexpr size_t og_lds_bytes = small_lds_bytes(1, 4, false) + sizeof(float) * 2 * SM_W * SM_LD;
static_assert(og_lds_bytes == 123136 && og_lds_bytes <= cg_lds_bytes, "the ODE gradient kernels");

template <int SCHEME>
struct FxCoef {                               // euler, midpoint, rk4 (ode_tableau.h)
    static constexpr int NS = fx_stages<SCHEME>();
    static __device__ __forceinline__ double a(int s, int q) { return fx_a<SCHEME>(s, q); }
    static __device__ __forceinline__ double b(int s) { return fx_b<SCHEME>(s); }
};
template <int TAB>
struct RkCoef {                               // dopri5, tsit5: the six stages of an accepted step, b = row 5 of a
    static constexpr int NS = 6;
    static __device__ __forceinline__ double a(int s, int q) { return rk_a<TAB>(s, q); }
    static __device__ __forceinline__ double b(int s) { return rk_a<TAB>(NS - 1, s); }
};

struct OgLds { float *Wl, *WT, *bl, *wt, *P0, *P1, *Q0, *Q1; };

// the carve of og_lds_bytes, the net and the transposed copies staged.  (The zeroing of the accumulators stays in the two
// kernels: behind this helper the compiler keeps dWa in arch VGPRs and ode_small_fixed_grad<rk4> needs all 512 registers,
// profiles/grad_unit_split.txt.)
__device__ __forceinline__ OgLds og_prologue(const SmArgs& A, int d, float* lds, int tid) {
    constexpr int TS = SM_ROWS * SM_LD, WS = SM_W * SM_LD;
    OgLds L;
    L.Wl = lds;
    L.WT = L.Wl + 4 * WS;                     // W1^T, W2^T
    L.bl = L.WT + 2 * WS;
    L.wt = L.bl + 4 * SM_W;
    L.P0 = L.wt + SM_W;
    L.P1 = L.P0 + TS;
    L.Q0 = L.P1 + TS;
    L.Q1 = L.Q0 + TS;
    sm_stage_weights(A, d, L.Wl, L.bl, L.wt, tid);
    cg_stage_transposed(A, L.WT, tid);
    return L;
}

// lam_{n+1} -> lam_{n+1} + sum_s Yb_s, and the step's share of the parameter gradient into dWa, dba, dwt
template <class T>
__device__ __forceinline__ void og_reverse_step(const SmArgs& A, const OgLds& L, int nrows, int wv, int lane, int col,
                                                const SmTile& y, SmTile& lam, float h, const float (&tsg)[T::NS],
                                                f32x4 (&dWa)[4][4], float (&dba)[4], float& dwt) {
    constexpr int NS = T::NS, WS = SM_W * SM_LD;
    float* const Wl = L.Wl; float* const bl = L.bl; float* const wt = L.wt;
    float* const P0 = L.P0; float* const P1 = L.P1; float* const Q0 = L.Q0; float* const Q1 = L.Q1;
    const float* W1T = L.WT;
    const float* W2T = L.WT + WS;
    const float* W3 = Wl + 3 * WS;

    // ---- the stages forward: s_l, h_l, Y_s (the arithmetic of sm_field and of the forward's stage combination) ----
    SmTile s[NS][3], hh[NS][3], Y[NS], f[NS];
    f32x4 c[SM_MB];
#pragma unroll
    for (int sg = 0; sg < NS; ++sg) {
        Y[sg] = y;
        if (sg > 0) {
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                float acc = (float)T::a(sg - 1, 0) * f[0].v[i];
#pragma unroll
                for (int q = 1; q < NS - 1; ++q)
                    if (q < sg) acc = fmaf((float)T::a(sg - 1, q), f[q].v[i], acc);
                Y[sg].v[i] = fmaf(h, acc, y.v[i]);
            }
        }
        cg_put(P0, Y[sg], lane, col);
        sm_lds_barrier();
        float* src = P0; float* dst = P1;
#pragma unroll
        for (int l = 0; l < (sg < NS - 1 ? 4 : 3); ++l) {          // no Y depends on the last stage's slope
            const int N = A.dims[l + 1];
            sm_gemm(src, Wl + l * WS, wv, lane, c);
            const float bv = (col < N) ? bl[l * SM_W + col] : 0.f;
            const float wtc = (l == 0 && col < N) ? wt[col] : 0.f;
#pragma unroll
            for (int i = 0; i < SM_V; ++i) {
                float z = c[0][i] + bv;
                if (l == 0) z = fmaf(tsg[sg], wtc, z);
                if (l < 3) {
                    s[sg][l].v[i] = (col < N && sm_row(i, lane) < nrows) ? selu_slope(z) : 0.f;
                    hh[sg][l].v[i] = (col < N) ? selu_f(z) : 0.f;
                } else {
                    f[sg].v[i] = (col < N) ? z : 0.f;
                }
            }
            if (l < 2 || (l == 2 && sg < NS - 1)) {
                cg_put(dst, hh[sg][l], lane, col);
                sm_lds_barrier();
                float* tmp = src; src = dst; dst = tmp;
            }
        }
    }

    // ---- the stages backward: one vector-Jacobian product each ----
    SmTile Yb[NS], lamn = lam;
#pragma unroll
    for (int sg = NS - 1; sg >= 0; --sg) {
        SmTile kb, zb;
#pragma unroll
        for (int i = 0; i < SM_V; ++i) {
            float acc = (float)T::b(sg) * lam.v[i];
#pragma unroll
            for (int r = sg + 1; r < NS; ++r) acc = fmaf((float)T::a(r - 1, sg), Yb[r].v[i], acc);
            kb.v[i] = h * acc;
        }
        cg_put(Q0, kb, lane, col);
        cg_put(Q1, hh[sg][2], lane, col);
        sm_lds_barrier();
        dba[3] += cg_sum4(kb);
        cg_outer(Q0, Q1, wv, lane, dWa[3]);
        cg_gemm_t(Q0, W3, wv, lane, c[0]);
#pragma unroll
        for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[sg][2].v[i];
        dba[2] += cg_sum4(zb);
        cg_put(P0, zb, lane, col);
        cg_put(P1, hh[sg][1], lane, col);
        sm_lds_barrier();
        cg_outer(P0, P1, wv, lane, dWa[2]);
        sm_gemm(P0, W2T, wv, lane, c);
#pragma unroll
        for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[sg][1].v[i];
        dba[1] += cg_sum4(zb);
        cg_put(Q0, zb, lane, col);
        cg_put(Q1, hh[sg][0], lane, col);
        sm_lds_barrier();
        cg_outer(Q0, Q1, wv, lane, dWa[1]);
        sm_gemm(Q0, W1T, wv, lane, c);
#pragma unroll
        for (int i = 0; i < SM_V; ++i) zb.v[i] = c[0][i] * s[sg][0].v[i];
        {
            const float zs = cg_sum4(zb);
            dba[0] += zs;
            dwt = fmaf(tsg[sg], zs, dwt);
        }
        cg_put(P0, zb, lane, col);
        cg_put(P1, Y[sg], lane, col);
        sm_lds_barrier();
        cg_outer(P0, P1, wv, lane, dWa[0]);
        cg_gemm_t(P0, Wl, wv, lane, c[0]);                                          // zb1 W0[:, :d]
#pragma unroll
        for (int i = 0; i < SM_V; ++i) { Yb[sg].v[i] = c[0][i]; lamn.v[i] += c[0][i]; }
    }
    lam = lamn;
    sm_lds_barrier();       // the last product read (P0, P1): the next step writes y_n there first
}
