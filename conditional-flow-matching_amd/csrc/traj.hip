// traj.hip — multi-marginal flow matching: interval select + gather + interpolant + noise + leave-out rule, one launch.
//
// Replaces, for a batch of trajectories X [B,T,d], the per-row Python loops of runner/src/models/cfm_module.py:
//   linear : preprocess_batch :173-193 (x0.append(tmp_ot_list[ti][0][i]) ...), calc_loc_and_target :225-242
//            (mu_t, x, ut, the `ut /= 2`, `t *= 2` rule and t + t_select)
//   spline : SplineCFMLitModule :1372-1377 and the per-row torchcubicspline evaluate / derivative of :1396-1397, :1406
// Every row reads its interval from t_select and gathers its operands from X where they lie, through the index pairs
// of the interval's coupling (linear) or the chain of draws (spline); nothing is materialised in between.
//
// Linear mode restates the ICFM, SB and scheduled-bridge closed forms of elem.hip's xt_ut_kernel operation by operation
// (separately rounded IEEE ops in the reference's order, contraction off), so it is bit-equal to that kernel on the
// gathered pair.
// Spline mode: all rows share the knots, so the map S from knot values to the natural spline's second derivatives is
// ONE Tp x Tp matrix (host, float64, passed as fp32, staged in LDS); a row needs M_i and M_{i+1} only — two length-Tp
// dot products per element — and then the standard piecewise cubic and its derivative.  Rows of S sum to zero (a
// constant has no curvature), so the products run on y_k - y_i: an offset of the data costs no digits.
// HBM-bound; 16-byte accesses when d % 4 == 0; no atomics, no dependency between workgroups.
#include "cfm_common.h"
#pragma clang fp contract(off)

#define TRAJ_MAX_KNOTS 32

__device__ __forceinline__ float t_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float t_add(float a, float b) { return a + b; }
__device__ __forceinline__ float t_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float t_div(float a, float b) { return a / b; }

template <int W>
struct Vec { float v[W]; };

template <int W>
__device__ __forceinline__ Vec<W> ld(const float* p) {
    Vec<W> r;
    if (W == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r.v[0] = q.x; r.v[1 % W] = q.y; r.v[2 % W] = q.z; r.v[3 % W] = q.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int W>
__device__ __forceinline__ void st(float* p, const Vec<W>& r) {
    if (W == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1 % W], r.v[2 % W], r.v[3 % W]);
    else *p = r.v[0];
}

// slice of X behind interval k's start slice: k + 1, or k + 2 across the left-out slice
__device__ __forceinline__ int next_slice(int k, int leaveout) { return k + 1 + ((leaveout > 0 && k + 1 == leaveout) ? 1 : 0); }

// ------------------------------------------------------------------------------------------------ linear
// idx [T-1][2][B]: (i, j) of interval k at idx + (2 k) B and idx + (2 k + 1) B; NULL = identity.
template <int VARIANT, int W>
__global__ __launch_bounds__(256) void traj_linear_kernel(const float* __restrict__ X, int B, int T, int d,
                                                          const int64_t* __restrict__ idx,
                                                          const int64_t* __restrict__ t_select,
                                                          const float* __restrict__ t, const float* __restrict__ eps,
                                                          float sigma_f, const float* __restrict__ sigma_t, int leaveout,
                                                          float* __restrict__ xt, float* __restrict__ ut,
                                                          float* __restrict__ t_net) {
    const size_t per_row = (size_t)d / W;
    const size_t total = (size_t)B * per_row;
    const size_t row_stride = (size_t)T * d;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
        const int b = (int)(g / per_row);
        const size_t c = (g - (size_t)b * per_row) * W;
        int k = (int)t_select[b];
        k = k < 0 ? 0 : (k > T - 2 ? T - 2 : k);             // (the binding checks the range; never index outside X)
        int k1 = next_slice(k, leaveout);
        const bool halved = k1 != k + 1;
        k1 = k1 > T - 1 ? T - 1 : k1;
        const size_t r0 = idx ? (size_t)idx[((size_t)2 * k) * B + b] : (size_t)b;
        const size_t r1 = idx ? (size_t)idx[((size_t)2 * k + 1) * B + b] : (size_t)b;
        const float tb = t[b];
        const float omt = t_sub(1.0f, tb);
        float sig = sigma_f, ratio = 0.f, rr = 0.f, cc = 0.f;
        if (VARIANT == CFM_VARIANT_SB) {
            sig = sigma_t[b];                                 // the caller's own sigma * sqrt(t (1 - t)) (elem.hip)
            const float two_t = t_mul(2.0f, tb);
            ratio = t_div(t_sub(1.0f, two_t), t_add(t_mul(two_t, omt), 1e-8f));
        } else if (VARIANT == CFM_VARIANT_SCHED) {
            // the caller's [B, 4] table at the row's local time: r, sigma_t, a, g^2 / F(1) (elem.hip)
            const float4 q = reinterpret_cast<const float4*>(sigma_t)[b];
            rr = q.x; sig = q.y; ratio = q.z; cc = q.w;
        }
        const Vec<W> a0 = ld<W>(X + r0 * row_stride + (size_t)k * d + c);
        const Vec<W> a1 = ld<W>(X + r1 * row_stride + (size_t)k1 * d + c);
        const size_t o = (size_t)b * d + c;
        const Vec<W> e = ld<W>(eps + o);
        Vec<W> vx, vu;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const float dx = t_sub(a1.v[q], a0.v[q]);
            const float mu = VARIANT == CFM_VARIANT_SCHED ? t_add(a0.v[q], t_mul(dx, rr))
                                                          : t_add(t_mul(tb, a1.v[q]), t_mul(omt, a0.v[q]));
            vx.v[q] = t_add(mu, t_mul(sig, e.v[q]));
            float u = VARIANT == CFM_VARIANT_SB ? t_sub(t_add(t_mul(ratio, t_sub(vx.v[q], mu)), a1.v[q]), a0.v[q])
                    : VARIANT == CFM_VARIANT_SCHED ? t_add(t_mul(ratio, t_sub(vx.v[q], mu)), t_mul(dx, cc))
                                                   : dx;
            if (halved) u = t_div(u, 2.0f);
            vu.v[q] = u;
        }
        st<W>(xt + o, vx);
        st<W>(ut + o, vu);
        if (c == 0) t_net[b] = t_add(halved ? t_mul(tb, 2.0f) : tb, (float)k);
    }
}

// ------------------------------------------------------------------------------------------------ spline
// Knot q of the Tp = T - (leaveout > 0) knots is slice q + (leaveout > 0 && q >= leaveout) of X, at time tau = that slice
// number.  chain [Tp][B]: the row of X that trajectory b visits at knot q; NULL = identity.  S [Tp][Tp].
__device__ __forceinline__ int knot_slice(int q, int leaveout) { return q + ((leaveout > 0 && q >= leaveout) ? 1 : 0); }

template <int W>
__global__ __launch_bounds__(256) void traj_spline_kernel(const float* __restrict__ X, int B, int T, int d,
                                                          const int64_t* __restrict__ chain,
                                                          const int64_t* __restrict__ t_select,
                                                          const float* __restrict__ u01, const float* __restrict__ eps,
                                                          float sigma_f, int leaveout, const float* __restrict__ S,
                                                          float* __restrict__ xt, float* __restrict__ ut,
                                                          float* __restrict__ t_net) {
    __shared__ float Ssh[TRAJ_MAX_KNOTS * TRAJ_MAX_KNOTS];
    const int Tp = T - (leaveout > 0 ? 1 : 0);
    for (int e = threadIdx.x; e < Tp * Tp; e += 256) Ssh[e] = S[e];
    __syncthreads();
    const size_t per_row = (size_t)d / W;
    const size_t total = (size_t)B * per_row;
    const size_t row_stride = (size_t)T * d;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
        const int b = (int)(g / per_row);
        const size_t c = (g - (size_t)b * per_row) * W;
        int i = (int)t_select[b];
        i = i < 0 ? 0 : (i > Tp - 2 ? Tp - 2 : i);
        const int s0 = knot_slice(i, leaveout), s1 = knot_slice(i + 1, leaveout);
        const float h = (float)(s1 - s0);
        const float u = u01[b], a = 1.0f - u;
        const size_t r0 = chain ? (size_t)chain[(size_t)i * B + b] : (size_t)b;
        const size_t r1 = chain ? (size_t)chain[(size_t)(i + 1) * B + b] : (size_t)b;
        const Vec<W> y0 = ld<W>(X + r0 * row_stride + (size_t)s0 * d + c);
        const Vec<W> y1 = ld<W>(X + r1 * row_stride + (size_t)s1 * d + c);
        Vec<W> m0, m1;
#pragma unroll
        for (int q = 0; q < W; ++q) m0.v[q] = m1.v[q] = 0.f;
        const float* Si = Ssh + i * Tp;
        for (int k = 0; k < Tp; ++k) {
            const size_t rk = chain ? (size_t)chain[(size_t)k * B + b] : (size_t)b;
            const Vec<W> yk = ld<W>(X + rk * row_stride + (size_t)knot_slice(k, leaveout) * d + c);
            const float w0 = Si[k], w1 = Si[Tp + k];
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const float dy = yk.v[q] - y0.v[q];
                m0.v[q] = fmaf(w0, dy, m0.v[q]);
                m1.v[q] = fmaf(w1, dy, m1.v[q]);
            }
        }
        // s(tau_i + u h) = a y_i + u y_{i+1} + h^2/6 ((a^3 - a) M_i + (u^3 - u) M_{i+1})
        // s'             = (y_{i+1} - y_i) / h + h/6 ((3 u^2 - 1) M_{i+1} - (3 a^2 - 1) M_i)
        const float ca = (a * a * a - a) * (h * h / 6.0f), cb = (u * u * u - u) * (h * h / 6.0f);
        const float da = (3.0f * a * a - 1.0f) * (h / 6.0f), db = (3.0f * u * u - 1.0f) * (h / 6.0f);
        const size_t o = (size_t)b * d + c;
        const Vec<W> e = ld<W>(eps + o);
        Vec<W> vx, vu;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const float mu = fmaf(a, y0.v[q], u * y1.v[q]) + fmaf(ca, m0.v[q], cb * m1.v[q]);
            vx.v[q] = fmaf(sigma_f, e.v[q], mu);
            vu.v[q] = (y1.v[q] - y0.v[q]) / h + fmaf(db, m1.v[q], -(da * m0.v[q]));
        }
        st<W>(xt + o, vx);
        st<W>(ut + o, vu);
        if (c == 0) t_net[b] = fmaf(u, h, (float)s0);
    }
}

extern "C" int cfm_traj_xt_ut_f32(int mode, int variant, const float* X, int B, int T, int d, const int64_t* idx,
                                  const int64_t* t_select, const float* t, const float* eps, double sigma,
                                  const float* sigma_t, int leaveout, const float* S, float* xt, float* ut, float* t_net,
                                  void* stream) {
    if (!X || !t_select || !t || !eps || !xt || !ut || !t_net || B < 0 || T < 2 || d <= 0) return CFM_EINVAL;
    if (mode != 0 && mode != 1) return CFM_EINVAL;
    if (leaveout > 0 && (leaveout > T - 2)) return CFM_EINVAL;      // an interior slice, 1 <= L <= T - 2
    if (leaveout < 0) leaveout = 0;
    if (mode == 0 && variant != CFM_VARIANT_ICFM && variant != CFM_VARIANT_SB && variant != CFM_VARIANT_SCHED) return CFM_EINVAL;
    if (mode == 0 && variant != CFM_VARIANT_ICFM && !sigma_t) return CFM_EINVAL;
    if (mode == 0 && variant == CFM_VARIANT_SCHED && (((uintptr_t)sigma_t) & 15)) return CFM_EALIGN;      // the [B, 4] table
    if (mode == 1) {
        const int Tp = T - (leaveout > 0 ? 1 : 0);
        if (variant != CFM_VARIANT_ICFM || !S || Tp < 2 || Tp > TRAJ_MAX_KNOTS) return CFM_EINVAL;
    }
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    auto al = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    const bool vec = (d % 4 == 0) && al(X) && al(eps) && al(xt) && al(ut);
    const size_t total = (size_t)B * (size_t)(vec ? d / 4 : d);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    const float sf = (float)sigma;
#define CFM_TRAJ_LINEAR(V, W)                                                                                          \
    hipLaunchKernelGGL((traj_linear_kernel<V, W>), dim3(blocks), dim3(256), 0, s, X, B, T, d, idx, t_select, t, eps, sf, \
                       sigma_t, leaveout, xt, ut, t_net)
    if (mode == 0) {
        if (variant == CFM_VARIANT_SB) { if (vec) CFM_TRAJ_LINEAR(CFM_VARIANT_SB, 4); else CFM_TRAJ_LINEAR(CFM_VARIANT_SB, 1); }
        else if (variant == CFM_VARIANT_SCHED) { if (vec) CFM_TRAJ_LINEAR(CFM_VARIANT_SCHED, 4); else CFM_TRAJ_LINEAR(CFM_VARIANT_SCHED, 1); }
        else                           { if (vec) CFM_TRAJ_LINEAR(CFM_VARIANT_ICFM, 4); else CFM_TRAJ_LINEAR(CFM_VARIANT_ICFM, 1); }
    } else {
        if (vec) hipLaunchKernelGGL((traj_spline_kernel<4>), dim3(blocks), dim3(256), 0, s, X, B, T, d, idx, t_select, t, eps,
                                    sf, leaveout, S, xt, ut, t_net);
        else     hipLaunchKernelGGL((traj_spline_kernel<1>), dim3(blocks), dim3(256), 0, s, X, B, T, d, idx, t_select, t, eps,
                                    sf, leaveout, S, xt, ut, t_net);
    }
#undef CFM_TRAJ_LINEAR
    return cfm_status();
}
