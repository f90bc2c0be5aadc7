// elem.hip — K7+K8: fused gather + probability-path sample + conditional flow.
//
// Replaces x0[i], x1[j] (torchcfm/optimal_transport.py:145) and the eager
// elementwise chains of torchcfm/conditional_flow_matching.py:
//   ICFM/OT  :82-83 (mu_t), :126-129 (xt), :153-154 (ut)
//   SB       :446 (sigma_t), :474-478 (ut)
//   Target   :349-350, :368, :393-394
//   VP       :588-589, :617-618
// and, for the scheduled bridge (cfm_sample_xt_ut_sched_f32), the chain of runner/src/models/cfm_module.py:834-850, :856.
// The reference's tests demand bit equality with eager fp32
// (tests/test_conditional_flow_matcher.py:124-126), so every operation below is
// a separately rounded IEEE op in the reference's operation order: the file is
// compiled with contraction off (pragma + -ffp-contract=off) and uses sqrtf / '/'
// (correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt).  NOTE: HIP's f_sqrt/f_div are
// NOT IEEE on ROCm 7.2 without OCML_BASIC_ROUNDED_OPERATIONS (they lower to the
// native approximations) — measured 1-ulp mismatches on gfx950 — so they are not used.  HBM-bound: reads x0[i], x1[j],
// eps once, writes xt, ut once (16-byte accesses when rows allow it).
#include "cfm_common.h"
#include "sde_srk.h"
#pragma clang fp contract(off)

__device__ __forceinline__ float f_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float f_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float f_div(float a, float b) { return a / b; }
__device__ __forceinline__ float f_sqrt(float a) { return sqrtf(a); }

struct RowCoef {       // per-sample scalars
    float c1;          // multiplies x1 in mu
    float c0;          // multiplies x0 in mu
    float sig;         // multiplies eps
    float a;           // variant-specific (SB: sigma'/sigma ratio; Target: 1-(1-s)t)
};

template <int VARIANT>
__device__ __forceinline__ RowCoef row_coef(float t, float sigma_f, float oms_f, const float* c0p,
                                            const float* c1p, int b) {
    RowCoef r;
    if (VARIANT == CFM_VARIANT_ICFM) {
        r.c1 = t; r.c0 = f_sub(1.0f, t); r.sig = sigma_f; r.a = 0.f;
    } else if (VARIANT == CFM_VARIANT_SB) {
        const float omt = f_sub(1.0f, t);
        r.c1 = t; r.c0 = omt;
        // sigma_t = sigma*sqrt(t*(1-t)): taken from the caller's tensor library when provided
        // (c0p) — eager torch.sqrt is NOT correctly rounded on every backend (CPU/MKL deviates
        // by 1 ulp on ~0.6 % of inputs), so bit parity needs the caller's own sqrt; otherwise IEEE.
        r.sig = c0p ? c0p[b] : f_mul(sigma_f, f_sqrt(f_mul(t, omt)));
        const float two_t = f_mul(2.0f, t);
        const float num = f_sub(1.0f, two_t);                             // 1 - 2t
        const float den = f_add(f_mul(two_t, omt), 1e-8f);            // 2t(1-t) + 1e-8
        r.a = f_div(num, den);
    } else if (VARIANT == CFM_VARIANT_TARGET) {
        r.c1 = t; r.c0 = 0.f;
        r.sig = f_sub(1.0f, f_mul(oms_f, t));                         // 1 - (1-sigma) t
        r.a = r.sig;
    } else if (VARIANT == CFM_VARIANT_SCHED) {
        // the packed [B, 4] table of the caller's tensor library (sin, cos and sqrt as eager computes them):
        // r = F(t)/F(1), sigma_t, a = g^2 (1 - 2r) / (2 sigma_t^2 + 1e-8), g^2 / F(1).  t is not read.
        const float4 q = reinterpret_cast<const float4*>(c0p)[b];
        r.c1 = q.x; r.sig = q.y; r.a = q.z; r.c0 = q.w;
    } else {  // VP
        r.c0 = c0p[b]; r.c1 = c1p[b]; r.sig = sigma_f; r.a = 0.f;
    }
    return r;
}

template <int VARIANT>
__device__ __forceinline__ void point(const RowCoef& r, float oms_f, float a0, float a1, float e,
                                      bool have_xt, float xin, float& xt, float& ut) {
    const float HALF_PI = 1.5707963267948966f;
    if (VARIANT == CFM_VARIANT_ICFM) {
        const float mu = f_add(f_mul(r.c1, a1), f_mul(r.c0, a0));
        xt = have_xt ? xin : f_add(mu, f_mul(r.sig, e));
        ut = f_sub(a1, a0);
    } else if (VARIANT == CFM_VARIANT_SB) {
        const float mu = f_add(f_mul(r.c1, a1), f_mul(r.c0, a0));
        xt = have_xt ? xin : f_add(mu, f_mul(r.sig, e));
        ut = f_sub(f_add(f_mul(r.a, f_sub(xt, mu)), a1), a0);
    } else if (VARIANT == CFM_VARIANT_TARGET) {
        const float mu = f_mul(r.c1, a1);
        xt = have_xt ? xin : f_add(mu, f_mul(r.sig, e));
        ut = f_div(f_sub(a1, f_mul(oms_f, xt)), r.a);
    } else if (VARIANT == CFM_VARIANT_SCHED) {
        // mu = x0 + (x1 - x0) r;  ut = a (xt - mu) + (x1 - x0) g^2/F(1): ScheduledBridgeConditionalFlowMatcher's order
        const float dx = f_sub(a1, a0);
        const float mu = f_add(a0, f_mul(dx, r.c1));
        xt = have_xt ? xin : f_add(mu, f_mul(r.sig, e));
        ut = f_add(f_mul(r.a, f_sub(xt, mu)), f_mul(dx, r.c0));
    } else {
        const float mu = f_add(f_mul(r.c0, a0), f_mul(r.c1, a1));
        xt = have_xt ? xin : f_add(mu, f_mul(r.sig, e));
        ut = f_mul(HALF_PI, f_sub(f_mul(r.c0, a1), f_mul(r.c1, a0)));
    }
}

template <int VARIANT, bool VEC>
__global__ __launch_bounds__(256) void xt_ut_kernel(const float* __restrict__ x0,
                                                    const float* __restrict__ x1,
                                                    const int64_t* __restrict__ gi,
                                                    const int64_t* __restrict__ gj,
                                                    const float* __restrict__ t,
                                                    const float* __restrict__ eps, float sigma_f,
                                                    float oms_f, const float* __restrict__ c0p,
                                                    const float* __restrict__ c1p,
                                                    const float* __restrict__ xt_in, int B, int d,
                                                    float* __restrict__ xt, float* __restrict__ ut,
                                                    float* __restrict__ x0g,
                                                    float* __restrict__ x1g) {
    constexpr int W = VEC ? 4 : 1;
    const size_t per_row = (size_t)d / W;
    const size_t total = (size_t)B * per_row;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
        const int b = (int)(g / per_row);
        const size_t k = (g - (size_t)b * per_row) * W;
        const size_t r0 = gi ? (size_t)gi[b] : (size_t)b;
        const size_t r1 = gj ? (size_t)gj[b] : (size_t)b;
        const RowCoef rc = row_coef<VARIANT>(VARIANT == CFM_VARIANT_SCHED ? 0.f : t[b], sigma_f, oms_f, c0p, c1p, b);
        const size_t o = (size_t)b * d + k;
        if (VEC) {
            const float4 a0 = *reinterpret_cast<const float4*>(x0 + r0 * d + k);
            const float4 a1 = *reinterpret_cast<const float4*>(x1 + r1 * d + k);
            const float4 e = eps ? *reinterpret_cast<const float4*>(eps + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            const bool hx = xt_in != nullptr;
            const float4 xi = hx ? *reinterpret_cast<const float4*>(xt_in + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 vx, vu;
            point<VARIANT>(rc, oms_f, a0.x, a1.x, e.x, hx, xi.x, vx.x, vu.x);
            point<VARIANT>(rc, oms_f, a0.y, a1.y, e.y, hx, xi.y, vx.y, vu.y);
            point<VARIANT>(rc, oms_f, a0.z, a1.z, e.z, hx, xi.z, vx.z, vu.z);
            point<VARIANT>(rc, oms_f, a0.w, a1.w, e.w, hx, xi.w, vx.w, vu.w);
            if (xt) *reinterpret_cast<float4*>(xt + o) = vx;
            *reinterpret_cast<float4*>(ut + o) = vu;
            if (x0g) *reinterpret_cast<float4*>(x0g + o) = a0;
            if (x1g) *reinterpret_cast<float4*>(x1g + o) = a1;
        } else {
            const float a0 = x0[r0 * d + k], a1 = x1[r1 * d + k], e = eps ? eps[o] : 0.f;
            const bool hx = xt_in != nullptr;
            float vx, vu;
            point<VARIANT>(rc, oms_f, a0, a1, e, hx, hx ? xt_in[o] : 0.f, vx, vu);
            if (xt) xt[o] = vx;
            ut[o] = vu;
            if (x0g) x0g[o] = a0;
            if (x1g) x1g[o] = a1;
        }
    }
}

template <int VARIANT>
static void launch_xt_ut(bool vec, int blocks, hipStream_t s, const float* x0, const float* x1,
                         const int64_t* i, const int64_t* j, const float* t, const float* eps,
                         float sf, float of, const float* c0, const float* c1, const float* xin, int B, int d, float* xt,
                         float* ut, float* x0g, float* x1g) {
    if (vec) hipLaunchKernelGGL((xt_ut_kernel<VARIANT, true>), dim3(blocks), dim3(256), 0, s, x0, x1, i, j, t, eps, sf, of, c0, c1, xin, B, d, xt, ut, x0g, x1g);
    else     hipLaunchKernelGGL((xt_ut_kernel<VARIANT, false>), dim3(blocks), dim3(256), 0, s, x0, x1, i, j, t, eps, sf, of, c0, c1, xin, B, d, xt, ut, x0g, x1g);
}

extern "C" int cfm_sample_xt_ut_f32(int variant, const float* x0, const float* x1, const int64_t* i,
                                    const int64_t* j, const float* t, const float* eps, double sigma,
                                    const float* c0, const float* c1, const float* xin, int B, int d,
                                    float* xt, float* ut, float* x0g, float* x1g, void* stream) {
    if (!x0 || !x1 || !t || !ut || B < 0 || d <= 0) return CFM_EINVAL;
    if (!xin && (!eps || !xt)) return CFM_EINVAL;
    if (variant < 0 || variant > 3) return CFM_EINVAL;
    if (variant == CFM_VARIANT_VP && (!c0 || !c1)) return CFM_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const float sf = (float)sigma;
    const float of = (float)(1.0 - sigma);
    auto al = [](const void* p) { return p == nullptr || (((uintptr_t)p) & 15) == 0; };
    const bool vec = (d % 4 == 0) && al(x0) && al(x1) && al(eps) && al(xt) && al(ut) && al(x0g) && al(x1g) && al(xin);
    const size_t total = (size_t)B * (size_t)(vec ? d / 4 : d);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    switch (variant) {
        case CFM_VARIANT_ICFM:   launch_xt_ut<CFM_VARIANT_ICFM>(vec, blocks, s, x0, x1, i, j, t, eps, sf, of, c0, c1, xin, B, d, xt, ut, x0g, x1g); break;
        case CFM_VARIANT_SB:     launch_xt_ut<CFM_VARIANT_SB>(vec, blocks, s, x0, x1, i, j, t, eps, sf, of, c0, c1, xin, B, d, xt, ut, x0g, x1g); break;
        case CFM_VARIANT_TARGET: launch_xt_ut<CFM_VARIANT_TARGET>(vec, blocks, s, x0, x1, i, j, t, eps, sf, of, c0, c1, xin, B, d, xt, ut, x0g, x1g); break;
        default:                 launch_xt_ut<CFM_VARIANT_VP>(vec, blocks, s, x0, x1, i, j, t, eps, sf, of, c0, c1, xin, B, d, xt, ut, x0g, x1g); break;
    }
    return cfm_status();
}

// The scheduled bridge (ScheduledBridgeConditionalFlowMatcher: the [SF]2M path with a noise schedule g(t),
// runner/src/models/cfm_module.py:834-850 with the flow coefficient (d sigma_t/dt)/sigma_t) on the same kernel: the four
// per-row scalars arrive as one packed [B, 4] table, read with one 16-byte load per row.
extern "C" int cfm_sample_xt_ut_sched_f32(const float* x0, const float* x1, const int64_t* i, const int64_t* j,
                                          const float* coef, const float* eps, const float* xin, int B, int d,
                                          float* xt, float* ut, void* stream) {
    if (!x0 || !x1 || !coef || !ut || B < 0 || d <= 0) return CFM_EINVAL;
    if (!xin && (!eps || !xt)) return CFM_EINVAL;
    if (((uintptr_t)coef) & 15) return CFM_EALIGN;
    if (B == 0) return 0;
    auto al = [](const void* p) { return p == nullptr || (((uintptr_t)p) & 15) == 0; };
    const bool vec = (d % 4 == 0) && al(x0) && al(x1) && al(eps) && al(xt) && al(ut) && al(xin);
    const size_t total = (size_t)B * (size_t)(vec ? d / 4 : d);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    launch_xt_ut<CFM_VARIANT_SCHED>(vec, blocks, (hipStream_t)stream, x0, x1, i, j, nullptr, eps, 0.f, 0.f, coef, nullptr,
                                    xin, B, d, xt, ut, nullptr, nullptr);
    return cfm_status();
}

// DSBM (DSBMConditionalFlowMatcher): the scheduled bridge's x_t and the two drift targets that the forward and the backward
// net regress, runner/src/models/cfm_module.py:834-841 (mu_t, sigma_t), :1187-1200 (x_t, the targets).  The xt_ut_kernel
// loop with three outputs: the per-row scalars arrive as one packed [B, 4] table (r, sigma_t, cf, cb), one 16-byte load
// per row; every op separately rounded, in the matcher's eager order:
//   dx = x1 - x0;  mu = x0 + dx r;  xt = mu + sigma_t eps;  ft = dx - cf eps;  bt = (x0 - x1) - cb eps
__device__ __forceinline__ void dsbm_point(const float4& q, float a0, float a1, float e, float& xt, float& ft, float& bt) {
    const float dx = f_sub(a1, a0);
    const float mu = f_add(a0, f_mul(dx, q.x));
    xt = f_add(mu, f_mul(q.y, e));
    ft = f_sub(dx, f_mul(q.z, e));
    bt = f_sub(f_sub(a0, a1), f_mul(q.w, e));
}

template <bool VEC>
__global__ __launch_bounds__(256) void dsbm_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                   const int64_t* __restrict__ gi, const int64_t* __restrict__ gj,
                                                   const float* __restrict__ coef, const float* __restrict__ eps, int B, int d,
                                                   float* __restrict__ xt, float* __restrict__ ft, float* __restrict__ bt) {
    constexpr int W = VEC ? 4 : 1;
    const size_t per_row = (size_t)d / W;
    const size_t total = (size_t)B * per_row;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
        const int b = (int)(g / per_row);
        const size_t k = (g - (size_t)b * per_row) * W;
        const size_t r0 = gi ? (size_t)gi[b] : (size_t)b;
        const size_t r1 = gj ? (size_t)gj[b] : (size_t)b;
        const float4 q = reinterpret_cast<const float4*>(coef)[b];
        const size_t o = (size_t)b * d + k;
        if (VEC) {
            const float4 a0 = *reinterpret_cast<const float4*>(x0 + r0 * d + k);
            const float4 a1 = *reinterpret_cast<const float4*>(x1 + r1 * d + k);
            const float4 e = *reinterpret_cast<const float4*>(eps + o);
            float4 vx, vf, vb;
            dsbm_point(q, a0.x, a1.x, e.x, vx.x, vf.x, vb.x);
            dsbm_point(q, a0.y, a1.y, e.y, vx.y, vf.y, vb.y);
            dsbm_point(q, a0.z, a1.z, e.z, vx.z, vf.z, vb.z);
            dsbm_point(q, a0.w, a1.w, e.w, vx.w, vf.w, vb.w);
            *reinterpret_cast<float4*>(xt + o) = vx;
            *reinterpret_cast<float4*>(ft + o) = vf;
            *reinterpret_cast<float4*>(bt + o) = vb;
        } else {
            float vx, vf, vb;
            dsbm_point(q, x0[r0 * d + k], x1[r1 * d + k], eps[o], vx, vf, vb);
            xt[o] = vx; ft[o] = vf; bt[o] = vb;
        }
    }
}

extern "C" int cfm_sample_dsbm_f32(const float* x0, const float* x1, const int64_t* i, const int64_t* j, const float* coef,
                                   const float* eps, int B, int d, float* xt, float* ft, float* bt, void* stream) {
    if (!x0 || !x1 || !coef || !eps || !xt || !ft || !bt || B < 0 || d <= 0) return CFM_EINVAL;
    if (((uintptr_t)coef) & 15) return CFM_EALIGN;
    if (B == 0) return 0;
    auto al = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    const bool vec = (d % 4 == 0) && al(x0) && al(x1) && al(eps) && al(xt) && al(ft) && al(bt);
    const size_t total = (size_t)B * (size_t)(vec ? d / 4 : d);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    if (vec) hipLaunchKernelGGL(dsbm_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x0, x1, i, j, coef, eps, B, d, xt, ft, bt);
    else     hipLaunchKernelGGL(dsbm_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x0, x1, i, j, coef, eps, B, d, xt, ft, bt);
    return cfm_status();
}

// generic row gather (labels y0[i], y1[j]; also x0[i], x1[j] for sample_plan)
__global__ __launch_bounds__(256) void gather_rows_kernel(const unsigned char* __restrict__ src,
                                                          const int64_t* __restrict__ idx, int n,
                                                          size_t row_bytes,
                                                          unsigned char* __restrict__ out, int w16) {
    if (w16) {
        const size_t per_row = row_bytes / 16;
        const size_t total = (size_t)n * per_row;
        for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
            const size_t b = g / per_row, k = g - b * per_row;
            reinterpret_cast<uint4*>(out + b * row_bytes)[k] =
                reinterpret_cast<const uint4*>(src + (size_t)idx[b] * row_bytes)[k];
        }
    } else {
        const size_t total = (size_t)n * row_bytes;
        for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
            const size_t b = g / row_bytes, k = g - b * row_bytes;
            out[b * row_bytes + k] = src[(size_t)idx[b] * row_bytes + k];
        }
    }
}

extern "C" int cfm_gather_rows(const void* src, const int64_t* idx, int n, size_t row_bytes, void* out,
                               void* stream) {
    if (n < 0) return CFM_EINVAL;
    if (n == 0 || row_bytes == 0) return 0;      // (an empty index or output tensor has a null data pointer)
    if (!src || !idx || !out) return CFM_EINVAL;
    const int w16 = (row_bytes % 16 == 0) && (((uintptr_t)src & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const size_t total = (size_t)n * (w16 ? row_bytes / 16 : row_bytes);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)src, idx, n, row_bytes, (unsigned char*)out, w16);
    return cfm_status();
}

// ---------------------------------------------------------------- SDE step ----
// One Euler-Maruyama step of dy = (v + s) dt + g dW (SF2M sampling: f = drift(x) + score(x), g = sigma under
// torchsde.sdeint(..., method="euler"): runner/src/models/components/solver.py:157-182 at sde_solver: euler.  The
// notebooks run torchsde's default "srk" instead — sde_srk_step_kernel below):
//   y <- y + dt * (v [+ s]) + g * sqrt_dt * xi
// v, s: drift and score network outputs, xi ~ N(0, 1) drawn by the caller's generator.  In place.
__global__ __launch_bounds__(256) void sde_em_step_kernel(float* __restrict__ y, const float* __restrict__ v,
                                                          const float* __restrict__ s, const float* __restrict__ xi,
                                                          float dt, float g_sqrt_dt, float ssign, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        float f = v[e];
        if (s) f = fmaf(ssign, s[e], f);
        float r = fmaf(dt, f, y[e]);
        if (xi) r = fmaf(g_sqrt_dt, xi[e], r);
        y[e] = r;
    }
}

extern "C" int cfm_sde_em_step_f32(float* y, const float* v, const float* s, const float* xi, double dt, double g,
                                   double score_sign, size_t n, void* stream) {
    if (!y || !v) return CFM_EINVAL;
    if (n == 0) return 0;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sde_em_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, y, v, s, xi, (float)dt,
                       (float)(g * sqrt(fabs(dt))), (float)score_sign, n);
    return cfm_status();
}

// One stage of an `srk` step (sde_srk.h: SRI2W1 with constant g, torchsde's default method for the reference's
// SDE classes: the default-method torchsde.sdeint calls of single-cell_example.ipynb / mnist_example.ipynb /
// conditional_mnist.ipynb / SF2M_tutorial.ipynb cell 5, and runner/src/models/components/solver.py:169-179 at
// sde_solver: srk) for fields that do not fit the one-launch sampler.  f_i = v_i + ssign * s_i as above.
//   stage 1: ys = y + h f1          stage 2: ys = y + (h/4)(f1 + f2) + c3 (xi1 + xi2 / sqrt(3))
//   stage 3: y <- y + (h/6)(f1 + f2 + 4 f3) + gs xi1      (in place)
template <int STAGE>
__global__ __launch_bounds__(256) void sde_srk_step_kernel(float* __restrict__ y, float* __restrict__ ys,
                                                           const float* __restrict__ v1, const float* __restrict__ s1,
                                                           const float* __restrict__ v2, const float* __restrict__ s2,
                                                           const float* __restrict__ v3, const float* __restrict__ s3,
                                                           const float* __restrict__ xi1, const float* __restrict__ xi2,
                                                           float h, float gs, float c3, float ssign, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float k1 = srk_drift(v1[e], s1 ? s1[e] : 0.f, s1 != nullptr, ssign);
        if (STAGE == 1) { ys[e] = srk_stage2(y[e], k1, h); continue; }
        const float k2 = srk_drift(v2[e], s2 ? s2[e] : 0.f, s2 != nullptr, ssign);
        const float z1 = xi1 ? xi1[e] : 0.f;
        if (STAGE == 2) { ys[e] = srk_stage3(y[e], k1, k2, h, c3, z1, xi2 ? xi2[e] : 0.f); continue; }
        const float k3 = srk_drift(v3[e], s3 ? s3[e] : 0.f, s3 != nullptr, ssign);
        y[e] = srk_final(y[e], k1, k2, k3, h, gs, z1);
    }
}

extern "C" int cfm_sde_srk_step_f32(int stage, float* y, float* ys, const float* v1, const float* s1, const float* v2,
                                    const float* s2, const float* v3, const float* s3, const float* xi1,
                                    const float* xi2, double h, double g, double score_sign, size_t n, void* stream) {
    if (stage < 1 || stage > 3 || !y || !v1) return CFM_EINVAL;
    if (stage < 3 && (!ys || ys == y)) return CFM_EINVAL;
    if (stage >= 2 && !v2) return CFM_EINVAL;
    if (stage == 3 && !v3) return CFM_EINVAL;
    if (n == 0) return 0;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    const float gs = (float)(g * sqrt(fabs(h))), c3 = (float)(0.75 * g * sqrt(fabs(h)));
    hipStream_t st = (hipStream_t)stream;
#define CFM_SRK_STAGE(K)                                                                                              \
    hipLaunchKernelGGL(sde_srk_step_kernel<K>, dim3(blocks), dim3(256), 0, st, y, ys, v1, s1, v2, s2, v3, s3, xi1, xi2, \
                       (float)h, gs, c3, (float)score_sign, n)
    if (stage == 1) CFM_SRK_STAGE(1); else if (stage == 2) CFM_SRK_STAGE(2); else CFM_SRK_STAGE(3);
#undef CFM_SRK_STAGE
    return cfm_status();
}

// ------------------------------------------------------- mixture-RBF sums ----
// sum over a squared-distance matrix D of sum_sigma exp(-D / (2 sigma^2)): the three kernel sums of the
// mixture-RBF MMD (runner/src/models/components/mmd.py:43-63,80-110) without materialising any kernel
// matrix.  fp64 accumulation, one atomic per workgroup.  out[0] += the sum (caller zeroes it).
__global__ __launch_bounds__(256) void rbf_mix_sum_kernel(const float* __restrict__ D, size_t n,
                                                          const float* __restrict__ gammas, int ng,
                                                          double* __restrict__ out) {
    double acc = 0.0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float dsq = D[e];
        float k = 0.f;
        for (int q = 0; q < ng; ++q) k += expf(-gammas[q] * dsq);
        acc += (double)k;
    }
    acc = wave_sum_d(acc);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, (sh[0] + sh[1]) + (sh[2] + sh[3]));
}

extern "C" int cfm_rbf_mix_sum_f32(const float* D, size_t n, const float* gammas, int n_gamma, double* out,
                                   void* stream) {
    if (!D || !gammas || !out || n_gamma < 1) return CFM_EINVAL;
    if (n == 0) return 0;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(rbf_mix_sum_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, D, n, gammas, n_gamma, out);
    return cfm_status();
}
