// sde_srk.h — per-element arithmetic of one `srk` step, shared by the one-launch sampler (sde_small.h: ode_small_srk)
// and the launch-per-step kernel (elem.hip: sde_srk_step_kernel).  Both call these helpers and nothing else for the
// state updates, which is what makes the two paths bit-equal on the same noise.
//
// The scheme is Roessler's SRI2W1 (strong order 1.5; torchsde's default method "srk" for diagonal Ito noise) with
// CONSTANT g = sigma, where every diffusion-derivative term of the tableau vanishes:
//   I1 = sqrt(h) xi1,  I10 = (h^1.5 / 2) (xi1 + xi2 / sqrt(3))
//   k1 = f(t, y);  k2 = f(t + h, y + h k1);  k3 = f(t + h/2, y + (h/4)(k1 + k2) + (3/2) sigma I10 / h)
//   y+ = y + h (k1 / 6 + k2 / 6 + (2/3) k3) + sigma I1
// Every product-sum is an explicit fmaf in a fixed order (the library is built with -ffp-contract=off).
#pragma once

struct SrkStep {       // per step, filled by the host with float32 casts
    float te1, te2, te3;   // field times of the three stages (reverse: 1 - stage time)
    float h;               // step
    float gs;              // sigma sqrt|h|          (multiplies xi1 in the final update)
    float c3;              // 0.75 sigma sqrt|h|     (multiplies xi1 + xi2 / sqrt(3) in the stage-3 state)
    int is_out, pad;       // trajectory point after this step
};

// drift f = v [+ ssign * s]; v arrives with its sign (reverse time: the caller negates the flow)
__device__ __forceinline__ float srk_drift(float v, float s, bool has_s, float ssign) {
    return has_s ? fmaf(ssign, s, v) : v;
}
// stage-2 state: y + h k1
__device__ __forceinline__ float srk_stage2(float y, float k1, float h) { return fmaf(h, k1, y); }
// stage-3 state: y + (h/4)(k1 + k2) + c3 (xi1 + xi2 / sqrt(3))
__device__ __forceinline__ float srk_stage3(float y, float k1, float k2, float h, float c3, float xi1, float xi2) {
    const float r = fmaf(0.25f * h, k1 + k2, y);
    const float w = fmaf(0.57735026918962576f, xi2, xi1);
    return fmaf(c3, w, r);
}
// y+ = y + (h/6)((k1 + k2) + 4 k3) + gs xi1
__device__ __forceinline__ float srk_final(float y, float k1, float k2, float k3, float h, float gs, float xi1) {
    const float a = fmaf(4.0f, k3, k1 + k2);
    const float r = fmaf(h * 0.16666666666666666f, a, y);
    return fmaf(gs, xi1, r);
}
