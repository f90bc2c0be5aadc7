// ode_tableau.h — the Runge-Kutta tableaus of the ODE solvers (ode.hip) and of their gradient kernels (small_grad.hip:
// ode_grad.h, ode_adaptive_grad.h): one definition that both translation units see.
#pragma once

// ---- tableaus ----------------------------------------------------------------------------------------------------
// Entries as compile-time constants: in the kernels every index is a constant after unrolling, the host drivers
// read the same tables.  Every use casts the fp64 constant: (float)rk_a<TAB>(s, q), (float)rk_e<TAB>(q).
// Adaptive pairs (7 stages, FSAL, row 6 of a = b, so stage 6's y is x_new; e = b - b_alt):
//   CFM_ODE_DOPRI5: Dormand-Prince 5(4);  CFM_ODE_TSIT5: Tsitouras 5(4) (Tsitouras 2011, the
//   coefficients torchdyn's default solver carries).
template <int TAB>
__host__ __device__ __forceinline__ double rk_a(int s, int q) {
    if constexpr (TAB == CFM_ODE_TSIT5) {
        constexpr double A[6][6] = {
            {0.161, 0, 0, 0, 0, 0},
            {-0.008480655492356989, 0.335480655492357, 0, 0, 0, 0},
            {2.8971530571054935, -6.359448489975075, 4.3622954328695815, 0, 0, 0},
            {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525, 0, 0},
            {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383, 0},
            {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774}};
        return A[s][q];
    } else {
        constexpr double A[6][6] = {
            {1.0 / 5, 0, 0, 0, 0, 0},
            {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
            {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
            {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
            {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
            {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
        return A[s][q];
    }
}
template <int TAB>
__host__ __device__ __forceinline__ float rk_c(int s) {
    if constexpr (TAB == CFM_ODE_TSIT5) {
        constexpr float C[6] = {(float)0.161, (float)0.327, (float)0.9, (float)0.9800255409045097, 1.f, 1.f};
        return C[s];
    } else {
        constexpr float C[6] = {1.f / 5, 3.f / 10, 4.f / 5, 8.f / 9, 1.f, 1.f};
        return C[s];
    }
}
template <int TAB>
__host__ __device__ __forceinline__ double rk_e(int q) {
    if constexpr (TAB == CFM_ODE_TSIT5) {
        constexpr double E[7] = {0.001780011052226, 0.000816434459657, -0.007880878010262, 0.144711007173263,
                                 -0.582357165452555, 0.458082105929187, -1.0 / 66};
        return E[q];
    } else {
        constexpr double BS[7] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0};
        constexpr double BA[7] = {1951.0 / 21600, 0, 22642.0 / 50085, 451.0 / 720, -12231.0 / 42400, 649.0 / 6300, 1.0 / 60};
        return BS[q] - BA[q];
    }
}
static double rk_a_host(int tab, int s, int q) { return tab == CFM_ODE_TSIT5 ? rk_a<CFM_ODE_TSIT5>(s, q) : rk_a<CFM_ODE_DOPRI5>(s, q); }
static float rk_c_host(int tab, int s) { return tab == CFM_ODE_TSIT5 ? rk_c<CFM_ODE_TSIT5>(s) : rk_c<CFM_ODE_DOPRI5>(s); }
static double rk_e_host(int tab, int q) { return tab == CFM_ODE_TSIT5 ? rk_e<CFM_ODE_TSIT5>(q) : rk_e<CFM_ODE_DOPRI5>(q); }
static int rk_adaptive_known(int tab) { return tab == CFM_ODE_DOPRI5 || tab == CFM_ODE_TSIT5; }

// Fixed-step schemes: stage s >= 1 is y = x + dt * sum_{q<s} a[s-1][q] k_q at t + c[s-1] dt; x_new = x + dt * sum b k.
//   CFM_ODE_EULER;  CFM_ODE_MIDPOINT: x + dt f(t + dt/2, x + dt/2 k1);  CFM_ODE_RK4: the 3/8 rule.
template <int SCHEME>
__host__ __device__ __forceinline__ constexpr int fx_stages() { return SCHEME == CFM_ODE_RK4 ? 4 : SCHEME == CFM_ODE_MIDPOINT ? 2 : 1; }
template <int SCHEME>
__host__ __device__ __forceinline__ double fx_a(int s, int q) {
    if constexpr (SCHEME == CFM_ODE_RK4) {
        constexpr double A[3][3] = {{1.0 / 3, 0, 0}, {-1.0 / 3, 1, 0}, {1, -1, 1}};
        return A[s][q];
    } else {
        constexpr double A[3][3] = {{1.0 / 2, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        return A[s][q];
    }
}
template <int SCHEME>
__host__ __device__ __forceinline__ double fx_c(int s) {
    if constexpr (SCHEME == CFM_ODE_RK4) {
        constexpr double C[3] = {1.0 / 3, 2.0 / 3, 1};
        return C[s];
    } else {
        constexpr double C[3] = {1.0 / 2, 0, 0};
        return C[s];
    }
}
template <int SCHEME>
__host__ __device__ __forceinline__ double fx_b(int q) {
    if constexpr (SCHEME == CFM_ODE_RK4) {
        constexpr double Bv[4] = {1.0 / 8, 3.0 / 8, 3.0 / 8, 1.0 / 8};
        return Bv[q];
    } else if constexpr (SCHEME == CFM_ODE_MIDPOINT) {
        constexpr double Bv[4] = {0, 1, 0, 0};
        return Bv[q];
    } else {
        constexpr double Bv[4] = {1, 0, 0, 0};
        return Bv[q];
    }
}
static int fx_known(int scheme) { return scheme == CFM_ODE_EULER || scheme == CFM_ODE_MIDPOINT || scheme == CFM_ODE_RK4; }
static int fx_stages_host(int scheme) { return scheme == CFM_ODE_RK4 ? 4 : scheme == CFM_ODE_MIDPOINT ? 2 : 1; }
static double fx_a_host(int sc, int s, int q) { return sc == CFM_ODE_RK4 ? fx_a<CFM_ODE_RK4>(s, q) : fx_a<CFM_ODE_MIDPOINT>(s, q); }
static double fx_c_host(int sc, int s) { return sc == CFM_ODE_RK4 ? fx_c<CFM_ODE_RK4>(s) : fx_c<CFM_ODE_MIDPOINT>(s); }
static double fx_b_host(int sc, int q) {
    return sc == CFM_ODE_RK4 ? fx_b<CFM_ODE_RK4>(q) : sc == CFM_ODE_MIDPOINT ? fx_b<CFM_ODE_MIDPOINT>(q) : fx_b<CFM_ODE_EULER>(q);
}
