/*
 * cfm_gfx950.h — C ABI of libcfm_gfx950.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the minibatch-OT coupling + CFM sampling hot path of
 * TorchCFM (atong01/conditional-flow-matching).  The reference has no FFI of
 * its own (it is pure Python); each entry point below replaces the third-party
 * native routine or eager-op chain that the cited reference line executes.
 * Citations are relative to the reference repository root.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (contiguous,
 *     row-major) unless the parameter is documented "host";
 *   - `stream` is a hipStream_t passed as void*; ALL work (launches, memsets, copies) is enqueued on it and the
 *     call returns without synchronising, EXCEPT cfm_assign_exact_f32, cfm_assign_exact_batch_f32 and the ADAPTIVE
 *     solves (cfm_ode_dopri5_mlp_f32, cfm_ode_adaptive_mlp_f32, cfm_ode_adaptive_rec_mlp_f32,
 *     cfm_ode_dopri5_cnf_mlp_f32, cfm_ode_adaptive_cnf_mlp_f32, cfm_ode_adaptive_gradmlp_f32) whose control flow is
 *     data dependent: they pump their step kernels on `stream` and read a few bytes of device state back, so they
 *     return only when the result is resident in the output buffers.  The fixed-step solves (cfm_ode_euler_*,
 *     cfm_ode_fixed_*), the SDE trajectories and every gradient entry are asynchronous like the rest: their nfe is
 *     known on the host, their trajectory is ready when `stream` reaches it;
 *   - a HOST array passed to an entry (pointer tables, dims, t_span, step records) may be overwritten or freed as
 *     soon as the call returns, also by the asynchronous entries: the tables are read during the call, and the
 *     data arrays are copied with hipMemcpyAsync from pageable memory, which the runtime stages before it returns
 *     (tests/test_gpu_stream_contract.py overwrites each behind a busy stream, at up to 640 KB);
 *   - no entry point allocates or frees device memory: scratch comes from the
 *     caller through `ws` (size from cfm_workspace_bytes);
 *   - the contents of `ws` and of every output buffer on entry are ARBITRARY (stale bytes of another solve, zeros, NaN
 *     patterns): an entry initialises every word it waits on, sums into or indexes by, on `stream`, and writes its
 *     outputs whole.  Nothing outside the output buffers and the first cfm_workspace_bytes bytes of `ws` (for the
 *     entries that state their own size: those bytes) is written, and inputs are not modified, except by the entries
 *     documented as in place (cfm_scale_inv_f32, cfm_sqrt_inplace_f32, cfm_adam_step_f32, cfm_sde_em_step_f32).  The
 *     one precondition on an output is stated where it holds: `out` of cfm_rbf_mix_sum_f32 is zeroed by the caller.
 *     Where an entry declines a shape (CFM_EINVAL for a t_span that does not fit its scratch, for a solve outside
 *     the one-launch kernel's envelope), the declining call has written nothing.
 *     (tests/test_gpu_memory_contract.py: every entry on 0x00-, 0xFF- and stale-filled buffers between guard zones);
 *   - return value: 0 = ok, <0 = invalid argument (CFM_E*), >0 = hipError_t;
 *   - no exceptions cross the boundary; no global state except a lazily
 *     initialised per-device properties cache, per HOST THREAD the captured launch
 *     programs (hipGraphs) of the exact solver's last four (workspace, size, batch,
 *     stream) combinations + 2 KiB of pinned memory, per HOST THREAD 64 bytes of pinned memory the adaptive ODE
 *     drivers read their norms and controller words back through (allocated by the thread's first adaptive solve;
 *     host threads on their own streams never share a read-back buffer), one process-wide mutex that lets ONE
 *     persistent adaptive solve run at a time, and the solver-parameter table
 *     of include/cfm_gfx950_tuning.h (measurement / tuning exports that no
 *     binding needs; a solve snapshots the table under a mutex when it starts).
 */
#ifndef CFM_GFX950_H
#define CFM_GFX950_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: only what this header (and cfm_gfx950_tuning.h) declares leaves it. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define CFM_ABI_VERSION 3

/* error codes (negative) */
#define CFM_EINVAL   (-1)  /* bad shape / null pointer / unsupported size      */
#define CFM_EALIGN   (-2)  /* pointer not aligned as documented                */
#define CFM_ENOCONV  (-3)  /* solver hit its step cap without a certificate    */
#define CFM_ETIMEOUT (-4)  /* device state machine made no progress            */

/* ops for cfm_workspace_bytes */
#define CFM_OP_SINKHORN      1
#define CFM_OP_ASSIGN        2
#define CFM_OP_SAMPLE_DENSE  3
#define CFM_OP_MLP           4
#define CFM_OP_ODE           5
#define CFM_OP_UNBALANCED    6   /* also the partial (Dykstra) solver */
#define CFM_OP_COST          7   /* cfm_sqeuclid_cost_ws_f32 (B0, B1, d)  */
#define CFM_OP_MLP_TRAIN     8   /* cfm_mlp_backward_f32 (B, widest layer, largest weight's element count) */
#define CFM_OP_TRANSPORT     9   /* cfm_transport_exact_f32 (B0, B1, 0) */
#define CFM_OP_CNF_GRAD     10   /* cfm_cnf_euler_grad_f32 (B, n_t, 0): per-workgroup partial gradients + t_span */
#define CFM_OP_ACTION_GRAD  11   /* cfm_action_matching_grad_f32 (B, 0, 0): per-workgroup partial gradients + loss terms */
#define CFM_OP_ODE_GRAD     12   /* cfm_ode_fixed_grad_f32, cfm_ode_adaptive_grad_f32 (B, n_t, 0): per-workgroup partial gradients + t_span */

/* variants for cfm_sample_xt_ut_f32 (reference class in parentheses) */
#define CFM_VARIANT_ICFM   0  /* ConditionalFlowMatcher / ExactOT...          */
#define CFM_VARIANT_SB     1  /* SchrodingerBridgeConditionalFlowMatcher      */
#define CFM_VARIANT_TARGET 2  /* TargetConditionalFlowMatcher                 */
#define CFM_VARIANT_VP     3  /* VariancePreservingConditionalFlowMatcher     */
/* the scheduled bridge (cfm_sample_xt_ut_sched_f32, cfm_traj_xt_ut_f32 mode 0 only; cfm_sample_xt_ut_f32 refuses it) */
#define CFM_VARIANT_SCHED  4  /* ScheduledBridgeConditionalFlowMatcher (runner's SF2M with a NoiseScheduler) */

int cfm_abi_version(void);

/* Bytes of device scratch an op needs for the given problem (0 on bad op). */
size_t cfm_workspace_bytes(int op, int B0, int B1, int d);

/* Runtime — a HIP stream restricted to a subset of the chip's compute units (hipExtStreamCreateWithCUMask).
 * The reference overlaps nothing: its coupling runs on the host between two model steps
 * (torchcfm/conditional_flow_matching.py:271-272, examples/images/cifar10/train_cifar10.py:141-151).  Here the
 * couplings of the next minibatches run beside the model step (cfm_amd.prefetch); the latency-bound rounds of the
 * exact solver and the dense fp32-MFMA products then fight for workgroup slots on every CU unless the chip is
 * PARTITIONED: solver streams on one CU subset, dense streams on the complement.
 * cu_mask: HOST array of n_words 32-bit words; bit i = logical CU i of the current device (gfx950 in SPX mode:
 * XCD i % 8, CU i / 8 of that XCD); every XCD must keep at least one CU (CFM_EINVAL otherwise: a queue without
 * CUs on one XCD never drains).  *stream receives a hipStream_t the caller owns (cfm_stream_destroy). */
int cfm_stream_create_cu_mask(const uint32_t* cu_mask, int n_words, void** stream);
int cfm_stream_destroy(void* stream);

/* K1 — squared-Euclidean cost matrix  M[i,j] = sum_k (x0[i,k]-x1[j,k])^2.
 * Replaces  torch.cdist(x0, x1) ** 2       torchcfm/optimal_transport.py:84
 * (also :176, :297 with power 1 -> see cfm_euclid_cost_f32).
 * If opt_max != NULL it receives max(M) (one float; for normalize_cost, :85-86).
 * x0 [B0,d], x1 [B1,d], M [B0,B1], fp32. */
int cfm_sqeuclid_cost_f32(const float* x0, const float* x1, int B0, int B1, int d,
                          float* M, float* opt_max, void* stream);

/* K1, matrix-core form — same contract and result class as cfm_sqeuclid_cost_f32, with scratch:
 * for d >= 64 and B0, B1 >= 256 the Gram form |a|^2 + |b|^2 - 2<a,b> of the points centred on a
 * sample mean runs on v_mfma_f32_32x32x2_f32, and every entry where that form cancels (result
 * below 1/8 of |a|^2 + |b|^2: near-duplicates, an x-vs-x diagonal) is recomputed in the
 * direct-difference form; other shapes take the direct kernels of cfm_sqeuclid_cost_f32.
 * ws: cfm_workspace_bytes(CFM_OP_COST,B0,B1,d) bytes, 16-byte aligned. */
int cfm_sqeuclid_cost_ws_f32(const float* x0, const float* x1, int B0, int B1, int d,
                             float* M, float* opt_max, void* ws, void* stream);

/* M[i] *= 1/(*maxval)   — `M / M.max()`     torchcfm/optimal_transport.py:86 */
int cfm_scale_inv_f32(float* M, size_t n, const float* maxval, void* stream);

/* In-place sqrt — Euclidean (power=1) cost for wasserstein(), :297-299. */
int cfm_sqrt_inplace_f32(float* M, size_t n, void* stream);

/* K5 — log-domain Sinkhorn with POT loop semantics (uniform marginals).
 * Replaces  pot.sinkhorn(a, b, M, reg)      torchcfm/optimal_transport.py:51,87
 * in its numerically stable form (POT method="sinkhorn_log"): u0 = 0,
 *   v = log b - LSE_i(-M/reg + u),  u = log a - LSE_j(-M/reg + v),
 * marginal check every `check_every` iterations (ii % check_every == 0):
 * err = || sum_i exp(-M/reg + u + v) - b ||_2 ; stop when err < stop_thr or
 * after max_iter iterations (reg, stop_thr are doubles: the reference passes
 * Python floats to POT).  The iteration runs with fp32 exp() (HBM-bound fast
 * path) and switches itself to fp64 exp once the measured violation approaches
 * the fp32 noise floor, so stop_thr = 1e-9 is honoured.  Outputs f = reg*u [B0],
 * g = reg*v [B1] (fp32), *iters_done, *last_err (device scalars).
 * ws: cfm_workspace_bytes(CFM_OP_SINKHORN,B0,B1,0) bytes, 16-byte aligned;
 * it keeps the fp64 potentials (see cfm_sinkhorn_potentials_f64). */
int cfm_sinkhorn_log_f32(const float* M, int B0, int B1, double reg, int max_iter,
                         double stop_thr, int check_every, float* f, float* g,
                         int* iters_done, float* last_err, void* ws, void* stream);

/* K5, variant B — the same solve for low-dimensional clouds (1 <= d <= 8) with the cost entry
 * recomputed from the coordinates inside the LSE passes instead of streamed from the B0 x B1 matrix
 * (cdist at torchcfm/optimal_transport.py:84 + pot.sinkhorn at :51,87 in one: no B^2 traffic).  The
 * entry is formed exactly as cfm_sqeuclid_cost_f32 forms it for d <= 8, so f, g and the potentials in
 * `ws` belong to that matrix and feed cfm_plan_sample_dense / cfm_sinkhorn_plan_f64 / _cost_f64 unchanged.
 * x0 [B0,d], x1 [B1,d]; everything else as cfm_sinkhorn_log_f32 (same ws size and layout). */
int cfm_sinkhorn_log_points_f32(const float* x0, const float* x1, int B0, int B1, int d, double reg,
                                int max_iter, double stop_thr, int check_every, float* f, float* g,
                                int* iters_done, float* last_err, void* ws, void* stream);

/* Copy the fp64 log-scalings u [B0], v [B1] left in `ws` by the last
 * cfm_sinkhorn_log_f32 call on it. */
int cfm_sinkhorn_potentials_f64(const void* ws, int B0, int B1, double* u, double* v,
                                void* stream);

/* Dense plan  pi[i,j] = exp(u_i + v_j - M[i,j]/reg)  in fp64 from the fp64
 * log-scalings in `ws`  — what get_map() hands back to Python,
 * torchcfm/optimal_transport.py:87 (return value of pot.sinkhorn). */
int cfm_sinkhorn_plan_f64(const float* M, int B0, int B1, double reg, const void* ws,
                          double* pi, void* stream);

/* sum_ij pi_ij * M_ij — pot.sinkhorn2 value, torchcfm/optimal_transport.py:288.
 * out: one double. */
int cfm_sinkhorn_cost_f64(const float* M, int B0, int B1, double reg, const void* ws,
                          double* out, void* stream);

/* K5u — unbalanced entropic OT, uniform marginals, kernel space, fp64.
 * Replaces  pot.unbalanced.sinkhorn_knopp_unbalanced(a, b, M, reg, reg_m)
 *                                   torchcfm/optimal_transport.py:52-53,87
 * following the in-repo statement of POT's loop
 * (runner/src/models/components/sinkhorn_knopp_unbalanced.py:113-201, reg_m_1 = reg_m_2):
 *   K = exp(M / -reg);  u = (a / K v)^fi,  v = (b / K^T u)^fi,  fi = reg_m / (reg_m + reg);
 *   numerical error (K^T u == 0, nan, inf) -> the previous (u, v) and stop;
 *   every 10th iteration err = mean of the relative sup-norm changes of u and v; stop at
 *   err <= stop_thr or after max_iter iterations (POT defaults 1000, 1e-6).
 * plan [B0,B1] fp64 receives u_i K_ij v_j (what get_map() returns, :87).
 * info (device int32[4], may be NULL): {iterations, status (1 = numerical error, previous
 * iterate returned), zeros in K, non-finite entries in K}.
 * ws: cfm_workspace_bytes(CFM_OP_UNBALANCED,B0,B1,0) bytes, 16-byte aligned. */
int cfm_unbalanced_sinkhorn_f64(const float* M, int B0, int B1, double reg, double reg_m,
                                int max_iter, double stop_thr, double* plan, int* info,
                                void* ws, void* stream);

/* K5p — entropic partial OT (Dykstra), uniform marginals, transported mass m, fp64.
 * Replaces  pot.partial.entropic_partial_wasserstein(a, b, M, reg)
 *                                   torchcfm/optimal_transport.py:54-55,87
 * (m = min(sum a, sum b) = 1 when the reference calls it; POT defaults numItermax = 1000,
 * stopThr = 1e-100, error ||K_prev - K||_F every 10th iteration).  The three B0 x B1
 * Dykstra corrections are constant along rows / columns / everywhere, so the iteration is
 * carried on two scaling vectors and a scalar over K0 = exp(M / -reg) * m / sum.
 * If K0 has zeros POT's 0/0 poisons the plan with NaN; so does this (info[2] counts them).
 * plan, info, ws as for cfm_unbalanced_sinkhorn_f64. */
int cfm_partial_entropic_f64(const float* M, int B0, int B1, double reg, double m,
                             int max_iter, double stop_thr, double* plan, int* info,
                             void* ws, void* stream);

/* K4 — exact optimal assignment for uniform, equal-size marginals.
 * Replaces  pot.emd(a, b, M)                torchcfm/optimal_transport.py:49,87
 * and       scipy.optimize.linear_sum_assignment(M)                    :179.
 * M [B,B] fp32.  perm[i] = column matched to row i (int32 [B]).
 * *certified (device int) = 1 iff the fp64 dual certificate holds
 * (complementary slackness + dual feasibility to 1e-10*max|M|);
 * *total_cost (device double) = sum_i M[i,perm[i]];
 * stats (device int32[8], may be NULL): {auction_rounds, arr_rounds,
 *  free_rows_after_arr, sap_batches, sap_row_scans, total_row_scans, steps,
 *  eps_phases | multi_source_phases << 8 | dense_fallback_row_scans << 16}.
 * 2 <= B <= 256 (the reference's tutorial batches) is solved by ONE launch of ONE workgroup
 * (cost matrix in registers); stats[7] then has bit 30 set and stats[6] = 1.  A solve that hits
 * that path's round caps is redone by the chip-wide state machine; the call never returns 0
 * with an uncertified permutation (CFM_ENOCONV instead).
 * ws: cfm_workspace_bytes(CFM_OP_ASSIGN,B,B,0) bytes. */
int cfm_assign_exact_f32(const float* M, int B, int* perm, int* certified,
                         double* total_cost, int* stats, void* ws, void* stream);

/* K4, batched — nb independent assignment problems of the same size B in ONE chain of launches.
 * The reference couples one minibatch per call (torchcfm/optimal_transport.py:87, called from
 * conditional_flow_matching.py:271); the solve is a latency-bound chain (~110 dependent launches and a
 * one-workgroup list solver), so the couplings of the next nb minibatches of a training loop — they depend on
 * the data only — cost little more than one when every launch carries all of them (grid.y = problem).
 * Results are those of nb calls of cfm_assign_exact_f32 (same kernels, same state machine per problem).
 * M, perm: HOST arrays of nb device pointers ([B,B] fp32 / int32 [B]); certified [nb], total_cost [nb],
 * stats [nb][8] device arrays (each may be NULL).  nb > 16 is processed in groups of 16.
 * ws: cfm_workspace_bytes(CFM_OP_ASSIGN,B,B,nb) bytes. */
int cfm_assign_exact_batch_f32(const float* const* M, int nb, int B, int* const* perm, int* certified,
                               double* total_cost, int* stats, void* ws, void* stream);

/* K4r — exact OT between uniform marginals of DIFFERENT sizes (masses 1/B0 on the rows, 1/B1 on the columns).
 * Replaces  pot.emd(a, b, M)  for x0.shape[0] != x1.shape[0]   torchcfm/optimal_transport.py:49,79,87
 * The transportation problem on the B0 x B1 matrix itself (every row supplies B1/g units, every column takes B0/g,
 * g = gcd; no lcm x lcm expansion): the primal-dual method with one shortest-path forest into the open columns and a
 * push of ALL open supply down that forest per phase — one workgroup, node state in LDS (matrix and flows too when they
 * fit), then a chip-wide plan / certificate pass.  B0 + B1 <= 2048 (CFM_EINVAL beyond).
 * sigma (device int32[min(B0,B1)], or NULL): optional warm start — an optimal assignment of the rows of the SMALLER side
 * to distinct indices of the larger side (the square solver on the matrix padded with zero rows gives one); it is
 * validated (distinct, in range, its duals must exist) and ignored otherwise: the result never depends on it.  With
 * it, sizes that differ by one (127 vs 128: the case the lcm route cannot take) need ONE phase.
 * plan [B0,B1] fp64 (written whole: zero off the support, units / lcm on it); *total_cost = <plan, M>;
 * info (device int32[8]): {status (1 = optimal and certified in fp64: reduced costs >= -1e-10 max|M|, zero on the
 * support, marginals exact; < 0 = failed, nothing certified), phases, label-correcting sweeps, support size, violations,
 * units per row, units per column of the oriented problem, bit 0: matrix staged in LDS, bit 1: warm start used}.
 * ws: cfm_workspace_bytes(CFM_OP_TRANSPORT,B0,B1,0) bytes, 16-byte aligned.  Asynchronous on `stream`; the caller
 * reads info[0]. */
int cfm_transport_exact_f32(const float* M, int B0, int B1, const int* sigma, double* plan, double* total_cost,
                            int* info, void* ws, void* stream);

/* K6 (exact path) — draw n index pairs from the permutation plan.
 * Replaces sample_map()                      torchcfm/optimal_transport.py:116-121
 * for pi = P_perm / B:  np.random.choice over the flattened plan consumes n
 * uniforms u01 (drawn by the caller from np.random) and returns, per draw,
 * the first flat index whose cdf exceeds u:  i = floor(u*B) (cdf steps k/B),
 * j = perm[i].  u01: device double[n];  i,j: device int64[n]. */
int cfm_plan_sample_perm(const int* perm, const double* u01, int B, int n,
                         int64_t* i, int64_t* j, void* stream);

/* K6 (entropic path) — draw n index pairs from the dense Sinkhorn plan without
 * materialising it: fp64 row sums of exp(u_i+v_j-M_ij/reg), row scan, inverse
 * cdf in flattened (row-major) order, same searchsorted(side="right")
 * semantics as np.random.choice              torchcfm/optimal_transport.py:116-121.
 * ws: cfm_workspace_bytes(CFM_OP_SAMPLE_DENSE,B0,B1,0); `sk_ws` is the Sinkhorn
 * workspace holding u,v. */
int cfm_plan_sample_dense(const float* M, int B0, int B1, double reg, const void* sk_ws,
                          const double* u01, int n, int64_t* i, int64_t* j, void* ws,
                          void* stream);

/* Same draw from an explicit fp64 plan pi [B0,B1] (API path sample_map(pi,...)
 * with a caller-supplied plan; entries of `pi` may be zeroed between calls to
 * implement replace=False exactly as numpy does). */
int cfm_plan_sample_pi_f64(const double* pi, int B0, int B1, const double* u01, int n,
                           int64_t* i, int64_t* j, void* ws, void* stream);

/* K6 (trajectories) — one draw per entry of `rows` from the CONDITIONAL distribution of that plan row.
 * Replaces the inner loop of sample_trajectory()   torchcfm/optimal_transport.py:237-246
 *     for i in indices[-1]:  j.append(np.random.choice(pi.shape[1], p=pi[i] / pi[i].sum()))
 * np.random.choice consumes one uniform per call (u01[q], drawn by the caller in order) and returns the first column
 * whose running sum of the row exceeds u x (row total).  rows: device int64[n] (clamped to [0, B0)); j: device
 * int64[n].  _dense reads the entropic plan from the potentials in `sk_ws` and the cost row (never materialised;
 * ws: cfm_workspace_bytes(CFM_OP_SAMPLE_DENSE,B0,B1,0)); _pi_f64 reads an explicit fp64 plan.  The indices of a chain
 * of time slices stay on the device (the reference moves every B x B plan to the host and loops in Python). */
int cfm_plan_sample_rows_dense(const float* M, int B0, int B1, double reg, const void* sk_ws,
                               const int64_t* rows, const double* u01, int n, int64_t* j, void* ws,
                               void* stream);
int cfm_plan_sample_rows_pi_f64(const double* pi, int B0, int B1, const int64_t* rows, const double* u01,
                                int n, int64_t* j, void* stream);

/* K7+K8 — fused gather + probability-path sample + conditional flow.
 * Replaces x0[i], x1[j]                      torchcfm/optimal_transport.py:145
 * and the eager chain of                     torchcfm/conditional_flow_matching.py
 *   :82-83,126-129,153-154 (ICFM/OT), :446,474-478 (SB),
 *   :349-350,368,393-394 (Target), :588-589,617-618 (VP)
 * with the reference's operation order and no FMA contraction (bit-equal to
 * eager fp32).  i, j may be NULL (identity).  t [B], eps [B,d] (eps may be
 * NULL only when sigma terms vanish is NOT assumed: pass eps always).
 * VP: c0 = cos(pi/2 t), c1 = sin(pi/2 t) are passed in ([B] each, computed by
 * the caller's tensor library so they match its libm bit for bit); NULL for
 * the other variants, except SB where c0 (optional) = sigma_t = sigma*sqrt(t(1-t))
 * as the caller's library computes it (eager sqrt is not IEEE on every backend).
 * `sigma` is the Python-side value (double): the kernel
 * uses (float)sigma and, for TARGET, (float)(1.0 - sigma) exactly as eager
 * PyTorch casts Python scalars.  Outputs xt, ut [B,d]; x0g, x1g (may be NULL)
 * receive the gathered pairs.  xt_in (may be NULL): use this xt instead of
 * sampling one (compute_conditional_flow(x0, x1, t, xt) with a caller's xt);
 * xt may then be NULL. */
int cfm_sample_xt_ut_f32(int variant, const float* x0, const float* x1,
                         const int64_t* i, const int64_t* j, const float* t,
                         const float* eps, double sigma, const float* c0,
                         const float* c1, const float* xt_in, int B, int d, float* xt,
                         float* ut, float* x0g, float* x1g, void* stream);

/* K7+K8 (scheduled bridge) — the same fused gather + sample + flow for the Brownian bridge of dX = g(t) dW with a
 * noise schedule g(t), F(t) = int_0^t g^2.  Replaces x0[i], x1[j] and the eager chain of
 *   runner/src/models/cfm_module.py:819-827 (sigma: NoiseScheduler, OT reg 2 F(1)), :834-841 (mu_t, sigma_t), :856 (x_t),
 *   :843-850 (calc_u — here with the coefficient (d sigma_t/dt) / sigma_t, the time derivative of x_t)
 * coef [B,4] (16-byte aligned, else CFM_EALIGN), per row and evaluated by the caller's tensor library on t's device (so
 * sin, cos and sqrt match eager bit for bit):  r = F(t)/F(1),  sigma_t,  a = g^2 (1 - 2r) / (2 sigma_t^2 + 1e-8),
 * c = g^2/F(1).  Separately rounded ops, no contraction, in this order:
 *   mu = x0 + (x1 - x0) r;   xt = mu + sigma_t eps  (or xt_in);   ut = a (xt - mu) + (x1 - x0) c.
 * i, j, eps, xt_in, xt as for cfm_sample_xt_ut_f32. */
int cfm_sample_xt_ut_sched_f32(const float* x0, const float* x1, const int64_t* i,
                               const int64_t* j, const float* coef, const float* eps,
                               const float* xt_in, int B, int d, float* xt, float* ut,
                               void* stream);

/* K7+K8 (DSBM) — the scheduled bridge's x_t with the two drift targets of diffusion Schrodinger bridge matching: fused
 * gather + sample + both targets, three outputs in one launch.  Replaces x0[i], x1[j] and the eager chain of
 *   runner/src/models/cfm_module.py:834-841 (mu_t, sigma_t), :1187-1200 (x_t, forward and backward target).
 * coef [B,4] (16-byte aligned, else CFM_EALIGN), per row and evaluated by the caller's tensor library on t's device:
 *   r = F(t)/F(1),  sigma_t,  cf = g sqrt(t / (1 - t + 1e-6)),  cb = g sqrt((1 - t) / (t + 1e-6)).
 * Separately rounded ops, no contraction, in this order:
 *   dx = x1 - x0;  mu = x0 + dx r;  xt = mu + sigma_t eps;  ft = dx - cf eps;  bt = (x0 - x1) - cb eps.
 * i, j as for cfm_sample_xt_ut_f32 (NULL: identity); eps, xt, ft, bt [B,d], all required. */
int cfm_sample_dsbm_f32(const float* x0, const float* x1, const int64_t* i, const int64_t* j,
                        const float* coef, const float* eps, int B, int d, float* xt, float* ft,
                        float* bt, void* stream);

/* Row gather  out[b,:] = src[idx[b],:]  (labels y0[i], y1[j]; :215-218).
 * elem_bytes = bytes per row. */
int cfm_gather_rows(const void* src, const int64_t* idx, int n, size_t row_bytes,
                    void* out, void* stream);

/* K7t — multi-marginal flow matching on trajectories X [B,T,d]: interval select + gather + interpolant + noise +
 * leave-out rule in one launch.  Replaces the per-row loops of
 *   runner/src/models/cfm_module.py:173-193 (x0.append(tmp_ot_list[ti][0][i]) ...) and :225-242
 *   (calc_loc_and_target: mu_t, x, ut, `ut /= 2`, `t *= 2`, t + t_select)                              mode 0, linear
 *   runner/src/models/cfm_module.py:1372-1377 and the per-row torchcubicspline evaluate / derivative
 *   of :1396-1397, x = mu_t + sigma * eps :1406                                                         mode 1, spline
 * t_select [B] int64: the interval of each row (0 <= t_select <= T - 2; mode 1: the knot interval, 0 <= . <= Tp - 2);
 * t [B]: the local time in [0, 1); eps [B,d].  leaveout: the left-out slice L, 1 <= L <= T - 2, or <= 0 for none.
 * mode 0: variant CFM_VARIANT_ICFM or CFM_VARIANT_SB, in the arithmetic of cfm_sample_xt_ut_f32 (bit-equal to it on
 *   the gathered pair); sigma_t [B] = sigma * sqrt(t (1 - t)) from the caller's library (SB; else NULL).
 *   Variant CFM_VARIANT_SCHED: the arithmetic of cfm_sample_xt_ut_sched_f32; sigma_t is then its [B,4] coefficient
 *   table (16-byte aligned) at the rows' local times and sigma is not read.
 *   idx: NULL (identity) or int64 [T-1][2][B], the index pair (i, j) of every interval's coupling: row b of interval k
 *   is (X[i[b], k], X[j[b], k'])  with k' = k + 1, or k + 2 when k + 1 == L; such rows get ut / 2 and t * 2.
 *   t_net = t + t_select.  S is not read.
 * mode 1: variant CFM_VARIANT_ICFM.  The knots are the slices of X without slice L (Tp = T or T - 1 of them, at most
 *   32), at times tau = slice number.  idx: NULL or int64 [Tp][B], the row of X trajectory b visits at each knot.
 *   S [Tp][Tp] fp32: second derivatives at the knots = S @ knot values, for the natural cubic spline on tau.
 *   xt = spline(t_net) + sigma * eps, ut = spline'(t_net), t_net = tau_i + t (tau_{i+1} - tau_i).
 * Outputs xt, ut [B,d], t_net [B]. */
int cfm_traj_xt_ut_f32(int mode, int variant, const float* X, int B, int T, int d,
                       const int64_t* idx, const int64_t* t_select, const float* t,
                       const float* eps, double sigma, const float* sigma_t, int leaveout,
                       const float* S, float* xt, float* ut, float* t_net, void* stream);

/* K10 — MLP vector field  Linear-SELU x3 + Linear  with the time column folded
 * in.  Replaces MLP.forward + torch_wrapper.forward
 *   torchcfm/models/models.py:10-21, torchcfm/utils.py:51-52.
 * x [B,d]; t: device float, either one scalar (t_per_row=0) or [B]
 * (t_per_row=1), or NULL when the net is not time varying;
 * W[l] [out_l, in_l] row-major (torch.nn.Linear layout), b[l] [out_l];
 * dims[n_layers+1] (host) = {d(+1 if time varying), w, ..., out};
 * W, b: host arrays of device pointers.  out [B, dims[n_layers]].
 * ws: cfm_workspace_bytes(CFM_OP_MLP, B, max width, 0). */
int cfm_mlp_forward_f32(const float* x, const float* t, int t_per_row,
                        const float* const* W, const float* const* b,
                        const int* dims, int n_layers, int B, float* out, void* ws,
                        void* stream);

/* K10 (training) — the same network with its hidden activations kept, its backward pass and the
 * optimizer step.  Replaces what autograd and torch.optim.Adam execute for
 *   vt = net(torch.cat([xt, t[:, None]], -1)); loss.backward(); optim.step()
 *   examples/images/cifar10/train_cifar10.py:141-151, torchcfm/models/models.py:10-21.
 * Forward: x [B, dims[0]] already holds every input column (the caller concatenated the time);
 * hidden / preact: host arrays of n_layers-1 device buffers [B, dims[l+1]] <- selu(z_l) / z_l.
 * Backward: acts / preact: host arrays of n_layers device pointers (acts[0] = x, acts[l] = hidden[l-1],
 * preact[l] = the forward's preact[l-1], preact[0] unused);
 * dout [B, dims[n_layers]]; writes dW[l] [dims[l+1], dims[l]], db[l] [dims[l+1]] and, when dx is not
 * NULL, dx [B, dims[0]].  Split-K partial sums are reduced in a fixed order (deterministic).
 * ws: cfm_workspace_bytes(CFM_OP_MLP_TRAIN, B, widest layer incl. input/output, largest dims[l]*dims[l+1]): two
 * [B, widest] gradient buffers, a pool for the split-K partials of four layers of the largest size at 32 splits, and
 * 4096 loss partials.  Nets of up to four layers are reduced by one launch at the end; a deeper net (n_layers <= 15)
 * whose partials outgrow the pool is reduced in several launches, the pool reused in between: the same bits, the same
 * workspace size, never a refusal. */
int cfm_mlp_forward_train_f32(const float* x, const float* const* W, const float* const* b,
                              const int* dims, int n_layers, int B, float* const* hidden,
                              float* const* preact, float* out, void* stream);
int cfm_mlp_backward_f32(const float* const* acts, const float* const* preact, const float* const* W,
                         const int* dims, int n_layers, int B, const float* dout, float* const* dW,
                         float* const* db, float* dx, void* ws, void* stream);
/* One regression step of the vector field on a coupled batch, everything but the optimizer update, in 13
 * launches of this library's kernels (4-layer field) and nothing in between:
 *     v = net([xt, t]);  loss = mean((v - ut)^2);  dW, db = d loss / d parameters
 * Replaces `vt = model(torch.cat([xt, t[:, None]], -1)); loss = torch.mean((vt - ut) ** 2); loss.backward()` of the
 * reference's training loops: examples/images/cifar10/train_cifar10.py:147-149,
 * examples/2D_tutorials/Flow_matching_tutorial.ipynb cell 9 (torchcfm/models/models.py:10-21 is the net).
 * xt [B, dims[0] - 1] and t [B] when the net is time varying (the time column is never materialised), or
 * xt [B, dims[0]] and t = NULL.  hidden / preact as in cfm_mlp_forward_train_f32; g [B, dims[n_layers]] receives
 * d loss / d v; dW[l] [dims[l+1], dims[l]], db[l]; loss: device float.  Deterministic (fixed-order reductions).
 * layer_done (HOST array of n_layers hipEvent_t, or NULL): the data-parallel form of the reference's DDP wrapper
 * (examples/images/cifar10/train_cifar10_ddp.py:92 — gradient buckets all-reduced while the backward still runs):
 * layer l's split partials are reduced right after its weight-gradient product (one small launch per layer instead of
 * one at the end; same sums in the same order, bit-equal gradients) and layer_done[l] is recorded on `stream`, so the
 * caller's communication stream can all-reduce dW[l], db[l] under the remaining layers' products.
 * ws: cfm_workspace_bytes(CFM_OP_MLP_TRAIN, B, widest layer incl. input/output, largest dims[l]*dims[l+1]), as for
 * cfm_mlp_backward_f32 (any depth up to 15 layers at any batch; with layer_done every layer reuses the pool's start). */
int cfm_mlp_regression_step_f32(const float* xt, const float* t, const float* ut,
                                const float* const* W, const float* const* b, const int* dims, int n_layers,
                                int B, float* const* hidden, float* const* preact, float* g,
                                float* const* dW, float* const* db, float* loss, void* const* layer_done,
                                void* ws, void* stream);
/* One [SF]2M training step — a flow net and a score net of EQUAL layer sizes on one coupled batch, everything but the
 * optimizer update, in the launch count of ONE cfm_mlp_regression_step_f32 (every launch serves both nets):
 *     v = flow([xt, t]);  s = score([xt, t])
 *     losses[0] = mean((v - ut)^2);  losses[1] = mean((lam[:, None] * s + eps)^2)
 *     dW, db = d (losses[0] + score_weight * losses[1]) / d parameters
 * Replaces, of the reference's [SF]2M loops (examples/2D_tutorials/SF2M_tutorial.ipynb cell 3,
 * examples/single_cell/single-cell_example.ipynb, runner/src/models/cfm_module.py:896-909 with its score_weight),
 *     vt = model(torch.cat([xt, t[:, None]], dim=-1)); st = score_model(torch.cat([xt, t[:, None]], dim=-1))
 *     flow_loss = torch.mean((vt - ut) ** 2); score_loss = torch.mean((lambda_t[:, None] * st + eps) ** 2)
 *     loss = flow_loss + score_loss; loss.backward()
 * xt, t, ut, dims, n_layers, B as in cfm_mlp_regression_step_f32 (t == NULL: the nets are not time varying); eps
 * [B, dims[n_layers]]; lam [B] (the caller's FM.compute_lambda(t): not recomputed here).  W, b, dW, db: HOST tables
 * of 2 * n_layers device pointers, the flow net's layers first, then the score net's; hidden, preact: 2 * (n_layers - 1)
 * in the same order.  g_flow, g_score [B, dims[n_layers]] receive d loss / d v and d loss / d s.  losses: two device
 * floats, flow and score, both UNweighted (score_weight scales the score net's gradient seed, 2 * score_weight / (B * N),
 * not the reported loss).  The kernel of every product is chosen per net exactly as the one-net step chooses it, so
 * the flow net's gradients are the bits of cfm_mlp_regression_step_f32 on ut, and the score net's, with lam = 1 and
 * score_weight = 1, its bits on -eps.  Deterministic.  n_layers <= 7 (the one reduction's table holds the jobs of two
 * 7-layer nets) and at most 4096 output tiles of 64 x 64 in the last layer; beyond either: CFM_EINVAL.
 * ws: TWO workspaces of cfm_workspace_bytes(CFM_OP_MLP_TRAIN, B, widest layer, largest dims[l]*dims[l+1]) bytes back to
 * back (the second starts at that byte count, a multiple of 256); nets deeper than four layers reuse each pool as
 * cfm_mlp_backward_f32 does, the two loss reductions staying in the last launch. */
int cfm_mlp_sf2m_step_f32(const float* xt, const float* t, const float* ut, const float* eps, const float* lam,
                          const float* const* W, const float* const* b, float* const* hidden, float* const* preact,
                          float* const* dW, float* const* db, const int* dims, int n_layers, int B,
                          float* g_flow, float* g_score, float* losses, float score_weight, void* ws, void* stream);
/* One DSBM training step — a forward and a backward drift net of EQUAL layer sizes on one bridge batch, everything but
 * the optimizer update, in the launch count of ONE cfm_mlp_regression_step_f32 (the two-net driver of
 * cfm_mlp_sf2m_step_f32 with a row-weighted loss epilogue on both nets):
 *     f = fwd([xt, t]);  b = bwd([xt, t])
 *     losses[0] = mean(wf[:, None] * (f - ft)^2);  losses[1] = mean(wb[:, None] * (b - bt)^2)
 *     dW, db = d (losses[0] + losses[1]) / d parameters
 * Replaces runner/src/models/cfm_module.py:1203-1227 (DSBMLitModule.step: both nets on [xt, t], the two row-scaled
 * MSEs, their sum's backward).  The reference's "Loss Not Finite" check needs a host read of the loss: the caller's.
 * xt, t, dims, n_layers, B as in cfm_mlp_regression_step_f32; ft, bt [B, dims[n_layers]]; wf, wb [B] (the matcher's
 * forward_scaling, backward_scaling).  W, b, dW, db, hidden, preact: HOST tables as in cfm_mlp_sf2m_step_f32, the
 * forward net's layers first.  g_fwd, g_bwd receive d loss / d f, d loss / d b: ((f - ft) * 2 / (B N)) * wf.  With
 * wf = wb = 1 each net's loss and gradients are the bits of cfm_mlp_regression_step_f32 on its own target.
 * Deterministic.  Limits and ws as for cfm_mlp_sf2m_step_f32. */
int cfm_mlp_dsbm_step_f32(const float* xt, const float* t, const float* ft, const float* bt, const float* wf,
                          const float* wb, const float* const* W, const float* const* b, float* const* hidden,
                          float* const* preact, float* const* dW, float* const* db, const int* dims, int n_layers,
                          int B, float* g_fwd, float* g_bwd, float* losses, void* ws, void* stream);
/* One torch.optim.Adam step (amsgrad=False, maximize=False) on n_tensors fp32 tensors in ONE launch.
 * table: DEVICE array of n_tensors records {float* param; const float* grad; float* exp_avg;
 * float* exp_avg_sq; uint64 numel} (40 bytes each).  step >= 1 is the step count AFTER this update
 * (bias corrections 1 - beta^step are formed in double on the host, as torch does).
 * grad_scale (> 0): 1.0, or 1 / world size for a data-parallel run whose gradient buffers hold the all-reduced SUM:
 * the gradient is multiplied first (one fp32 rounding, what `grad.mul_(1 / world)` does) and written back, so .grad
 * holds the mean afterwards as under DDP (train_cifar10_ddp.py:92) — no separate elementwise launch. */
int cfm_adam_step_f32(const void* table, int n_tensors, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int step, double grad_scale, void* stream);

/* SF2M sampling — one Euler-Maruyama step  y <- y + dt (v + score_sign * s) + g sqrt(|dt|) xi,  in place.
 * Replaces the step torchsde.sdeint(sde, x0, ts, method="euler") takes for the reference's SDE
 * (f = drift + score, g = sigma): runner/src/models/components/solver.py:129-139,157-182 at sde_solver: euler.
 * (The notebooks run torchsde's default method "srk": cfm_sde_srk_step_f32 / cfm_sde_srk_mlp_f32.)  s and xi may be
 * NULL. */
int cfm_sde_em_step_f32(float* y, const float* v, const float* s, const float* xi, double dt, double g,
                        double score_sign, size_t n, void* stream);
/* SF2M sampling — the WHOLE Euler-Maruyama trajectory of a batch in one launch, for two small MLP fields (flow v and
 * score s: 4 layers, widths <= 64, time column last; Ws = bs = NULL: no score):
 *     y <- y + h (+-v(te, y) + s(te, y)) + g sqrt|h| xi        (reverse: -v, fields evaluated at te = 1 - t)
 * Replaces torchsde.sdeint(SDE(model, score_model, ...), x0, ts, method="euler", dt=...):
 * runner/src/models/components/solver.py:129-139,157-182 at sde_solver: euler.  steps_host: n_steps records {float te, h, g_sqrt_h;
 * int is_out} on the HOST (copied into ws: >= 16 n_steps bytes of device scratch); out [n_out, B, d] receives the
 * state after every step with is_out != 0.  xi: caller's N(0,1) noise [n_steps, B, d] (then the trajectory is
 * bit-equal to stepping with cfm_mlp_forward_f32 + cfm_sde_em_step_f32), or NULL: Philox4x32-10 noise from `seed`
 * in the kernel.  CFM_EINVAL for other field shapes (step launch by launch instead).
 * flags: bit 0 = reverse (as above), bit 1 = logqp, any higher bit: CFM_EINVAL before any work.  With bit 1 clear every
 * byte read and written is as described above.  logqp (torchsde's sdeint(..., logqp=True) with prior drift h = 0) also
 * integrates 1/2 sum_j (f_j / g)^2 with the same Euler steps, f being the drift of the state update:
 *   steps_host: the n_steps records followed by n_steps floats qw_k = h_k / (2 g_k^2) (the host divides, in double, and
 *               rounds once; g_k = 0 is the caller's to refuse);  ws: >= (16 + 4) n_steps bytes;
 *   out:        the trajectory [n_out, B, d] followed by logratio [n_out, B], n_out the records with is_out != 0:
 *               logratio[o][b] is the INCREASE over the steps since trajectory point o - 1 (since y0 for o = 0), not a
 *               running sum.  The trajectory is bit-equal to the one without the bit.
 * The stream of xi == NULL (pinned by tests/test_philox_host.py and tests/test_gpu_sde_philox.py against the host
 * restatement tests/philox_ref.py; it is not torchsde's stream):
 *   block:    Philox4x32-10 (Salmon et al., SC'11) on counter {elem lo, elem hi, step, stream} under key {seed lo,
 *             seed hi}; step = k, the index of the record in steps_host (the refined grid, non-output steps included);
 *             stream = 0x5f2d.  A step with g_sqrt_h == 0 draws nothing.
 *   uniforms: the top 24 bits of each word: u0 = ((c0 >> 8) + 1) / 2^24, u1 = (c1 >> 8) / 2^24, u2, u3 likewise from c2, c3;
 *   normals:  Box-Muller in float32: r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2),
 *             z = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3, r1 sin 2 pi u3);  |z| <= sqrt(48 ln 2).
 *   elements: batch row `row`, state column `col` takes z[row % 4] of the block at
 *             elem = 256 (row / 16) + 64 (col / 16) + 16 ((row % 16) / 4) + col % 16
 *             (256 lanes per 16-row tile: the lane that holds the element in the kernel).
 * So a row's noise depends on its position in the batch, the step and the seed — not on B, d, the flags or the number of
 * fields: the first rows of a larger batch reproduce a smaller one bit for bit. */
int cfm_sde_em_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Ws,
                       const float* const* bs, const int* dims, int n_layers, const float* y0, int B,
                       const void* steps_host, int n_steps, int flags, const float* xi,
                       unsigned long long seed, float* out, void* ws, void* stream);
/* SF2M sampling — one stage of an `srk` step: Roessler's SRI2W1 (strong order 1.5) for CONSTANT diagonal noise
 * g = sigma, the scheme torchsde.sdeint runs when no method is given (noise_type "diagonal", sde_type "ito").
 * Replaces the steps of the default-method calls torchsde.sdeint(sde, x0, ts=...) in
 * examples/2D_tutorials/SF2M_tutorial.ipynb cell 5 (its solver="euler" is an ignored keyword),
 * examples/single_cell/single-cell_example.ipynb, examples/images/mnist_example.ipynb and
 * examples/images/conditional_mnist.ipynb, and runner/src/models/components/solver.py:169-179 at sde_solver: srk.
 *   f_i = v_i + score_sign * s_i  (s_i may be NULL), gs = g sqrt|h|, xi1, xi2 ~ N(0, 1) (NULL: no noise)
 *   stage 1: ys = y + h f1
 *   stage 2: ys = y + (h/4)(f1 + f2) + 0.75 gs (xi1 + xi2 / sqrt(3))
 *   stage 3: y <- y + (h/6)(f1 + f2 + 4 f3) + gs xi1                    (in place; ys unused)
 * f1 = field at (t, y), f2 at (t + h, ys of stage 1), f3 at (t + h/2, ys of stage 2).  Arguments a stage does not
 * read may be NULL; ys must not alias y.  CFM_EINVAL for another stage or a missing operand. */
int cfm_sde_srk_step_f32(int stage, float* y, float* ys, const float* v1, const float* s1, const float* v2,
                         const float* s2, const float* v3, const float* s3, const float* xi1, const float* xi2,
                         double h, double g, double score_sign, size_t n, void* stream);
/* SF2M sampling — the WHOLE `srk` trajectory of a batch in one launch, for the small field pairs of
 * cfm_sde_em_mlp_f32 (same arguments and return codes).  Replaces the same default-method torchsde.sdeint calls and
 * runner/src/models/components/solver.py:169-179 as cfm_sde_srk_step_f32.  steps_host: n_steps records {float te1,
 * te2, te3 (field times of the stages at t, t + h, t + h/2; reverse: 1 - them), h, g sqrt|h|, 0.75 g sqrt|h|; int
 * is_out, pad} on the HOST (copied into ws: >= 32 n_steps bytes of device scratch).  xi: caller's N(0,1) noise
 * [n_steps, 2, B, d] (plane 0: xi1, plane 1: xi2; then the trajectory is bit-equal to stepping with
 * cfm_mlp_forward_f32 + cfm_sde_srk_step_f32), or NULL: two Philox4x32-10 streams from `seed` in the kernel.
 * flags: bit 0 = reverse, bit 1 = logqp, any higher bit: CFM_EINVAL, as for cfm_sde_em_mlp_f32.  logqp integrates
 * 1/2 sum_j (f_j / g)^2 as one more drift-only component of the scheme: per step (h/6)((q1 + q2) + 4 q3) with
 * q_i = 1/2 sum_j (k_i,j / g)^2 on the three stage drifts.  steps_host: the n_steps records followed by n_steps floats
 * qw_k = h / (12 g^2); ws: >= (32 + 4) n_steps bytes; out: the trajectory [n_out, B, d] followed by logratio [n_out, B],
 * per-interval increases as for cfm_sde_em_mlp_f32.  With bit 1 clear nothing differs from the description above.
 * The streams of xi == NULL are cfm_sde_em_mlp_f32's (same key, counter, uniforms, Box-Muller and element map, step =
 * the record's index): xi1 at stream word 0x5f2d — the very normals the Euler-Maruyama entry draws from that seed —
 * and xi2 at stream word 0x5f2e on the same counters.  A row's noise depends on its position, the step and the seed,
 * not on B. */
int cfm_sde_srk_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Ws,
                        const float* const* bs, const int* dims, int n_layers, const float* y0, int B,
                        const void* steps_host, int n_steps, int flags, const float* xi,
                        unsigned long long seed, float* out, void* ws, void* stream);
/* Mixture-RBF kernel sum  out[0] += sum_e sum_q exp(-gammas[q] * D[e])  over a squared-distance matrix D
 * (n elements, device fp32; gammas device fp32[n_gamma]; out device double, zeroed by the caller).
 * Replaces the K_XX / K_XY / K_YY matrices of mix_rbf_mmd2: runner/src/models/components/mmd.py:43-63,80-110. */
int cfm_rbf_mix_sum_f32(const float* D, size_t n, const float* gammas, int n_gamma, double* out, void* stream);

/* K11 — ODE solve of dx/dt = MLP([x, t]) on a time grid (torchdyn-style).
 * Replaces NeuralODE(torch_wrapper(model), solver=...).trajectory(x, t_span)
 *   call sites: examples/2D_tutorials/Flow_matching_tutorial.ipynb cells 11/16,
 *   examples/images/cifar10/utils_cifar.py:63-68.
 * t_span: host float[n_t], strictly monotone (a decreasing grid integrates -f(-s, x) on s = -t_span, as
 * torchdyn does: runner/src/models/components/solver.py:184-216).  traj: device [n_t,B,d].
 * euler: fixed steps on t_span.  dopri5: adaptive Dormand-Prince 5(4), one
 * global RMS error norm over the batch, every t_span point is a step end.
 * n_steps/nfe: host ints (accepted+rejected steps, function evaluations). */
int cfm_ode_euler_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                          int n_layers, const float* x0, int B, const float* t_span,
                          int n_t, float* traj, int* nfe, void* ws, void* stream);
int cfm_ode_dopri5_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                           int n_layers, const float* x0, int B, const float* t_span,
                           int n_t, float atol, float rtol, float* traj, int* n_steps,
                           int* nfe, void* ws, void* stream);

/* The solver set of torchdyn's odeint behind one selector each.  Replaces NeuralODE(..., solver="tsit5") — torchdyn's
 * default, and what the runner switches to for every adaptive test-time rollout (runner/src/models/cfm_module.py:313 and
 * :1055 via FlowSolver.ode_solver) — and torchdyn's fixed-step set "euler" / "midpoint" / "rk4" (torchdyn odeint;
 * rk4 = the 3/8 rule, "torchdyn-style", unpinned).  tableau: an adaptive 5(4) FSAL pair stepped by the dopri5 driver
 * above (same controller, order 5); scheme: explicit fixed steps on t_span, nfe = stages * (n_t - 1).
 * CFM_EINVAL for an unknown selector.  Everything else as cfm_ode_dopri5_mlp_f32 / cfm_ode_euler_mlp_f32, which are
 * these entries at CFM_ODE_DOPRI5 / CFM_ODE_EULER. */
enum { CFM_ODE_DOPRI5 = 0, CFM_ODE_TSIT5 = 1 };                          /* tableau */
enum { CFM_ODE_EULER = 0, CFM_ODE_MIDPOINT = 1, CFM_ODE_RK4 = 2 };       /* scheme */
int cfm_ode_adaptive_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                             int n_layers, const float* x0, int B, const float* t_span,
                             int n_t, int tableau, float atol, float rtol, float* traj, int* n_steps,
                             int* nfe, void* ws, void* stream);
int cfm_ode_fixed_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                          int n_layers, const float* x0, int B, const float* t_span,
                          int n_t, int scheme, float* traj, int* nfe, void* ws, void* stream);
/* DSBM sampling — the probability-flow ODE of a forward and a backward drift net of EQUAL layer sizes,
 *     dx/dt = (f(t, x) - b(t, x)) / 2,
 * on the fixed-step schemes.  Replaces NeuralODE(forward_ode_drift).trajectory of the reference's DSBMFlowSolver:
 * runner/src/models/components/solver.py:259-263.  Every stage derivative is k = 0.5f * (f - b) (one rounded
 * subtraction, an exact halving); stages, steps, t_span (either direction) and nfe (one evaluation of the PAIR per
 * stage) as cfm_ode_fixed_mlp_f32.  4-layer nets of widths <= 64 run the whole solve in one launch with both nets'
 * weights in LDS; any other size, or with the fused small-field path disabled (cfm_ode_set_fused(0)), the layer
 * driver steps it (two forward passes, the halved difference and the stage combine per stage) — the same bits.
 * ws: cfm_workspace_bytes(CFM_OP_ODE, B, max hidden width, d). */
int cfm_ode_fixed_pair_mlp_f32(const float* const* Wf, const float* const* bf, const float* const* Wb,
                               const float* const* bb, const int* dims, int n_layers, const float* x0, int B,
                               const float* t_span, int n_t, int scheme, float* traj, int* nfe, void* ws,
                               void* stream);

/* K12 — continuous normalising flow of an MLP field v = MLP([x, t]) (4 linear layers, widths <= 64, dims[0] = d + 1).
 * mode 0: div = tr(dv/dx) (exact); mode 1: div = eps^T (dv/dx) eps (Hutchinson; eps device [B,d], fixed for a solve).
 * Replaces CNF + autograd_trace of examples/2D_tutorials/model-comparison-plotting.ipynb cells 2, 4 and 7, and
 * cnf_wrapper (exact / hutch_*) of examples/2D_tutorials/Maximum_likelihood_CNF_tutorial.ipynb cells 3 and 4.
 * Return CFM_EINVAL outside that envelope or with the fused small-field path disabled (cfm_ode_set_fused(0)).
 * One evaluation: x, v device [B,d], div device [B]; ws may be NULL. */
int cfm_mlp_divergence_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                           const float* x, int B, float t, int mode, const float* eps,
                           float* v, float* div, void* ws, void* stream);
/* Augmented solves of d[l, x]/dt = [-div, v]: x0 device [B,1+d], traj device [n_t,B,1+d], column 0 = l.
 * t_span: host float[n_t], strictly monotone either way.  ws: cfm_workspace_bytes(CFM_OP_ODE, B, max width, d + 1).
 * dopri5: the error and init-step norms run over all B (1 + d) elements. */
int cfm_ode_euler_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                              const float* x0, int B, const float* t_span, int n_t, int mode,
                              const float* eps, float* traj, int* nfe, void* ws, void* stream);
int cfm_ode_dopri5_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                               const float* x0, int B, const float* t_span, int n_t, int mode,
                               const float* eps, float atol, float rtol, float* traj, int* n_steps,
                               int* nfe, void* ws, void* stream);

/* The augmented solves with the solver selectors of cfm_ode_adaptive_mlp_f32 / cfm_ode_fixed_mlp_f32 (log-likelihood
 * under torchdyn's default "tsit5", runner/src/models/cfm_module.py:313, or a fixed-step torchdyn odeint scheme);
 * cfm_ode_dopri5_cnf_mlp_f32 / cfm_ode_euler_cnf_mlp_f32 are these at CFM_ODE_DOPRI5 / CFM_ODE_EULER. */
int cfm_ode_adaptive_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                 const float* x0, int B, const float* t_span, int n_t, int mode,
                                 const float* eps, int tableau, float atol, float rtol, float* traj, int* n_steps,
                                 int* nfe, void* ws, void* stream);
int cfm_ode_fixed_cnf_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                              const float* x0, int B, const float* t_span, int n_t, int mode,
                              const float* eps, int scheme, float* traj, int* nfe, void* ws, void* stream);

/* Gradient of the Euler augmented solve that cfm_ode_fixed_cnf_mlp_f32(..., CFM_ODE_EULER) wrote into traj: the
 * backward half of the training loop of examples/2D_tutorials/Maximum_likelihood_CNF_tutorial.ipynb cell 5
 * (NeuralODE(cnf_wrapper(model, "exact"), solver="euler", sensitivity="adjoint") ... loss.backward()).
 * Discretise-then-optimise: the exact gradient of the recurrence y += h v, l -= h div that the forward ran (torchdyn's
 * "adjoint" integrates the continuous adjoint with the same solver and differs from it by O(h)).
 * traj: device [n_t,B,1+d] (the states y_n are read as checkpoints); t_span: host float[n_t], as given to the forward;
 * mode / eps: as given to the forward; g_final: device [B,1+d] = dL/d[l_N, y_N].  Outputs (overwritten): dW[l], db[l]
 * device, laid out as W[l], b[l]; g_initial device [B,1+d] = dL/d[l_0, y_0], or NULL.
 * ws: cfm_workspace_bytes(CFM_OP_CNF_GRAD, B, n_t, 0).  Same envelope and CFM_EINVAL rule as cfm_mlp_divergence_f32.
 * The result is the same bit pattern run to run (per-workgroup partials, added in a fixed order by a second launch). */
int cfm_cnf_euler_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                           const float* traj, int B, const float* t_span, int n_t, int mode,
                           const float* eps, const float* g_final, float* const* dW, float* const* db,
                           float* g_initial, void* ws, void* stream);

/* trace modes of the regularised solve (modes 0 and 1 are the `mode` of cfm_mlp_divergence_f32) and its reg_mask bits */
#define CFM_TRACE_EXACT      0   /* l -= h tr(dv/dx), d exact directions */
#define CFM_TRACE_HUTCH      1   /* l -= h eps^T (dv/dx) eps, one probe per row, fixed for the solve */
#define CFM_TRACE_NONE       2   /* AugmentationModule(cnf_estimator=None): no l column, no divergence; eps is ignored */
#define CFM_REG_SQUARED_L2          1   /* SquaredL2Reg         (augmentation.py:31-34): |v|^2 */
#define CFM_REG_JACOBIAN_FROBENIUS  2   /* JacobianFrobeniusReg (:64-73): ||dv/dx||_F / d */
#define CFM_REG_L1                  4   /* L1Reg                (:21-23): (sum_j |v_j|) / d */
#define CFM_REG_L2                  8   /* L2Reg                (:26-28, :10-12): sqrt(sum_j v_j^2) / sqrt(d) */

/* The Euler solve of the state that AugmentationModule builds (runner/src/models/components/augmentation.py:137-210)
 * under AugmentedVectorField (:266-303), and its gradient.  With a trace it is regularised CNF training (RNODE /
 * TrajectoryNet): what CNFLitModule.step (runner/src/models/cfm_module.py:1412-1454) integrates and differentiates.
 * Without one (CFM_TRACE_NONE) it is the sampler with path diagnostics: FlowSolver.odeint under val_augmentations
 * (runner/src/models/components/solver.py:201-216, cfm_module.py:441-505).
 * mode: CFM_TRACE_*; reg_mask: CFM_REG_* bits, 1 <= reg_mask <= 15 (mask 0 with a trace is cfm_ode_fixed_cnf_mlp_f32 /
 * cfm_cnf_euler_grad_f32, without one cfm_ode_fixed_mlp_f32).  State rows [(l), (L1), (L2), (e), (f), x] in the
 * reference's order (:158-177), which is not bit order; D = (mode != 2) + popcount(reg_mask) + d.  Per step y += h v,
 * l -= h div, L1 += h (sum_j |v_j|) / d, L2 += h |v| / sqrt(d), e += h |v|^2, f += h ||J||_F / d, everything at (y_n, t_n).
 * Columns l and x are the bit patterns of cfm_ode_fixed_cnf_mlp_f32 at CFM_ODE_EULER (CFM_TRACE_NONE: x those of
 * cfm_ode_fixed_mlp_f32 at CFM_ODE_EULER), and l, e, f, x do not depend on bits 2 and 3.  eps as cfm_mlp_divergence_f32
 * (read with CFM_TRACE_HUTCH only).  CFM_REG_JACOBIAN_FROBENIUS needs CFM_TRACE_EXACT (the Jacobian's columns are the
 * exact trace's directions) and jac_sq: CFM_EINVAL otherwise, and for a mode outside 0..2 or a mask outside 1..15.
 * Forward: x0 device [B,D], traj device [n_t,B,D]; jac_sq device [n_t-1,B], written with bit 1 (||J||_F^2 per step and row,
 * which the gradient reads back), NULL allowed without it; t_span host float[n_t], strictly monotone either way;
 * ws: cfm_workspace_bytes(CFM_OP_ODE, B, max width, D), CFM_EINVAL when n_t > 3 B D.
 * Same envelope and CFM_EINVAL rule as cfm_mlp_divergence_f32. */
int cfm_ode_euler_cnf_reg_mlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                  const float* x0, int B, const float* t_span, int n_t, int mode,
                                  const float* eps, int reg_mask, float* traj, float* jac_sq, int* nfe, void* ws,
                                  void* stream);
/* Its gradient, discretise-then-optimise as cfm_cnf_euler_grad_f32: replaces loss.backward() through the augmented solve
 * of cfm_module.py:1443, which in autograd differentiates JacobianFrobeniusReg's d rows of
 * autograd.grad(..., create_graph=True) (augmentation.py:37-61) a second time.  traj, t_span, mode, eps, reg_mask, jac_sq:
 * as given to / written by the forward; g_final device [B,D] = dL/d(final state); outputs as cfm_cnf_euler_grad_f32, with
 * g_initial device [B,D] or NULL (the augmented columns pass through: each enters the recurrence linearly).  Where
 * ||J||_F = 0 its term has gradient 0, as torch.norm's backward has it; so has L2's where |v| = 0, and L1's where
 * v_j = 0 (torch.abs's backward: sign(0) = 0).  mode: CFM_TRACE_EXACT or CFM_TRACE_HUTCH; CFM_TRACE_NONE is CFM_EINVAL
 * (no training loop differentiates the sampler's diagnostics).
 * ws: cfm_workspace_bytes(CFM_OP_CNF_GRAD, B, n_t, 0).  The result is the same bit pattern run to run. */
int cfm_cnf_reg_euler_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                               const float* traj, int B, const float* t_span, int n_t, int mode,
                               const float* eps, int reg_mask, const float* jac_sq, const float* g_final,
                               float* const* dW, float* const* db, float* g_initial, void* ws, void* stream);

/* Gradient of the plain fixed-step solve that cfm_ode_fixed_mlp_f32(..., scheme) wrote into traj: what
 * sensitivity="adjoint" asks of NeuralODE(model, solver="euler", sensitivity="adjoint")
 * (examples/images/cifar10/utils_cifar.py:63; runner/src/models/cfm_module.py:290) when a loss is put on node(x, t_span).
 * Discretise-then-optimise, as cfm_cnf_euler_grad_f32: the exact gradient of the Runge-Kutta recurrence the forward ran,
 * for CFM_ODE_EULER, CFM_ODE_MIDPOINT and CFM_ODE_RK4.
 * traj: device [n_t,B,d], the forward's (the states y_n are read as checkpoints, the stages are recomputed from them);
 * t_span: host float[n_t], as given to the forward; g_traj: device [n_t,B,d] = dL/d traj, every slice (a loss on traj[-1]
 * alone has zeros elsewhere).  Outputs (overwritten): dW[l], db[l] device, laid out as W[l], b[l]; g_initial device
 * [B,d] = dL/d x0, or NULL.  n_t == 1: zero parameter gradients, g_initial = g_traj[0].
 * ws: cfm_workspace_bytes(CFM_OP_ODE_GRAD, B, n_t, 0).  Envelope: 4 layers, 1 <= every width <= 64, 1 <= d, d + 1 <= 64,
 * the fused small-field path on (cfm_ode_set_fused); CFM_EINVAL otherwise, there is no layer-per-kernel form.
 * The result is the same bit pattern run to run (per-workgroup partials, added in a fixed order by a second launch). */
int cfm_ode_fixed_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                           const float* traj, int B, const float* t_span, int n_t, int scheme,
                           const float* g_traj, float* const* dW, float* const* db, float* g_initial, void* ws,
                           void* stream);
/* Whether cfm_ode_fixed_grad_f32 takes a field of these dims (host int[n_layers + 1]): 0, or CFM_EINVAL.  No GPU work: a
 * caller that differentiates through the solve (utils_cifar.py:63) asks before the forward, since a backward pass cannot
 * fall back. */
int cfm_ode_fixed_grad_available(const int* dims, int n_layers);

/* Training through the adaptive sampler: NeuralODE(model, solver="dopri5" | "tsit5", sensitivity="adjoint", atol, rtol)
 * with a loss on node(x, t_span) (examples/images/cifar10/utils_cifar.py:63-68; the reference's standard sampler call).
 * Discretise-then-optimise: the gradient of the recurrence of ACCEPTED steps the forward ran, the step sequence taken as
 * a constant; rejected attempts contribute nothing.
 * Forward, cfm_ode_adaptive_rec_mlp_f32: cfm_ode_adaptive_mlp_f32 (same arguments; traj, n_steps and nfe are its bits)
 * that also records its accepted steps.  log: device, max_steps records {float t, dt, t_k1; int out} (16 bytes): solver-space
 * (s = sign * t) start and size of the step as its stages used them, the time its first slope was evaluated at (FSAL: the
 * previous accepted step's last stage time; t_span[0] for the first), and the t_span index its end lands on or -1.
 * ysteps: device [max_steps,B,d], the state every accepted step started from (ysteps[0] = x0).  n_accepted: host int.
 * CFM_EINVAL wherever cfm_ode_adaptive_mlp_f32 would leave its one-launch kernel (a net outside the small-field envelope,
 * B d < n_t, the fused path switched off: cfm_ode_set_fused) — only that kernel records — and then before any GPU work, so
 * a caller may step the solve another way at no cost; a failure after that is a hipError_t; CFM_ENOCONV when max_steps
 * accepted steps did not reach the end of the grid (the records written so far are valid, traj is not complete). */
int cfm_ode_adaptive_rec_mlp_f32(const float* const* W, const float* const* b, const int* dims,
                                 int n_layers, const float* x0, int B, const float* t_span,
                                 int n_t, int tableau, float atol, float rtol, float* traj, int* n_steps,
                                 int* nfe, int max_steps, void* log, float* ysteps, int* n_accepted, void* ws,
                                 void* stream);
/* Its gradient.  ysteps, log, n_accepted: as the forward left them; tsign: +1 for an increasing t_span, -1 for a decreasing
 * one; g_traj: device [n_t,B,d] = dL/d traj, every slice.  Outputs (overwritten): dW[l], db[l] device, laid out as W[l],
 * b[l]; g_initial device [B,d] = dL/d x0, or NULL.  Every step's six stages are recomputed from ysteps[n] in the forward's
 * arithmetic.  ws: cfm_workspace_bytes(CFM_OP_ODE_GRAD, B, n_t, 0).  Envelope and CFM_EINVAL rule of
 * cfm_ode_fixed_grad_f32.  The result is the same bit pattern run to run. */
int cfm_ode_adaptive_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                              const float* ysteps, const void* log, int n_accepted, int B, int n_t, int tableau,
                              float tsign, const float* g_traj, float* const* dW, float* const* db, float* g_initial,
                              void* ws, void* stream);
/* Whether cfm_ode_adaptive_grad_f32 takes a field of these dims: 0, or CFM_EINVAL.  No GPU work. */
int cfm_ode_adaptive_grad_available(const int* dims, int n_layers);

/* K13 — action matching: the field v = grad_x s(x, t) of a scalar action net s = MLP([x, t]) with one output
 * (4 linear layers, dims = [d + 1, n1, n2, n3, 1], 1 <= every width <= 64, d + 1 <= 64), and the solves over it.
 * Replaces GradModel(MLP(dim, out_dim=1, time_varying=True)) (torchcfm/models/models.py:24-32) as
 * examples/2D_tutorials/model-comparison-plotting.ipynb samples it (cell 4: NeuralODE(torch_wrapper(model), "euler")
 * over 101 points) and evaluates its density (cells 4 and 7: CNF + the exact trace on 201 points backward in time).
 * W, b, dims describe the ACTION net; its last bias is never read for a value.  Every entry returns CFM_EINVAL outside
 * that envelope or with the fused small-field path disabled (cfm_ode_set_fused(0)): this field has no layer-per-kernel
 * form.
 * One evaluation: x device, B rows of d values at a row stride of ldx floats (ldx >= d); v device [B,d];
 * lap device [B] = tr(dv/dx), the Laplacian of s, or NULL (v is the same bit pattern either way); ws may be NULL. */
int cfm_mlp_grad_field_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                           const float* x, int ldx, int B, float t, float* v, float* lap, void* ws, void* stream);
/* Solves of dx/dt = grad_x s(x, t): arguments, trajectory layout, nfe / n_steps and the reverse-time rule as
 * cfm_ode_fixed_mlp_f32 / cfm_ode_adaptive_mlp_f32 (models.py:24-32 under the notebook's cell 4).  ws:
 * cfm_workspace_bytes(CFM_OP_ODE, B, max width, d); CFM_EINVAL when t_span does not fit it (fixed: n_t > 3 B d,
 * adaptive: n_t > B d). */
int cfm_ode_fixed_gradmlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                              const float* x0, int B, const float* t_span, int n_t, int scheme, float* traj,
                              int* nfe, void* ws, void* stream);
int cfm_ode_adaptive_gradmlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                 const float* x0, int B, const float* t_span, int n_t, int tableau, float atol,
                                 float rtol, float* traj, int* n_steps, int* nfe, void* ws, void* stream);
/* The augmented solve d[l, x]/dt = [-lap s, grad_x s] (models.py:24-32 under the notebook's cells 4 and 7): arguments as
 * cfm_ode_fixed_cnf_mlp_f32, ws at d + 1.  mode 0 (exact trace) only: any other mode returns CFM_EINVAL; eps is ignored. */
int cfm_ode_fixed_cnf_gradmlp_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                  const float* x0, int B, const float* t_span, int n_t, int mode,
                                  const float* eps, int scheme, float* traj, int* nfe, void* ws, void* stream);

/* The action-matching objective and its parameter gradient: ActionMatchingLitModule.step
 * (runner/src/models/cfm_module.py:670-694: a0 - a1 + 1/2 |ds/dx|^2 + ds/dt at (xt, t), mean over the batch) together with
 * the loss.backward() that follows it, which in autograd is a double backward through autograd.grad(..., create_graph=True).
 * W, b, dims: the ACTION net, in the envelope of cfm_mlp_grad_field_f32 (CFM_EINVAL outside it or with the fused
 * small-field path off), any B >= 1.  x0, x1, xt: device [B,d]; t: device [B], the time column the net sees at xt (the
 * endpoints are evaluated at t = 0 and t = 1).  xt NULL: the reference's interpolant t * x1 + (1 - t) * x0 (line 682), in
 * its fp32 operation order.  Outputs (overwritten): loss device [1]; dW[l], db[l] device, laid out as
 * W[l], b[l] = d loss / d W[l], d loss / d b[l]; db[3] is an exact 0 (the loss does not depend on b[3]).  No gradient
 * with respect to x0, x1, xt, t (they carry no graph in the reference).  ws: cfm_workspace_bytes(CFM_OP_ACTION_GRAD, B, 0, 0).
 * The result is the same bit pattern run to run (per-workgroup partials, added in a fixed order by a second launch). */
int cfm_action_matching_grad_f32(const float* const* W, const float* const* b, const int* dims, int n_layers,
                                 const float* x0, const float* x1, const float* xt, const float* t, int B,
                                 float* loss, float* const* dW, float* const* db, void* ws, void* stream);

/* K14 — input-convex networks for optimal transport (Makkuva et al. 2020): the runner's ICNN
 * (runner/src/models/components/icnn_model.py) and the minimax objective of ICNNLitModule.training_step / compute_w2
 * (runner/src/models/icnn_module.py:98-135, 229-245), whose every step is three autograd.grad(create_graph=True) graphs.
 * A net of L = num_hidden_layers, width dimh, input d:  a_1 = Wz[0] x + bz0,  h_l = softplus(a_l) (beta 1, threshold 20),
 * a_{l+1} = Wz[l] h_l + Wx[l-1] x + bx[l-1] (l = 1 .. L-1),  out = Wz[L] h_L + Wx[L-1] x.  Wz[0], Wx[0 .. L-2]: [dimh, d];
 * Wz[1 .. L-1]: [dimh, dimh]; Wz[L]: [1, dimh]; Wx[L-1]: [1, d]; bz0, bx[.]: [dimh].  Entries of the tables beyond the net's
 * L are not read.  The gradient tables mirror the weight tables.
 * Envelope: f and g of one shape, 2 <= L <= 4, 1 <= dimh <= 64, 1 <= d <= CFM_ICNN_MAX_DIM, B >= 1, reg >= 0, the fused
 * small-field path on (cfm_ode_set_fused).  Outside it, for a wrong `size`, an unknown op or a missing operand the entry
 * returns CFM_EINVAL before any HIP call.
 *   CFM_ICNN_TRANSPORT  p [B,d] = grad_x f(x): the transport map of the net in slot f.  Reads f, x.  1 launch.
 *   CFM_ICNN_W2         p = grad g(y); losses = (w2, f_loss, g_loss) of compute_w2, no penalty.  Reads f, g, x, y.  3 launches.
 *   CFM_ICNN_F_STEP     p = grad g(y); losses = (loss_f, its data term mean(f(x) - f(p)), its penalty
 *                       reg sum_{W in f.Wz} |relu(-W)|^2 / 2); f's gradient tables = d loss_f / d theta_f.  3 launches.
 *   CFM_ICNN_G_STEP     p = grad g(y); w [B,d] = grad f(p) - y; losses = (loss_g, mean(f(p) - y.p), the penalty on g.Wz);
 *                       g's gradient tables = d loss_g / d theta_g with f held constant (a double backward in autograd).
 *                       4 launches.
 * x, y: device [B,d].  Outputs are overwritten whole: p by every op, w by G_STEP, losses[3] by every op but TRANSPORT, the
 * gradient tables of the net that is trained.  ws: cfm_workspace_bytes(CFM_OP_ICNN, B, 0, 0), unused by TRANSPORT.
 * The result is the same bit pattern run to run (per-workgroup partials, added in a fixed order by the last launch).
 * The operands travel in a descriptor: the caller writes sizeof(cfm_icnn_call) into `size`.  The stream is a field of
 * it, and every convention at the top of this header holds for this entry unchanged (all work on `stream`, no allocation,
 * ws and outputs arbitrary on entry, nothing else written, a declining call writes nothing, the descriptor may be
 * freed on return).  tests/test_gpu_icnn_contract.py asserts them; the case tables of tests/stream_cases.py find their
 * entries by a `void* stream` PARAMETER, so this entry's cases are to be folded into that table by hand. */
#define CFM_OP_ICNN        13   /* cfm_icnn_f32 (B, 0, 0): per-workgroup partial gradients + loss terms */
#define CFM_ICNN_MAX_DIM   64
#define CFM_ICNN_TRANSPORT  0
#define CFM_ICNN_W2         1
#define CFM_ICNN_F_STEP     2
#define CFM_ICNN_G_STEP     3
typedef struct cfm_icnn_net {
    const float* Wz[5];
    const float* bz0;
    const float* Wx[4];
    const float* bx[3];
    float* dWz[5];
    float* dbz0;
    float* dWx[4];
    float* dbx[3];
} cfm_icnn_net;
typedef struct cfm_icnn_call {
    size_t size;
    int op;
    int d;
    int dimh;
    int L;
    int B;
    float reg;
    cfm_icnn_net f;
    cfm_icnn_net g;
    const float* x;
    const float* y;
    float* p;
    float* w;
    float* losses;
    void* ws;
    void* stream;
} cfm_icnn_call;
int cfm_icnn_f32(const cfm_icnn_call* call);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CFM_GFX950_H */

