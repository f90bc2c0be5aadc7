/*
 * cfm_gfx950_tuning.h — measurement and tuning exports of libcfm_gfx950.so.
 *
 * NOT part of the operator ABI (include/cfm_gfx950.h): no binding of the reference needs any of these, the Python
 * mirror calls them only from tools/ (sweeps, profiles) and tests.  They are the one piece of process-wide state of
 * the library: a table of solver parameters.  A solve works on a snapshot of the table taken under a mutex when it
 * starts, so a setter called from another thread never tears a running solve; the getters read back what the LAST
 * solve of the calling thread (or on the given workspace) left behind and block until it is resident.
 */
#ifndef CFM_GFX950_TUNING_H
#define CFM_GFX950_TUNING_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* exact assignment (cfm_assign_exact_f32): epsilon schedule (theta, first / last epsilon as fractions of the cost
 * range, phase cut), round caps, launches per polled chunk.  Arguments <= 0 (stop_frac, arr_cap: < 0) keep the value. */
void cfm_assign_set_params(double theta, double eps0_frac, double eps_last_frac, double stop_frac, int round_cap,
                           int arr_cap, int chunk);
void cfm_assign_set_mode(int sparse);            /* 0: no candidate-list solver (dense state machine only) */
void cfm_assign_set_handoff(int handoff);        /* free rows at which phase C moves into the list solver (<= 64) */
void cfm_assign_set_stop_early(double f);        /* phase cut of every epsilon phase but the last */
void cfm_assign_set_wide_blocks(int cap);        /* upper bound on the grid of the chip-wide step kernel (0: none) */
void cfm_assign_set_bulk(int bulk, int min_n);   /* launches enqueued before the first poll, for n >= min_n */
/* on = 2 (the DEFAULT): every bid of a solve — the epsilon > 0 phases AND the epsilon = 0 rounds — in the one-launch
 * asynchronous auction (asg_auction), the whole solve as one unpolled program of 9 launches (11 with cfm_assign_set_sweep(0)); on = 1: only the epsilon > 0
 * phases there, the epsilon = 0 rounds as synchronous launches; on = 0: every round a launch (the A/B reference; always
 * the path of n < 512 and n > 8192).  blocks >= 0: workgroups per problem of the auction in the batch entry (0: as the
 * other kernels); last_div > 0: its last phase is cut at stop_frac / last_div.  The grid is capped at the CUs the
 * stream may use (CU-masked streams); a grid that cannot hold 1/256 of the rows per workgroup falls back to on = 0. */
void cfm_assign_set_async(int on, int blocks, int last_div);
/* The plain matrix sweeps of a solve's unpolled head (row minima, initial prices, column reduction, certificate):
 * 1 = in the lean 4-wave kernel asg_sweep, which shares a CU with dense work; 0 = every chip-wide step is an asg_step
 * launch (16-wave workgroups that each need an empty CU) — the A/B reference; < 0 = the library's defaults again (chosen
 * per form of the solve, batch or lone: csrc/assign.hip).  Same results bit for bit. */
void cfm_assign_set_sweep(int mode);
void cfm_assign_set_async_min_n(int n);          /* smallest n that takes the one-launch auction (default 512; >= 64) */
void cfm_assign_get_async(int* out3);            /* {on, blocks, last_div} as set (tests restore what they changed) */
void cfm_assign_set_small(int on);               /* 0: problems of n <= 256 take the chip-wide machine too */
void cfm_set_blocking_sync(int on);              /* THIS host thread's solver waits: 1 = sleep in the driver (hipEventBlockingSync) instead of spinning on a core; cfm_amd.prefetch sets it for its worker threads */
void cfm_ode_set_fused(int on);                  /* 0: layer-per-kernel ODE stages instead of the fused small-field drivers */
void cfm_mlp_set_glds(int mode);               /* MLP layers on 64 x 64 tiles: 0 = register-staged operand loads (gemm_core.h: the plain ascending-k chain, bit-equal to the fused small-field ODE drivers), 1 = direct-to-LDS DMA (gemm_glds64.h) when the rows are 16-byte aligned, 2 (default) = for 4-byte aligned rows too */
int cfm_mlp_get_glds(void);                    /* the mode in force (tests restore what they changed) */
int cfm_ode_rec_resident_rows(int tableau);    /* rows up to which cfm_ode_adaptive_rec_mlp_f32 keeps its state in registers (16 x the workgroups of its kernel that are resident at once; above it the streamed instantiation runs); < 0: query failed.  Needs the GPU */

/* read-backs (blocking) */
int cfm_assign_debug_times(const void* ws, double* us32);          /* microseconds per mode of the last solve on ws */
int cfm_assign_debug_solver(const void* ws, int n, long long* out16);   /* -DSP_PROFILE builds: list-solver cycle counters */
int cfm_assign_debug_lists(const void* ws, int n, int b, void* cl_out, double* cT_out, double* p_out);   /* candidate lists of the last solve on ws (problem b of a batch): n x 64 {column, cost bits}, n bounds, the n prices they were built from — host buffers */
/* ONE sweep step (mode 0 UMIN0, 1 INITRED, 5 UMIN, 6 COLRED, 7 ROOTMIN, 10 CERT) on a caller-made state with the kernel
 * cfm_assign_set_sweep selects; mode -1: the launch record of this thread's last chip-wide solve.  M, ws: device; the rest
 * host.  Arguments and outputs: csrc/assign_driver.h. */
int cfm_assign_debug_sweep(int mode, const float* M, int n, int blocks, const double* p_in, const double* bidval_in,
                           const int* list, int n_list, const int* perm_in, double* bidval_out,
                           unsigned long long* key_out, double* p_out, int* state_out, double* cost_out, void* ws, void* stream);
void cfm_assign_debug_small(int* out16);                           /* status block of this thread's last one-workgroup solve */
void cfm_assign_debug_fallback(int* out2);                         /* {solves of this PROCESS (all threads) redone by the dense machine, last device error} */
/* Kernel selection of the two Sinkhorn entry points for a shape: the host arithmetic the entry points themselves use, no
 * GPU call.  cfm_sinkhorn_dispatch_info (m_aligned16: the matrix starts on a 16-byte boundary) fills out16 =
 * {vec, row_fast, v_in_lds (by size), nchunk, rows_per_chunk, rows_per_wg, row_wgs, stream_nf4, stream grid before the
 * cap at the CU count, LDS bytes of the row pass, then the byte offsets of u, v[0], v[1], pm, ps in the workspace and
 * the end of ps}.  row_fast = 1 is the streaming row pass (the one-shot fast pass under CFM_SK_STREAM=0), else the
 * generic one.  cfm_sinkhorn_points_dispatch_info fills out8 = {stage_cap, col_grid, row_grid, other points per trip and
 * lane, prologue points per thread, LDS bytes, staged chunks of x0, staged chunks of x1}. */
int cfm_sinkhorn_dispatch_info(int B0, int B1, int m_aligned16, long long* out16);
int cfm_sinkhorn_points_dispatch_info(int B0, int B1, int d, long long* out8);
int cfm_plan_zero_entries_f64(double* pi, const int64_t* flat, int n, void* stream);   /* pi.flat[flat[q]] = 0 (sample_map(replace=False) bookkeeping of the mirror) */

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CFM_GFX950_TUNING_H */
