#!/usr/bin/env python
"""bench.py — OT-CFM train-step throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

One "step" = one pass of the hot path over one synthetic minibatch already resident in HBM
(config C3: x0 ~ N(0,I) in R^784, x1 MNIST-like, B = 4096 per GPU):
    cost matrix -> exact OT assignment -> plan sampling -> fused gather + xt/ut  (HIP kernels)
    -> MLP(785-512-512-512-784) forward, MSE, backward as ONE library call (cfm_amd.RegressionStep: fp32-MFMA HIP
       kernels, no eager op), one-launch Adam (HIP)
Schedule (--pipeline N --group G, default 3 x 4): the coupling depends only on the data, so the couplings of
the next batches are computed on side streams (background threads, cfm_amd.prefetch) while the model steps on
batch k, like data-loader workers: N prefetch jobs in flight, each coupling G consecutive minibatches together —
their G assignment problems go through ONE chain of launches (cfm_assign_exact_batch_f32; same kernels and the
same per-problem state machine as G single solves, bit-equal results).  The pipeline starts empty inside the timed
region and is drained inside it: K timed steps contain exactly K couplings and K model updates.
Host RNG draws stay on the main thread, in order.  `value` is that schedule; `value_sequential` (--full)
is the same K steps strictly one after the other (what an unmodified training script gets).
N > 1: one process per GPU (torchrun), every rank couples its own minibatch (no collective in
the OT path), the model is data parallel (gradient all-reduce over RCCL), and the final x_t of the
timed region is all-gathered once (the north star's "all-gather of the final samples"), inside
the timed region; weak scaling.  Rank 0 prints ONE JSON line.

A plain run sets up, runs W warm-up steps, times ONE region of exactly K steps, writes the arrays of the last timed
step if --dump-outputs is given (DIR/<name>.npy: t, xt, ut of the coupling; loss, parameters and gradients of the
model step) and prints the line: `value` = N x B x K / time of the region, `ms_per_step` = that time / K.  Everything
else below runs with --full only.

With --full, `value` is the median of --repeats such regions (51 by default, fewer for long regions: at most
20 000 timed steps in all; the counts follow from K alone), the dump is taken after the last of them,
and the line also carries (rank 0, N = 1): `value_sequential`, `steady_state`, `roofline` of the coupling's dominant
kernel family (the exact solver's chip-wide kernels asg_auction + asg_step, per solve from an un-overlapped leg, and
for the batch-of-4 form the schedule runs),
`value_public_api` (the sequential and the pipelined loop through FM.sample_location_and_conditional_flow[_group],
asserted bit-equal to the composition timed above), `c2` / `c5` (BASELINE configs[1] / configs[4]: Sinkhorn
iterations/s as the median of 7 windows with the solver's state after each, and, for C5, the dopri5 sampling time),
`c1` (exact-OT latency at B = 256 next to its CPU figure), `aux`, `parity` and `cpu_baseline`.
"""
import argparse
import collections
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this driver (RCCL across processes needs it)

import numpy as np  # noqa: E402
import torch  # noqa: E402

def thread_cpu_seconds():
    """CPU seconds (user + system) of every thread of this process, by thread name: which threads the host side of a rank
    keeps busy (the loop, the prefetch workers, the HIP runtime's own)."""
    out = {}
    try:
        tick = os.sysconf("SC_CLK_TCK")
        for tid in os.listdir("/proc/self/task"):
            try:
                comm = open(f"/proc/self/task/{tid}/comm").read().strip()
                f = open(f"/proc/self/task/{tid}/stat").read().rsplit(")", 1)[1].split()
                out[f"{comm}:{tid}"] = (int(f[11]) + int(f[12])) / tick
            except OSError:
                pass
    except Exception:  # noqa: BLE001
        pass
    return out


def newest_profile(name):
    """profiles/rNN_<name> of the latest round that has one (the committed rocprofv3 summaries bench.py quotes)."""
    import glob
    import re
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", "r*_" + name)):
        m = re.match(r"r(\d+)_", os.path.basename(f))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), f)
    return best[1] if best else None


HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec (MI355X_MICROARCH.md)
F32_PEAK_TFLOPS = 157.3   # fp32 vector = fp32-input MFMA peak


def synth_batches(B, d, n, seed, dev):
    """Pool of n synthetic (x0, x1) minibatches in HBM (C3 shapes)."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.rand(10, d, generator=g) * 2 - 1
    out = []
    for _ in range(n):
        x0 = torch.randn(B, d, generator=g)
        k = torch.randint(0, 10, (B,), generator=g)
        x1 = torch.clamp(0.35 * torch.randn(B, d, generator=g) + mu[k], -1, 1)
        out.append((x0.to(dev), x1.to(dev)))
    return out


# --------------------------------------------------------------------------- the timed loop
def job_sizes(count, group, ramp=(), tail=()):
    """Sizes of the prefetch jobs that cover `count` steps: `ramp` first, `tail` last (dropped from its front when the
    steps do not suffice), `group` in between (the job before the tail takes what is left)."""
    sizes, left = [], count
    for k in ramp:
        if left <= 0:
            break
        sizes.append(min(k, left)); left -= sizes[-1]
    tail = list(tail)
    while tail and sum(tail) > left:
        tail.pop(0)
    mid = left - sum(tail)
    while mid > 0:
        sizes.append(min(group, mid)); mid -= sizes[-1]
    return sizes + tail


def run_steps(pool, first, count, couple, model_step, draw, prefetcher=None, depth=0, group=1, couple_group=None, ramp=(),
              tail=()):
    """`count` steps starting at pool index `first`: every step = one coupling + one model update,
    all of them inside this call (a prefetch pipeline starts empty and is drained).  Returns the
    last (t, xt, ut).  Device agnostic: `couple(x0, x1, drawn)` and `model_step(t, xt, ut)` are the
    caller's; the CPU multi-process test drives this with CPU stand-ins.
    group > 1: the couplings of `group` consecutive minibatches are one prefetch job
    (`couple_group(batches, drawn_list)` -> one result per minibatch), `depth` such jobs in flight.
    ramp: group sizes of the FIRST jobs (then `group`): the pipeline starts empty inside the timed call, and the first
    model step cannot start before the first job is back — a small first job shortens that fill.
    tail: group sizes of the LAST jobs: the pipeline is drained inside the call too, and while the last job's chain of
    launches runs nothing is left to overlap with it — small last jobs shorten that drain."""
    last = None
    if not depth or prefetcher is None:
        for k in range(count):
            x0, x1 = pool[(first + k) % len(pool)]
            last = couple(x0, x1, draw())
            model_step(*last)
        return last
    inflight, submitted = collections.deque(), 0
    if group > 1 and couple_group is not None:
        njobs, plan = 0, job_sizes(count, group, ramp, tail)

        def submit_next():
            nonlocal submitted, njobs
            k = plan[njobs]
            njobs += 1
            batches = [pool[(first + submitted + q) % len(pool)] for q in range(k)]
            inflight.append(prefetcher.submit_group(batches, couple_group, draw)); submitted += k
        while submitted < count and len(inflight) < depth:
            submit_next()
        while inflight:
            outs = inflight.popleft().result()
            if submitted < count:
                submit_next()
            for last in outs:
                model_step(*last)
        return last
    while submitted < min(depth, count):
        inflight.append(prefetcher.submit(*pool[(first + submitted) % len(pool)], hook=couple, draw=draw)); submitted += 1
    for k in range(count):
        last = inflight.popleft().result()
        if submitted < count:
            inflight.append(prefetcher.submit(*pool[(first + submitted) % len(pool)], hook=couple, draw=draw)); submitted += 1
        model_step(*last)
    return last


def timed_region(D, sync, pool, warmup, steps, couple, model_step, draw, prefetcher, depth, device=None, group=1,
                 couple_group=None, ramp=(), tail=(), keep=None):
    """Warm-up, barrier + sync, K steps + ONE all-gather of the final samples, sync + barrier; the
    MAX over ranks of the elapsed time.  Returns (elapsed_s, gathered_final_xt).  keep: a dict that receives the last
    step's (t, xt, ut) as "last"."""
    run_steps(pool, 0, warmup, couple, model_step, draw, prefetcher, depth, group, couple_group, ramp, tail)
    D.barrier(); sync()
    t0 = time.perf_counter()
    last = run_steps(pool, warmup, steps, couple, model_step, draw, prefetcher, depth, group, couple_group, ramp, tail)
    gathered = D.all_gather_samples(last[1]) if last is not None else None
    sync(); D.barrier()
    if keep is not None:
        keep["last"] = last
    return D.max_over_ranks(time.perf_counter() - t0, device), gathered


FULL_STEPS = 20000      # --full: step budget of the repeated loops (their counts follow from K alone, never from time)


def full_repeats(steps, want=51):
    """Regions of `steps` steps a repeated --full loop runs by default: `want`, fewer when they would exceed FULL_STEPS."""
    return min(want, max(1, FULL_STEPS // max(1, steps)))


DUMP_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """Write `arrays` (name -> float32 / float64 NumPy array) as path/<name>.npy.  Should they exceed DUMP_BYTES in
    all, every array above 1 MiB keeps a fixed, seeded sample of its rows, and the row indices go beside it as
    <name>.rows.npy (float64)."""
    import zlib
    os.makedirs(path, exist_ok=True)
    out = dict(arrays)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BYTES:
        frac = 0.9 * DUMP_BYTES / total
        for name, a in arrays.items():
            if a.ndim >= 1 and a.shape[0] > 1 and a.nbytes > (1 << 20):
                rng = np.random.default_rng(zlib.crc32(name.encode()))
                rows = np.sort(rng.choice(a.shape[0], size=max(1, int(a.shape[0] * frac)), replace=False))
                out[name], out[name + ".rows"] = a[rows], rows.astype(np.float64)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(out)


# --------------------------------------------------------------------------- side legs (rank 0, N = 1)
def _sk_state(r):
    """The solver's own state block after a solve (first 48 bytes of its workspace: csrc/sinkhorn.hip SkState)."""
    s = r.ws[:48].cpu()
    i, d = s[:16].view(torch.int32), s[16:48].view(torch.float64)
    return {"iters_done": int(i[1]), "fp64_exp_engaged": bool(int(i[3])), "last_err": float(d[2])}


def _sk_windows(fn, iters, nwin):
    """nwin timed windows of `iters` iterations each (HIP events on the current stream), after a first-touch pass; every
    window with the solver's state after it — a slow window can then be told from a regime switch (the kernels move to
    fp64 exp once the marginal violation nears the fp32 noise floor) or an early stop."""
    # warm-up: first touch of every buffer, then at least 150 ms of the same work — the leg starts behind host-side input
    # generation during which the chip idles, and the first tens of milliseconds after an idle stretch run at a fraction
    # of the rate (power state): the driver's round-4 figure of 4.7 k it/s at C5 was ONE 200-iteration window right
    # there, and a first window at 2.4 k it/s next to six at 10.3 k was seen again in round 5 before this warm-up existed
    fn(20); torch.cuda.synchronize()
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 0.15:
        fn(iters); torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); r = fn(iters); e1.record(); torch.cuda.synchronize()
        st = _sk_state(r)
        out.append({"ms": e0.elapsed_time(e1), **st})
    return out


def sinkhorn_leg(dev, cfg, reg, iters=200, nwin=7):
    """Sinkhorn iterations/s (one iteration = one g-update + one f-update = two LSE passes over M): the MEDIAN of `nwin`
    windows of `iters` iterations, every window in the line with the iterations it really ran and whether the fp64-exp
    regime engaged; on its own stream (the legacy default stream joins with whatever the earlier legs left behind).
    d <= 8 (C2) is measured on the solver OTPlanSampler takes there — variant B, the cost entry recomputed on
    the fly, no B^2 traffic — and reported against the SAME algorithmic bytes, labelled; the
    matrix-streaming solver's rate on the same input is kept next to it."""
    import cfm_amd.optimal_transport as ot
    import cfm_oracle as oracle
    x0, x1 = oracle.config_inputs(cfg)
    points = x0.shape[1] <= 8
    with torch.cuda.stream(torch.cuda.Stream()):
        a, b = x0.to(dev), x1.to(dev)
        M = ot.cost_matrix(a, b)
        win_stream = _sk_windows(lambda n: ot.sinkhorn_log(M, reg, max_iter=n, stop_thr=0.0), iters, nwin)
        win = _sk_windows(lambda n: ot.sinkhorn_log_points(a, b, M, reg, max_iter=n, stop_thr=0.0), iters, nwin) if points else win_stream
        torch.cuda.synchronize()

    def rate(ws):          # iterations really run / time, window by window; then the median
        return float(np.median([w["iters_done"] / (w["ms"] * 1e-3) for w in ws]))
    its, its_stream = rate(win), rate(win_stream)
    rates = [w["iters_done"] / (w["ms"] * 1e-3) for w in win]
    B0, B1 = M.shape
    per_iter_bytes = 2 * 4 * B0 * B1 + 16 * B0
    gbs = per_iter_bytes * its / 1e9
    note = ("2 LSE passes over the fp32 cost matrix per iteration; the %d MiB matrix is %s" %
            (4 * B0 * B1 >> 20, "Infinity-Cache resident (256 MiB)" if 4 * B0 * B1 <= (200 << 20) else "HBM streamed"))
    if points:
        note = ("variant B: the cost entry is recomputed from the coordinates inside both LSE passes, so NO matrix "
                "bytes move; achieved = the algorithmic 2 x 4 x B^2 bytes per iteration / time (it may exceed the "
                "HBM peak: it is an equivalent rate, the kernel is VALU / exp bound); matrix-streaming solver on the "
                "same input: %.0f it/s" % its_stream)
    # HBM bytes per iteration from the committed counter passes (profiles/rNN_sk_pmc_summary.json: rocprofv3 --pmc
    # FETCH_SIZE x2 + WRITE_SIZE over tools/sk_probe.py), next to the algorithmic figure
    traffic = None
    try:
        pmc = json.load(open(newest_profile("sk_pmc_summary.json")))
        traffic = pmc.get(f"{cfg}_points_hbm_bytes_per_iteration" if points else f"{cfg}_streaming_hbm_bytes_per_iteration")
        traffic_stream = pmc.get(f"{cfg}_streaming_hbm_bytes_per_iteration")
    except Exception:  # noqa: BLE001
        traffic_stream = None
    return {"config": f"{cfg}: B={B0}, d={x0.shape[1]}, eps={reg}", "sinkhorn_iters_per_s": its,
            "ms_per_iter": 1e3 / its, "variant": "points (on-the-fly cost)" if points else "matrix streaming",
            "windows": len(win), "iters_per_window": iters,
            "iters_per_s_all": [round(x, 1) for x in rates], "spread_rel": (max(rates) - min(rates)) / its,
            "iters_done_all": [w["iters_done"] for w in win],
            "fp64_exp_engaged_all": [w["fp64_exp_engaged"] for w in win], "last_err": win[-1]["last_err"],
            "sinkhorn_iters_per_s_matrix_streaming": its_stream,
            "matrix_streaming_iters_per_s_all": [round(w["iters_done"] / (w["ms"] * 1e-3), 1) for w in win_stream],
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_matrix_streaming": traffic_stream,
                         "bytes_per_iter": per_iter_bytes, "note": note}}


def sinkhorn_extra_legs(dev, iters=200):
    """The Sinkhorn variants no line carried so far: variant B (cost recomputed from the coordinates)
    at its largest dimension d = 8, and the matrix-streaming solver on a d = 50 cloud at B = 4096 (the C5 data at the
    C2 batch size: a 64 MiB matrix, Infinity-Cache resident).  Fixed iteration counts (stop_thr = 0)."""
    import cfm_amd.optimal_transport as ot
    import cfm_oracle as oracle
    out = {}

    def timed(fn):
        fn(20); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(iters); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    g = torch.Generator().manual_seed(8)
    a = torch.randn(4096, 8, generator=g).to(dev); b = (torch.randn(4096, 8, generator=g) * 0.8 + 0.5).to(dev)
    M = ot.cost_matrix(a, b)
    ms = timed(lambda n: ot.sinkhorn_log_points(a, b, M, 0.5, max_iter=n, stop_thr=0.0))
    ms_s = timed(lambda n: ot.sinkhorn_log(M, 0.5, max_iter=n, stop_thr=0.0))
    out["points_d8_iters_per_s"] = iters / (ms * 1e-3)
    out["points_d8_matrix_streaming_iters_per_s"] = iters / (ms_s * 1e-3)
    x0, x1 = oracle.config_inputs("C5", B=4096)
    M50 = ot.cost_matrix(x0.to(dev), x1.to(dev))
    ms50 = timed(lambda n: ot.sinkhorn_log(M50, 0.1, max_iter=n, stop_thr=0.0))
    out["d50_B4096_iters_per_s"] = iters / (ms50 * 1e-3)
    out["d50_B4096_gbs"] = (2 * 4.0 * 4096 * 4096 + 16 * 4096) * iters / (ms50 * 1e-3) / 1e9
    out["extra_config"] = "B=4096: d=8 Gaussian clouds (variant B and the streaming solver, eps=0.5); d=50 C5-shaped clouds (streaming, eps=0.1)"
    return out


def c5_ode_leg(dev):
    """C5 sampling: dopri5 (atol = rtol = 1e-4, t_span = linspace(0, 1, 100)) through the 51-64-64-64-50
    SELU MLP field on B = 8192 points (single-cell_example.ipynb cells 5-9 shape)."""
    import cfm_amd
    import cfm_oracle as oracle
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    x0, _ = oracle.config_inputs("C5")
    torch.manual_seed(0)
    model = cfm_amd.MLP(dim=50, time_varying=True, w=64).to(dev)
    node = NeuralODE(torch_wrapper(model), solver="dopri5", sensitivity="adjoint", atol=1e-4, rtol=1e-4)
    ts = torch.linspace(0, 1, 100)
    x = x0.to(dev)
    # on its own stream (the drivers synchronise the stream they run on: on the legacy default stream that is a
    # device-wide join with whatever the earlier legs left behind); median of 5 wall-clock times
    times = []
    with torch.cuda.stream(torch.cuda.Stream()):
        node.trajectory(x, ts)
        torch.cuda.synchronize()
        for _ in range(5):
            t0 = time.perf_counter()
            node.trajectory(x, ts)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(times))
    flops = node.nfe * 2 * x.shape[0] * (51 * 64 + 64 * 64 + 64 * 64 + 64 * 50)
    tf = flops / (ms * 1e-3) / 1e12
    return {"dopri5_ms": ms, "dopri5_ms_all": [round(t, 3) for t in times], "nfe": int(node.nfe), "step_attempts": int(node.n_steps),
            "roofline_ode": {"bound": "latency", "us_per_nfe": 1e3 * ms / max(1, int(node.nfe)),
                             "us_per_step_attempt": 1e3 * ms / max(1, int(node.n_steps)),
                             "mfma_tflops_context": tf, "mfma_frac_context": tf / F32_PEAK_TFLOPS,
                             "note": "a chain of nfe dependent 4-layer products of width 64 in ONE persistent launch: the "
                                     "figure of merit is the time per function evaluation (us_per_nfe); the MFMA rate "
                                     "(nfe x MLP flops / wall) is context, not a roofline this chain can approach"}}


def c1_latency(dev, reps=20):
    """Exact-OT coupling latency at the reference's tutorial size (B = 256, d = 2; BASELINE configs[0])."""
    import cfm_amd.optimal_transport as ot
    import cfm_oracle as oracle
    x0, x1 = oracle.config_inputs("C1")
    a, b = x0.to(dev), x1.to(dev)
    samp = ot.OTPlanSampler(method="exact")
    for _ in range(3):
        samp.sample_plan(a, b)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); samp.sample_plan(a, b); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    M = ot.cost_matrix(a, b)
    tsolve = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); ot.assign_exact(M); tsolve.append(time.perf_counter() - t0)
    return {"sample_plan_ms": float(np.median(ts) * 1e3), "solve_ms": float(np.median(tsolve) * 1e3)}


def aux_legs(dev):
    """Timings of the path's other solvers (VERDICT r2 Weak #9: they were parity-only): the SF2M Euler-Maruyama
    sampler (two 3-64-64-64-2 fields, B = 2048, 100 steps: SF2M_tutorial.ipynb cell 5 shape) and one iteration of the
    kernel-space unbalanced / partial entropic solvers on the C2 clouds (B = 4096; reg = 5: the float64 Gibbs kernel
    is alive there; 2 x 8 x B^2 bytes of fp64 kernel per iteration)."""
    import cfm_amd
    import cfm_amd.optimal_transport as ot
    import cfm_oracle as oracle
    from cfm_amd.sde import FlowScoreSDE, sdeint
    out = {}
    torch.manual_seed(0)
    f = cfm_amd.MLP(dim=2, time_varying=True, w=64).to(dev); sc = cfm_amd.MLP(dim=2, time_varying=True, w=64).to(dev)
    x0, _ = oracle.config_inputs("C1", B=2048)
    y0 = x0.to(dev); ts = torch.linspace(0, 1, 2)
    sde = FlowScoreSDE(f, sc, sigma=0.1)
    sdeint(sde, y0, ts, dt=0.01); torch.cuda.synchronize()
    tt = []
    for _ in range(5):
        t0 = time.perf_counter(); sdeint(sde, y0, ts, dt=0.01); torch.cuda.synchronize()
        tt.append((time.perf_counter() - t0) * 1e3)
    out["sde_em_ms"] = float(np.median(tt))
    out["sde_em_config"] = "SF2M Euler-Maruyama, B=2048, d=2, two w=64 fields, 100 steps"
    a, b = oracle.config_inputs("C2")
    M = ot.cost_matrix(a.to(dev), b.to(dev))
    Bn = M.shape[0]
    for name, fn in (("unbalanced", lambda n: ot.unbalanced_plan(M, 5.0, 1.0, max_iter=n, stop_thr=0.0)),
                     ("partial", lambda n: ot.partial_plan(M, 5.0, 1.0, max_iter=n, stop_thr=0.0))):
        fn(5); torch.cuda.synchronize()

        def timed(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); _, info = fn(n); e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1), int(info[0].item())
        ta, ia = min(timed(5) for _ in range(5))         # fastest of five: a one-shot difference of two calls is at the
        tb, ib = min(timed(45) for _ in range(5))        # mercy of one allocator / clock hiccup
        if ib > ia:                                      # (the loops stop by themselves once they have converged)
            per = (tb - ta) / (ib - ia)                  # ms per iteration without the kernel build / plan write
            out[f"{name}_iters_per_s"] = 1e3 / per
            out[f"{name}_gbs"] = 2 * 8.0 * Bn * Bn / (per * 1e-3) / 1e9
        out[f"{name}_iters_timed"] = [ia, ib]
    # exact OT between batches of DIFFERENT sizes beyond the lcm expansion (127 vs 128): the transportation solver
    try:
        g = torch.Generator().manual_seed(0)
        xa = torch.randn(127, 2, generator=g).to(dev); xb = (torch.randn(128, 2, generator=g) * 0.7 + 0.5).to(dev)
        Mr = ot.cost_matrix(xa, xb)
        ot.transport_exact(Mr)
        tt = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter(); ot.transport_exact(Mr); tt.append((time.perf_counter() - t0) * 1e3)
        out["transport_127x128_ms"] = float(np.median(tt))
    except Exception as exc:  # noqa: BLE001 — a side leg must not take the line down
        out["transport_127x128_ms"] = None; out["transport_error"] = repr(exc)
    out["ot_kernel_space_config"] = "C2 clouds, B=4096, reg=5.0 (reg_m=1 / m=1): per-iteration rate from the 45- vs 5-iteration difference, fastest of five each (iteration counts read back)"
    return out


def cpu_baseline(B, d, budget_s=25.0):
    """The reference's CPU step restated by the oracle — OTPlanSampler('exact').sample_plan +
    sample_location_and_conditional_flow (optimal_transport.py:63-145, conditional_flow_matching.py:159-199)
    — timed on this box's host cores with a per-stage breakdown: torch.cdist ** 2, the exact solve
    (SciPy LSAP in float64: the stand-in for POT's network simplex, which is not installable here; it is
    single threaded whatever num_threads says, and an UPPER bound on POT's time), the reference's own
    O(B^2) sample_map (dense float64 plan, flatten, / sum, np.random.choice) and the eager gather + x_t / u_t."""
    import cfm_oracle as oracle
    x0, x1 = oracle.config_inputs("C3", B=B)
    torch.manual_seed(0); np.random.seed(0)
    threads_max = torch.get_num_threads()

    def one(nthreads):
        torch.set_num_threads(nthreads)
        t = [time.perf_counter()]
        M = oracle.ref_cost_f32(x0, x1); t.append(time.perf_counter())
        perm = oracle.exact_perm(M); t.append(time.perf_counter())
        pi = oracle.perm_plan(perm)                               # pot.emd returns the dense plan
        i, j = oracle.sample_map_reference(pi, B); t.append(time.perf_counter())
        a0, a1 = x0[i], x1[j]
        tt = torch.rand(B).type_as(x0); eps = torch.randn_like(a0)
        oracle.xt_ut("icfm", a0, a1, tt, eps, 0.0); t.append(time.perf_counter())
        return np.diff(t)

    t_start = time.perf_counter()
    one(threads_max)                                              # warm-up
    per = (time.perf_counter() - t_start)
    nrun = int(max(1, min(5, (budget_s - per) // max(per, 1e-3) - 1)))
    runs = np.array([one(threads_max) for _ in range(nrun)])
    run1 = one(1)                                                 # torch intra-op threads = 1 (reference default for emd)
    torch.set_num_threads(threads_max)
    med = np.median(runs, axis=0)
    total = float(med.sum())
    # CPU Sinkhorn iterations/s ("time a fixed 100 iterations of the float64 two-mat-vec loop"): POT's
    # sinkhorn_knopp iteration as the reference runs it (optimal_transport.py:51,87): K = exp(M / -reg) in float64,
    # v = b / (K^T u), u = 1 / (Kp v) — two dense mat-vecs over B^2 doubles per iteration (NumPy / the host BLAS, all
    # cores).  A FIXED number of iterations: at the reference's reg the loop would stop on its numerical-error check at
    # once (K underflows), which changes nothing about what an iteration costs.  C2 (B = 4096): 100 iterations; C5
    # (B = 8192, 512 MiB of K): 30.  Next to it the float64 log-domain loop in C (oracle/sinkhorn_oracle.c, OpenMP),
    # the form the GPU solver computes, 20 iterations at C2.
    def knopp_rate(cfg, reg, iters):
        a0, a1 = oracle.config_inputs(cfg)
        Mc = oracle.ref_cost_f32(a0, a1).astype(np.float64)
        K = np.exp(Mc / (-reg)); del Mc
        n, m = K.shape
        Kp = K * float(n)                                   # (1 / a) K with a = 1 / n
        u = np.full(n, 1.0 / n); v = np.full(m, 1.0 / m); b = np.full(m, 1.0 / m)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            KtU = K.T @ u; v = b / KtU; u = 1.0 / (Kp @ v)     # warm-up
            t0 = time.perf_counter()
            for _ in range(iters):
                KtU = K.T @ u
                v = b / KtU
                u = 1.0 / (Kp @ v)
            dt = time.perf_counter() - t0
        return {"config": f"{cfg}: B={n}, eps={reg}", "iters_per_s": iters / dt, "iters_timed": iters,
                "gbs": 2 * 8.0 * n * m * iters / dt / 1e9, "cores": os.cpu_count(), "kind": "port",
                "sample": f"{iters} iterations of the float64 two-mat-vec Knopp loop (NumPy / host BLAS)"}
    sk_cpu = None
    try:
        sk_cpu = {"c2_knopp": knopp_rate("C2", 0.05, 100), "c5_knopp": knopp_rate("C5", 0.1, 30)}
        import sinkhorn_c
        a0, a1 = oracle.config_inputs("C2")
        Mc = oracle.ref_cost_f32(a0, a1)
        sinkhorn_c.sinkhorn_log(Mc, 0.05, numItermax=1, stopThr=0.0)          # warm-up (loads / builds the library)
        t0 = time.perf_counter(); sinkhorn_c.sinkhorn_log(Mc, 0.05, numItermax=20, stopThr=0.0); dt = time.perf_counter() - t0
        nth = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
        sk_cpu["c2_log_domain_c"] = {"config": "C2: B=4096, d=2, eps=0.05", "iters_per_s": 20.0 / dt, "cores": nth, "kind": "port",
                                     "sample": f"20 iterations of the float64 log-domain loop in C (oracle/sinkhorn_oracle.c), "
                                               f"OpenMP over rows / columns, {nth} threads"}
        sk_cpu["iters_per_s"] = sk_cpu["c2_knopp"]["iters_per_s"]
    except Exception as e:                                                        # noqa: BLE001  (no C compiler on the box)
        sk_cpu = dict(sk_cpu or {}, error=str(e)[:160])
    # C1 (BASELINE configs[0] IS the reference's CPU path: Flow_matching_tutorial.ipynb cell 16): the exact coupling of
    # one B = 256, d = 2 minibatch on the host — cdist^2, LSAP, the dense-plan np.random.choice — median of 20
    c1_cpu = None
    try:
        b0, b1 = oracle.config_inputs("C1")
        ts = []
        for _ in range(21):
            t0 = time.perf_counter()
            Mq = oracle.ref_cost_f32(b0, b1); t1 = time.perf_counter()
            pq = oracle.exact_perm(Mq); t2 = time.perf_counter()
            oracle.sample_map_reference(oracle.perm_plan(pq), 256)
            ts.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
        med1 = np.median(np.array(ts[1:]), axis=0) * 1e3
        c1_cpu = {"cpu_ms": float(med1.sum()), "cpu_solve_ms": float(med1[1]), "cpu_cdist_ms": float(med1[0]),
                  "cpu_sample_map_ms": float(med1[2]), "cores": 1, "kind": "port",
                  "sample": "20 couplings of B=256, d=2 (cdist**2 + SciPy LSAP + dense-plan np.random.choice), per-stage medians"}
    except Exception as e:                                                        # noqa: BLE001
        c1_cpu = {"error": str(e)[:160]}
    return {"value": B / total, "unit": "samples/s", "cores": 1, "kind": "port", "sinkhorn_cpu": sk_cpu, "c1": c1_cpu,
            "s_per_step_median": total, "s_per_step_min": float(runs.sum(1).min()), "runs": int(nrun),
            "breakdown_s": {"cdist2": float(med[0]), "exact_solve_scipy_lsap": float(med[1]),
                            "sample_map_dense_choice": float(med[2]), "gather_xt_ut": float(med[3])},
            "s_per_step_torch_threads_1": float(run1.sum()),
            "sample": f"{nrun} timed step(s) after 1 warm-up of B={B}, d={d} (median): torch.cdist**2 + SciPy LSAP f64 "
                      f"(stand-in for POT emd; single threaded: the solve is 1 core whatever num_threads is, so "
                      f"cores=1 although torch used {threads_max} intra-op threads for cdist / gathers) + the "
                      f"reference's dense-plan np.random.choice sampling + eager xt/ut; host has {os.cpu_count()} cores"}


def parity_leg(dev, ot, budget_s=60.0):
    """Results parity of the product path against the REFERENCE path on the same inputs, reported in the line
    (VERDICT r2 Next #1): exact-OT plan indices of cost kernel + HIP solver vs LSAP on the reference's own fp32
    matrix torch.cdist(x0, x1) ** 2 (optimal_transport.py:84-87; SciPy LSAP in float64 = the support of pot.emd
    with uniform equal marginals, and the reference's own solver at :179).  The oracle is the checker here, never
    the thing measured.  c3: BASELINE configs[2] (B = 4096, d = 784).  c2: the d = 2 clouds of configs[1] used
    with the exact method, where SURVEY 0.5 found the optimum to be decided below fp32 cost rounding (18 of 4096
    indices differed between two fp32 roundings of the same matrix): the index agreement is reported together with
    the cost gap of the two optima priced on the reference's matrix."""
    import cfm_oracle as oracle
    out = {}

    def one(cfg, B):
        x0, x1 = oracle.config_inputs(cfg, B=B)
        Mref = oracle.ref_cost_f32(x0, x1)
        t0 = time.perf_counter(); ref = oracle.exact_perm(Mref); t_cpu = time.perf_counter() - t0
        perm = ot.assign_exact(ot.cost_matrix(x0.to(dev), x1.to(dev))).cpu().numpy()
        M64 = Mref.astype(np.float64); ar = np.arange(B)
        c_ref, c_gpu = float(M64[ar, ref].sum()), float(M64[ar, perm].sum())
        return float((perm == ref).mean()), (c_gpu - c_ref) / abs(c_ref), t_cpu

    agree, gap, t3 = one("C3", 4096)
    out.update({"c3_index_agreement": agree, "c3_cost_gap_rel": gap, "c3_B": 4096})
    agree, gap, t2 = one("C2", 2048)
    Bc2 = 2048
    if 10.0 * t2 + t3 < budget_s:                       # LSAP on d = 2 clouds: ~8x per doubling
        agree, gap, _ = one("C2", 4096); Bc2 = 4096
    out.update({"c2_index_agreement": agree, "c2_cost_gap_rel": gap, "c2_B": Bc2,
                "note": "index agreement = fraction of rows whose plan index equals LSAP (float64) on the reference's "
                        "torch.cdist**2 fp32 matrix; cost gap = (cost of the product path's permutation - optimum) / "
                        "optimum, both priced on the reference's matrix"})
    return out


def assign_roofline(dev, pool, lib, _lib, ot, B, nsolves=8, nbatch=4):
    """Dominant kernel family of the coupling: the chip-wide kernels of the exact-assignment state machine — asg_auction
    (the epsilon > 0 phases, one launch) and asg_step (every other chip-wide step).  Un-overlapped solves on one stream.
    Algorithmic bytes per SURVEY §8d: 4 B x n per row evaluation (the fp32 cost row) + 8 B x n prices per launch.
    Launch durations: the device books the time of every step on its own 100 MHz clock (cfm_assign_debug_times); HIP
    events bracket each solve on its stream.  `batch`: the same figure for the form the headline schedule runs —
    cfm_assign_exact_batch_f32 with `nbatch` problems in one chain of launches (the auction on 16 workgroups per
    problem): nbatch x the algorithmic bytes / the booked time of the chain's chip-wide launches."""
    Ms = [ot.cost_matrix(x0, x1) for (x0, x1) in pool[:nsolves]]
    ws = _lib.workspace(_lib.OP_ASSIGN, B, B, 0, dev)
    for M in Ms[:2]:
        ot.assign_exact(M)

    def booked(wsbuf):
        buf = (ctypes.c_double * 32)()
        _lib.check(lib.cfm_assign_debug_times(_lib.ptr(wsbuf), buf), "cfm_assign_debug_times")
        return np.array(list(buf))
    ev_ms, step_us, steps, scans, solver_us, listed, auction_us = [], [], [], [], [], [], []
    for M in Ms:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); perm, info = ot.assign_exact(M, return_info=True); e1.record(); torch.cuda.synchronize()
        t = booked(ws)
        ev_ms.append(e0.elapsed_time(e1)); step_us.append(float(t[:11].sum())); solver_us.append(float(t[11:13].sum()))
        steps.append(info["stats"][6]); scans.append(info["stats"][5]); listed.append(float(t[16])); auction_us.append(float(t[2]))
    steps_m, scans_m, listed_m = float(np.mean(steps)), float(np.mean(scans)), float(np.mean(listed))
    bytes_solve = scans_m * 4.0 * B + steps_m * 8.0 * B
    t_step = float(np.mean(step_us)) * 1e-6
    gbs = bytes_solve / t_step / 1e9
    traffic = None
    pmc = newest_profile("asg_pmc_summary.json")
    if pmc and os.path.exists(pmc):
        try:
            traffic = json.load(open(pmc)).get("asg_chip_wide_hbm_bytes_per_solve")      # (rounds 1-4 committed a per-launch figure: None then)
        except Exception:  # noqa: BLE001
            traffic = None
    # the batch form (what the pipelined schedule runs)
    batch = None
    try:
        nbq = min(nbatch, len(Ms))
        wsb = _lib.workspace(_lib.OP_ASSIGN, B, B, nbq, dev)
        ot.assign_exact_batch(Ms[:nbq]); torch.cuda.synchronize()
        b_ms, b_step_us, b_scans, b_steps = [], [], [], []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); _, infos = ot.assign_exact_batch(Ms[:nbq], return_info=True); e1.record(); torch.cuda.synchronize()
            tb = booked(wsb)                                   # (problem 0's books: the chain's launches carry all problems)
            b_ms.append(e0.elapsed_time(e1)); b_step_us.append(float(tb[:11].sum()))
            b_scans.append(sum(i["stats"][5] for i in infos)); b_steps.append(infos[0]["stats"][6])
        b_bytes = float(np.mean(b_scans)) * 4.0 * B + float(np.mean(b_steps)) * 8.0 * B * nbq
        b_gbs = b_bytes / (float(np.median(b_step_us)) * 1e-6) / 1e9
        batch = {"problems": nbq, "achieved": b_gbs, "frac": b_gbs / HBM_PEAK_GBS, "unit": "GB/s",
                 "chip_wide_launch_ms": float(np.median(b_step_us)) * 1e-3, "batch_ms": float(np.median(b_ms)),
                 "ms_per_problem": float(np.median(b_ms)) / nbq, "row_evaluations": float(np.mean(b_scans)),
                 "note": "cfm_assign_exact_batch_f32: the form the headline schedule runs; achieved = algorithmic bytes of all "
                         "problems / booked time of the chain's chip-wide launches (asg_auction on 16 workgroups per problem + "
                         "asg_step); the one-workgroup list solvers run beside the next launches and are not in this time"}
    except Exception as exc:  # noqa: BLE001 — a side figure must not take the line down
        batch = {"error": repr(exc)[:200]}
    return {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
            "traffic": traffic, "kernel": "asg_auction + asg_step (cfm_assign_exact_f32)",
            "launches_per_solve": steps_m, "avg_launch_us": float(np.mean(step_us)) / steps_m,
            "auction_launch_us": float(np.mean(auction_us)),
            "algorithmic_bytes_per_solve": bytes_solve, "algorithmic_bytes_per_launch": bytes_solve / steps_m, "row_scans_per_solve": scans_m,
            "row_scans_served_from_bid_lists": listed_m,
            "bytes_read_per_solve_by_construction": (scans_m - listed_m) * 4.0 * B + listed_m * 1024.0 + steps_m * 8.0 * B,
            "solve_ms": float(np.mean(ev_ms)), "list_solver_ms": float(np.mean(solver_us)) * 1e-3,
            # the same algorithmic bytes over the WHOLE solve (list build + one-workgroup list solver included): the figure
            # the north star's ">= 40 % of HBM" is about; `frac` above books the chip-wide launches only
            "whole_solve_achieved": bytes_solve / (float(np.mean(ev_ms)) * 1e-3) / 1e9,
            "whole_solve_frac": bytes_solve / (float(np.mean(ev_ms)) * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "chip_wide_ms": t_step * 1e3, "batch": batch,
            "note": "latency-bound: the figure of merit is solve_ms; achieved = (4B x n per row evaluation + 8B x n prices "
                    "per launch) / booked time of the chip-wide launches of an un-overlapped solve (SURVEY 8d's algorithmic "
                    "figure: a row evaluation = one bid of the auction / one row of the forest; "
                    "row_scans_served_from_bid_lists of them read the row's 64-entry bid list (512 B + 64 prices) instead of "
                    "the 4 B x n row, so the bytes actually requested are bytes_read_per_solve_by_construction); since round 5 "
                    "the epsilon > 0 phases are ONE launch (asg_auction, auction_launch_us) instead of ~90, so the unit of "
                    "achieved / traffic is the SOLVE (its chip-wide launches together); traffic (if present) = HBM bytes per "
                    "solve over asg_auction + asg_step from the committed rocprofv3 --pmc passes (profiles/), FETCH x2 + WRITE"}


def self_launch(args, argv):
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: start the N ranks ourselves (one process
    per GPU, `torch.distributed.run` on 127.0.0.1 — what examples/images/cifar10/train_cifar10_ddp.py:201-210 expects
    its user to type).  Returns the launcher's exit code, or None when this process is itself a rank (or N = 1).
    Fails loudly when the box has fewer GPUs than ranks: a silent N = 1 run would be reported as an N-GPU number."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return None
    if not args.cpu_standin:
        if not torch.cuda.is_available():
            raise SystemExit(f"bench.py --gpus {args.gpus}: no GPU visible (the bench measures the HIP path; no CPU fallback)")
        if torch.cuda.device_count() < args.gpus and not os.environ.get("CFM_BENCH_SHARE_GPU"):
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {torch.cuda.device_count()} GPU(s) visible on this box; "
                             f"one rank per GPU is required (refusing to oversubscribe or to run fewer ranks)")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    return subprocess.call(cmd, env=env)


def cpu_standin_main(args):
    """Launcher self-test (`--cpu-standin`, used by tests/test_bench_launcher.py): every rank runs bench.py's own
    rank plumbing — init from torchrun's env over gloo, per-rank pool, run_steps / timed_region with the prefetch
    pipeline, DDP model, one all-gather, max-over-ranks timing, rank 0 prints the line — on CPU tensors with a trivial
    index-paired coupling.  Nothing is measured: the line says so and carries "valid": false."""
    from cfm_amd import distributed as D
    from cfm_amd.prefetch import CouplingPrefetcher
    os.environ.setdefault("CFM_DIST_BACKEND", "gloo")
    rank, local, world = D.init_from_env(backend="gloo")
    B, d = min(args.batch, 64), min(args.dim, 8)
    g = torch.Generator().manual_seed(D.shard_seed(1000, rank))
    pool = [(torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)) for _ in range(4)]
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(d + 1, 16), torch.nn.SELU(), torch.nn.Linear(16, d))
    if world > 1:
        model = torch.nn.parallel.DistributedDataParallel(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    np.random.seed(D.shard_seed(1, rank)); torch.manual_seed(D.shard_seed(1, rank))

    def draw():
        return np.random.random_sample(B), torch.rand(B)

    def couple(x0, x1, drawn):
        t = drawn[1]
        return t, t[:, None] * x1 + (1 - t[:, None]) * x0, x1 - x0

    def model_step(t, xt, ut):
        opt.zero_grad(set_to_none=True)
        torch.mean((model(torch.cat([xt, t[:, None]], dim=-1)) - ut) ** 2).backward()
        opt.step()

    def couple_group(batches, drawn):
        return [couple(x0, x1, dr) for (x0, x1), dr in zip(batches, drawn)]

    if args.host_cost:
        # HOST-COST stand-in (VERDICT r4 Next #10): what the host side of a rank costs per step when the device work is
        # replaced by waits of its measured duration with the GIL released (a coupling job of g minibatches: g x 0.9 ms
        # of launch chain — the solver's host thread sits in hipEventSynchronize —, a model step: 0.45 ms in flight while
        # the host runs ahead): the real loop (run_steps, the prefetch workers, the host RNG draws of the real batch
        # size, the futures and hand-overs) with nothing but that left.  Reported: process CPU time per step (all
        # threads) — below the GPU step means one host core per rank carries the loop.
        Bh = args.batch
        hb = [(torch.zeros(1), torch.zeros(1)) for _ in range(4)]

        def draw():                                                   # noqa: F811  (the real draws: 8 B x B + 4 B x B per coupling)
            return np.random.random_sample(Bh), torch.rand(Bh)

        def couple(x0, x1, drawn):                                    # noqa: F811
            time.sleep(0.9e-3)
            return drawn[1], x0, x1

        def couple_group(batches, drawn):                             # noqa: F811
            time.sleep(0.9e-3 * len(batches))
            return [(dr[1], x0, x1) for (x0, x1), dr in zip(batches, drawn)]

        def model_step(t, xt, ut):                                    # noqa: F811
            time.sleep(0.45e-3)
        pool = hb

    pre = CouplingPrefetcher(None, torch.device("cpu"), workers=args.pipeline) if args.pipeline else None
    if pre is not None:
        pre.prime(lambda: None)
    regions, cpu_s = [], []
    for _ in range(max(1, args.repeats)):
        c0 = time.process_time()
        el, gathered = timed_region(D, lambda: None, pool, args.warmup, args.steps, couple, model_step, draw, pre,
                                    args.pipeline, torch.device("cpu"), args.group, couple_group)
        cpu_s.append(time.process_time() - c0)
        assert args.host_cost or gathered.shape[0] == world * B
        regions.append(el)
    elapsed = float(np.median(regions))
    # process CPU time (all threads) per step of the slowest rank, warm-up steps included in the denominator
    host_cpu_ms = D.max_over_ranks(float(np.median(cpu_s)) / (args.steps + args.warmup) * 1e3, torch.device("cpu"))
    if pre is not None:
        pre.close()
    if rank == 0:
        print(json.dumps({"metric": "OT-CFM train-step samples/sec (B=4096,d=784)", "value": world * B * args.steps / elapsed,
                          "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "repeats": len(regions), "ms_per_step_all": [round(r / args.steps * 1e3, 4) for r in regions],
                          "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "f32", "data": "cpu-standin (launcher self-test, NOT a measurement)",
                          "valid": False, "host_cpu_ms_per_step": host_cpu_ms, "host_cost_standin": bool(args.host_cost),
                          "host_cores": os.cpu_count(),
                          "config": {"workload": "launcher self-test", "parallelism": f"dp{world}"}}))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=784)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--sigma", type=float, default=0.0)
    ap.add_argument("--mode", default="train", choices=["train", "coupling"])
    ap.add_argument("--pipeline", type=int, default=3,
                    help="N > 0: up to N couplings of the next batches in flight on side streams while the "
                         "model steps on batch k (cfm_amd.prefetch); 0: strictly sequential")
    ap.add_argument("--group", type=int, default=4,
                    help="G > 1: a prefetch job couples G consecutive minibatches together (the exact solver takes the G "
                         "assignment problems in one chain of launches); --pipeline such jobs in flight")
    ap.add_argument("--ramp", default=os.environ.get("CFM_BENCH_RAMP", "1"),
                    help="comma-separated group sizes of the FIRST prefetch jobs of a run (then --group): the pipeline starts "
                         "empty inside the timed region, a small first job lets the first model step start sooner")
    ap.add_argument("--tail", default=os.environ.get("CFM_BENCH_TAIL", "2,1"),
                    help="comma-separated group sizes of the LAST prefetch jobs of a run: the pipeline is drained inside the "
                         "timed region, small last jobs shorten the stretch in which nothing overlaps with the last chain")
    ap.add_argument("--model-step", default="fused", choices=["fused", "eager"],
                    help="fused: cfm_amd.RegressionStep (one C call: forward + MSE + backward, then the one-launch Adam); "
                         "eager: the reference's four lines on the autograd.Function path")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the timed region (warm-up, barrier, K steps, barrier) is repeated this many times, each on a fresh "
                         "empty pipeline; `value` is the MEDIAN region, every region's ms/step is in the line together with "
                         "its p95 / max (VERDICT r5 #2: a median of 7 hid a second mode at 1.9 ms).  Default: 1; with --full "
                         "51, fewer when K x 51 exceeds 20000 steps")
    ap.add_argument("--seq-repeats", type=int, default=7, help="repeats of the sequential (un-overlapped) loops")
    ap.add_argument("--blocking-sync", type=int, default=int(os.environ.get("CFM_BLOCKING_SYNC", "1")),
                    help="1: the prefetch workers' solver waits block in the kernel driver (hipEventBlockingSync) instead of "
                         "spinning on a host core each; 0: HIP's default (spin)")
    ap.add_argument("--partition", type=int, default=int(os.environ.get("CFM_BENCH_PARTITION", "0")),
                    help="K > 0: chip partition (cfm_amd.streams.ChipPartition): K CUs of every XCD for the exact solver's "
                         "streams, the rest for the dense products (cost matrix, model step); 0: every stream on all CUs")
    ap.add_argument("--solver-all", action="store_true", default=bool(os.environ.get("CFM_BENCH_SOLVER_ALL")),
                    help="with --partition K: only the DENSE streams are masked (they leave K CUs per XCD free); the solver's "
                         "streams may use every CU")
    ap.add_argument("--priority", type=int, default=int(os.environ.get("CFM_BENCH_PRIORITY", "0")),
                    help="HIP priority of the coupling workers' streams when no partition is used (-1: high)")
    ap.add_argument("--solver-async", default="",
                    help="A/B switch (not used by the default run): 'on,blocks,last_div' for cfm_assign_set_async — on = 0: the exact "
                         "solver's epsilon > 0 phases as synchronous rounds; blocks: workgroups per problem of the one-launch "
                         "asynchronous auction in the batch entry; last_div: its last phase is cut at stop_frac / last_div")
    ap.add_argument("--solver-sched", default="",
                    help="A/B switch (not used by the default run): 'theta,eps0,eps_last,stop_frac' for cfm_assign_set_params (0 / -1 keep)")
    ap.add_argument("--public-only", action="store_true",
                    help="diagnostics: ONE headline region, then only the pipelined loop through the public API, --repeats times")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline region: the sequential and steady-state "
                         "loops, the public-API loops, the C1 / C2 / C5 / roofline legs, the CPU baseline and the parity "
                         "against the reference path")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the arrays of the last one as DIR/<name>.npy (t, xt, ut of the "
                         "coupling; loss, parameters and gradients of the model step; at most 64 MiB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and parity legs")
    ap.add_argument("--no-legs", action="store_true", help="with --full: skip the C1 / C2 / C5 / roofline legs")
    ap.add_argument("--host-cost", action="store_true",
                    help="with --cpu-standin: device work replaced by waits of its measured duration; the line carries the "
                         "host CPU time per step (max over ranks)")
    ap.add_argument("--cpu-standin", action="store_true",
                    help="launcher self-test on CPU tensors over gloo (no measurement; see cpu_standin_main)")
    args = ap.parse_args()
    pub_repeats = args.repeats if args.repeats is not None else full_repeats(args.steps)     # --public-only
    if args.repeats is None:
        args.repeats = full_repeats(args.steps) if args.full else 1
    if os.environ.get("CFM_BENCH_WATCHDOG"):     # debugging aid: dump every thread's Python stack and exit if the run hangs
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["CFM_BENCH_WATCHDOG"]), exit=True)
    rc = self_launch(args, sys.argv[1:])
    if rc is not None:
        raise SystemExit(rc)
    if args.cpu_standin:
        return cpu_standin_main(args)

    import cfm_amd
    from cfm_amd import _lib, distributed as D
    from cfm_amd.conditional_flow_matching import ExactOptimalTransportConditionalFlowMatcher
    import cfm_amd.optimal_transport as ot

    lib_ = _lib.load()
    if args.solver_async:
        on, blocks, div = (int(x) for x in args.solver_async.split(",")[:3])
        lib_.cfm_assign_set_async(on, blocks, div)
        if len(args.solver_async.split(",")) > 3:      # 4th field: cap on the grid of the solver's other chip-wide kernels
            lib_.cfm_assign_set_wide_blocks(int(args.solver_async.split(",")[3]))
    if args.solver_sched:
        th, e0, el, sf = (float(x) for x in args.solver_sched.split(","))
        lib_.cfm_assign_set_params(th, e0, el, sf, 0, -1, 0)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py measures the HIP path: it needs an MI355X (no CPU fallback exists)")
    rank, local, world = D.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus} (launch with --nproc-per-node {args.gpus}, "
                         f"or run `python bench.py --gpus {args.gpus}` and let it start the ranks)")
    # CFM_BENCH_SHARE_GPU=1 (with CFM_DIST_BACKEND=gloo): a test of the N > 1 code path on a one-GPU box, several ranks on
    # the same device — the line it prints is marked "valid": false, it is no measurement
    shared = bool(os.environ.get("CFM_BENCH_SHARE_GPU")) and world > torch.cuda.device_count()
    if world > torch.cuda.device_count() and not shared:
        raise SystemExit(f"bench.py: {world} ranks but {torch.cuda.device_count()} GPU(s) visible: one rank per GPU")
    dev_index = local % torch.cuda.device_count()     # one rank per GPU on a real node (identity there)
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)
    B, d = args.batch, args.dim

    pool = synth_batches(B, d, min(16, args.steps + args.warmup), D.shard_seed(1000, rank), dev)      # 16 distinct minibatches, cycled (solver time is instance dependent)
    fm = ExactOptimalTransportConditionalFlowMatcher(sigma=args.sigma)
    torch.manual_seed(0)
    model = cfm_amd.MLP(dim=d, time_varying=True, w=args.width).to(dev)
    if world > 1 and args.model_step != "fused":
        model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[dev_index])
    # (fused: RegressionStep averages its flat gradient buffer with one RCCL all-reduce itself; every rank starts
    #  from the same seed-0 weights)
    opt = cfm_amd.FusedAdam(model.parameters(), lr=1e-3)      # one-launch torch.optim.Adam arithmetic
    np.random.seed(D.shard_seed(1, rank)); torch.manual_seed(D.shard_seed(1, rank))

    def draw():
        """the host RNG calls of one coupling, in the reference's order (np.random.choice draw of
        sample_map, ref:118; t from the CPU torch generator, conditional_flow_matching.py:190)"""
        return np.random.random_sample(B), torch.rand(B)

    def couple(x0, x1, drawn):
        """cost -> exact assignment -> sampling -> fused gather + xt/ut, on the CURRENT stream."""
        u_host, t_host = drawn
        M = ot.cost_matrix(x0, x1)     # as OTPlanSampler(method="exact") does
        perm = ot.assign_exact(M)
        u = torch.from_numpy(u_host).to(dev)
        i, j = ot.sample_perm(perm, u, B)
        return fm._sample(x0, x1, t_host.type_as(x0), False, idx=(i, j))

    def couple_group(batches, drawn):
        """the same for several minibatches at once: the G assignment problems go through ONE chain of launches"""
        Ms = [ot.cost_matrix(x0, x1) for x0, x1 in batches]
        perms = ot.assign_exact_batch(Ms)
        outs = []
        for (x0, x1), (u_host, t_host), perm in zip(batches, drawn, perms):
            u = torch.from_numpy(u_host).to(dev)
            i, j = ot.sample_perm(perm, u, B)
            outs.append(fm._sample(x0, x1, t_host.type_as(x0), False, idx=(i, j)))
        return outs

    reg = cfm_amd.RegressionStep(model, opt) if args.model_step == "fused" else None
    eager_loss = {}

    def model_step(t, xt, ut):
        if args.mode != "train":
            return
        if reg is not None:
            # forward (time column fused) + MSE + backward + [gradient all-reduce] + Adam: 10 launches of the library
            reg(t, xt, ut)
            return
        opt.zero_grad(set_to_none=True)
        vt = model(torch.cat([xt, t[:, None]], dim=-1))
        loss = torch.mean((vt - ut) ** 2)
        loss.backward()
        opt.step()
        eager_loss["loss"] = loss

    pre = None
    ramp = tuple(int(x) for x in args.ramp.split(",") if x.strip()) if (args.pipeline and args.group > 1) else ()
    tail = tuple(int(x) for x in args.tail.split(",") if x.strip()) if (args.pipeline and args.group > 1) else ()
    part, main_stream = None, None
    if args.pipeline and args.partition > 0:
        from cfm_amd.streams import ChipPartition
        part = ChipPartition(dev, solver_cus_per_xcd=args.partition, solver_all=args.solver_all)
        main_stream = part.dense_stream()
        torch.cuda.set_stream(main_stream)          # the model step of the pipelined loop runs on the dense CU subset
    if args.pipeline:
        from cfm_amd.prefetch import CouplingPrefetcher
        pre = CouplingPrefetcher(fm, dev, workers=args.pipeline, partition=part, priority=args.priority,
                                 blocking_sync=bool(args.blocking_sync))
        # one-time costs per worker thread (stream, workspaces, the solver's captured launch programs for each job shape
        # the loops are going to submit) are paid before the warm-up steps, on every worker
        rs_np, rs_t = np.random.get_state(), torch.get_rng_state()
        shapes = ({args.group} | set(ramp) | set(tail) | set(range(1, args.group))) if args.group > 1 else {1}
        for k in sorted(shapes - {0}, reverse=True):
            if args.group > 1:
                pre.prime(lambda k=k: couple_group([pool[q % len(pool)] for q in range(k)], [draw() for _ in range(k)]))
            else:
                pre.prime(lambda: couple(*pool[0], draw()))
        np.random.set_state(rs_np); torch.set_rng_state(rs_t)
    # the timed region, `repeats` times (each: warm-up, barrier + sync, EXACTLY K steps on a pipeline that starts empty
    # and is drained, all-gather, sync + barrier; max over ranks) — `value` is the median region (one
    # 27 ms window is a sample, not a measurement)
    def fallbacks():
        fb = (ctypes.c_int * 2)(); lib_.cfm_assign_debug_fallback(fb)
        return int(fb[0]), int(fb[1])
    fb_start = fallbacks()[0]
    thr0 = thread_cpu_seconds()
    cpu0, wall0 = time.process_time(), time.perf_counter()
    kept = {}

    def headline_region():
        el, gathered = timed_region(D, torch.cuda.synchronize, pool, args.warmup, args.steps, couple, model_step,
                                    draw, pre, args.pipeline, dev, args.group, couple_group, ramp, tail, keep=kept)
        assert gathered is None or gathered.shape[0] == world * B
        kept["gathered"] = gathered
        return el
    regions = [headline_region() for _ in range(1 if args.public_only else max(1, args.repeats))]
    # host CPU time of this rank (all threads: the loop + the prefetch workers + the HIP runtime's own) per step, warm-up
    # steps included in the denominator; with spinning event waits every worker in a solve costs a full core
    host_cpu_ms = (time.process_time() - cpu0) / (len(regions) * (args.steps + args.warmup)) * 1e3
    host_wall_ms = (time.perf_counter() - wall0) / (len(regions) * (args.steps + args.warmup)) * 1e3
    thr1 = thread_cpu_seconds()
    wall_regions = time.perf_counter() - wall0
    # busiest threads over the headline regions: CPU seconds / wall seconds of the regions (1.0 = a core kept busy)
    host_threads = sorted(((k.split(":")[0], round((v - thr0.get(k, 0.0)) / wall_regions, 3)) for k, v in thr1.items()),
                          key=lambda kv: -kv[1])[:8]
    fb_headline = fallbacks()[0] - fb_start
    elapsed = float(np.median(regions))
    dumped = None
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path holds after its last step (the last region's), before anything else runs
        arrays = dict(zip(("t", "xt", "ut"), kept.get("last") or ()))
        if world > 1:
            arrays["xt_all_ranks"] = kept["gathered"]
        if args.mode == "train":
            loss = reg.loss if reg is not None else eager_loss.get("loss")
            if loss is not None:
                arrays["loss"] = loss
            for name, p in model.named_parameters():
                arrays["param." + name] = p
                if p.grad is not None:
                    arrays["grad." + name] = p.grad
        arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
        arrays = {k: v if v.dtype in (np.float32, np.float64) else v.astype(np.float32) for k, v in arrays.items()}
        dumped = dump_outputs(args.dump_outputs, arrays)
    # the same loop over a region ten times as long (N = 1): what a step costs once the empty pipeline's fill and its
    # drain (a first coupling nothing overlaps: ~2.6 ms of a 20-step region) are amortised.  Reported next to `value`,
    # never instead of it.
    steady = None
    if args.full and pre is not None and world == 1 and not args.no_legs and not args.public_only:
        ks = min(10 * args.steps, max(args.steps, FULL_STEPS))
        long_regions = [timed_region(D, torch.cuda.synchronize, pool, args.warmup, ks, couple, model_step, draw, pre,
                                     args.pipeline, dev, args.group, couple_group, ramp, tail)[0] for _ in range(3)]
        el = float(np.median(long_regions))
        steady = {"steps": ks, "repeats": 3, "ms_per_step": el / ks * 1e3, "value": B * ks / el,
                  "ms_per_step_all": [round(r / ks * 1e3, 4) for r in long_regions],
                  "note": "same schedule, region of 10 x K steps (at most max(K, 20000); fill + drain of the pipeline "
                          "amortised); `value` is the K-step region"}
    if pre is not None:
        pre.close()
    if main_stream is not None:
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
    # the same K steps strictly one after the other (no overlap at all): what an unmodified script gets
    seq_s, seq_all = None, []
    if args.full and args.pipeline and world == 1:
        n_seq = min(20, args.steps)
        run_steps(pool, 0, 2, couple, model_step, draw)
        for _ in range(max(1, args.seq_repeats)):
            torch.cuda.synchronize(); ts = time.perf_counter()
            run_steps(pool, args.warmup, n_seq, couple, model_step, draw)
            torch.cuda.synchronize(); seq_all.append((time.perf_counter() - ts) / n_seq)
        seq_s = float(np.median(seq_all))
    # the same two loops through the PUBLIC entry points, verbatim (VERDICT r4 Next #6b): the reference's line
    # `t, xt, ut = FM.sample_location_and_conditional_flow(x0, x1)` (conditional_flow_matching.py:241-272;
    # train_cifar10.py:141-149) in the sequential loop, FM.sample_location_and_conditional_flow_group in the pipelined one
    # (the host RNG is then consumed inside the calls — on the worker threads in the pipelined loop).  Both are first
    # asserted BIT-EQUAL to the hand-composed couple() / couple_group() the headline schedule runs, from one RNG state.
    public = None
    if world == 1 and args.pipeline and args.group > 1 and ((args.full and not args.no_legs) or args.public_only):
        def rng_get():
            return np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(dev)

        def rng_set(st):
            np.random.set_state(st[0]); torch.set_rng_state(st[1]); torch.cuda.set_rng_state(st[2], dev)
        st0 = rng_get()
        ref1 = couple(*pool[0], draw())
        rng_set(st0)
        pub1 = fm.sample_location_and_conditional_flow(*pool[0])
        gb = [pool[q % len(pool)] for q in range(args.group)]
        rng_set(st0)
        refg = couple_group(gb, [draw() for _ in gb])
        rng_set(st0)
        pubg = fm.sample_location_and_conditional_flow_group(gb)
        torch.cuda.synchronize()
        bit_equal = all(torch.equal(a, b) for a, b in zip(ref1, pub1)) and \
            all(torch.equal(a, b) for ra, rb in zip(refg, pubg) for a, b in zip(ra, rb))
        rng_set(st0)

        def couple_pub(x0, x1, _drawn):
            return fm.sample_location_and_conditional_flow(x0, x1)

        def couple_group_pub(batches, _drawn):
            return fm.sample_location_and_conditional_flow_group(batches)
        no_draw = lambda: None      # noqa: E731
        n_seq = min(20, args.steps)
        run_steps(pool, 0, 2, couple_pub, model_step, no_draw)
        pub_seq = []
        for _ in range(max(1, args.seq_repeats)):
            torch.cuda.synchronize(); ts = time.perf_counter()
            run_steps(pool, args.warmup, n_seq, couple_pub, model_step, no_draw)
            torch.cuda.synchronize(); pub_seq.append((time.perf_counter() - ts) / n_seq)
        from cfm_amd.prefetch import CouplingPrefetcher
        fb_pub0 = fallbacks()[0]
        pre2 = CouplingPrefetcher(fm, dev, workers=args.pipeline, priority=args.priority, blocking_sync=bool(args.blocking_sync))
        for k in sorted(({args.group} | set(ramp) | set(tail) | set(range(1, args.group))) - {0}, reverse=True):
            pre2.prime(lambda k=k: couple_group_pub([pool[q % len(pool)] for q in range(k)], None))
        pub_regions = [timed_region(D, torch.cuda.synchronize, pool, args.warmup, args.steps, couple_pub, model_step, no_draw,
                                    pre2, args.pipeline, dev, args.group, couple_group_pub, ramp, tail)[0]
                       for _ in range(max(1, pub_repeats if args.public_only else args.repeats))]
        pre2.close()
        pe, ps = float(np.median(pub_regions)), float(np.median(pub_seq))
        public = {"bit_equal_to_headline_composition": bool(bit_equal),
                  "regions": len(pub_regions),
                  "ms_per_step_pipelined_p95": float(np.percentile(pub_regions, 95)) / args.steps * 1e3,
                  "ms_per_step_pipelined_max": max(pub_regions) / args.steps * 1e3,
                  "dense_fallbacks": fallbacks()[0] - fb_pub0,
                  "value_pipelined": B * args.steps / pe, "ms_per_step_pipelined": pe / args.steps * 1e3,
                  "ms_per_step_pipelined_all": [round(r / args.steps * 1e3, 4) for r in pub_regions],
                  "value_sequential": B / ps, "ms_per_step_sequential": ps * 1e3,
                  "ms_per_step_sequential_all": [round(x * 1e3, 4) for x in pub_seq],
                  "note": "sequential: FM.sample_location_and_conditional_flow(x0, x1) per step, verbatim the reference's "
                          "training line; pipelined: FM.sample_location_and_conditional_flow_group(batches) on the prefetch "
                          "workers (same schedule as `value`; the host RNG is drawn inside the calls)"}
    if part is not None:
        part.close()

    if rank != 0:
        return
    value = world * B * args.steps / elapsed
    out = {
        "metric": "OT-CFM train-step samples/sec (B=4096,d=784)", "value": value, "unit": "samples/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "repeats": len(regions), "ms_per_step_all": [round(r / args.steps * 1e3, 4) for r in regions],
        "ms_per_step_min": min(regions) / args.steps * 1e3, "ms_per_step_max": max(regions) / args.steps * 1e3,
        "spread_rel": (max(regions) - min(regions)) / elapsed,
        "spread_rel_iqr": float(np.percentile(regions, 75) - np.percentile(regions, 25)) / elapsed,
        "ms_per_step_p95": float(np.percentile(regions, 95)) / args.steps * 1e3,
        "regions_above_1p15x_median": int(sum(r > 1.15 * elapsed for r in regions)),
        "dense_fallbacks": fb_headline, "dense_fallback_last_error": fallbacks()[1], "host_cpu_ms_per_step": host_cpu_ms, "host_wall_ms_per_step": host_wall_ms,
        "blocking_sync": bool(args.blocking_sync), "host_threads_busy_fraction": host_threads,
        "config": {"workload": "C3: MNIST-shaped d=784, B=4096 per GPU, ExactOptimalTransportConditionalFlowMatcher "
                               "coupling (HIP) + 785-512-512-512-784 SELU MLP fwd/bwd (fp32-MFMA HIP kernels) + fused Adam (HIP)"
                               + ("; one all-gather of the final x_t over RCCL inside the timed region" if world > 1 else ""),
                   "batch_per_gpu": B, "dim": d, "mlp_width": args.width, "mode": args.mode, "model_step": args.model_step,
                   "schedule": ((f"{args.pipeline} prefetch job(s) in flight on side streams during the model step, "
                                 f"each coupling {args.group} consecutive minibatch(es)"
                                 + (" together (their assignment problems share one chain of launches: "
                                    "cfm_assign_exact_batch_f32)" if args.group > 1 else ""))
                                if args.pipeline else "sequential"),
                   "prefetch_jobs": args.pipeline, "prefetch_group": args.group if args.pipeline else 0,
                   "prefetch_ramp": list(ramp), "prefetch_tail": list(tail),
                   "prefetch_job_sizes": job_sizes(args.steps, args.group, ramp, tail) if (args.pipeline and args.group > 1) else None,
                   "chip_partition": ({"solver_cus": part.solver_cus, "dense_cus": part.dense_cus,
                                       "note": "CU-masked streams: the exact solver's launches on solver_cus, cost matrix "
                                               "/ sampling / model step on dense_cus"} if part is not None else None),
                   "worker_stream_priority": args.priority,
                   "parallelism": f"dp{world}" if world > 1 else "single"},
        **({"valid": False, "data": "synthetic; ranks SHARE one GPU (CFM_BENCH_SHARE_GPU): code-path test, NOT a measurement"}
           if shared else {}),
        "value_sequential": (B / seq_s) if seq_s else None,
        "ms_per_step_sequential": seq_s * 1e3 if seq_s else None,
        "ms_per_step_sequential_all": [round(x * 1e3, 4) for x in seq_all],
        "steady_state": steady,
        "value_public_api": public,
    }
    if dumped is not None:
        out["outputs_dumped"] = dumped
    if args.full and world == 1 and not args.no_legs and not args.public_only:
        with torch.cuda.stream(torch.cuda.Stream()):
            out["roofline"] = assign_roofline(dev, pool, lib_, _lib, ot, B)
            out["c1"] = c1_latency(dev)
        c2 = sinkhorn_leg(dev, "C2", 0.05)
        c2.update(sinkhorn_extra_legs(dev))
        out["c2"] = c2
        out["sinkhorn_iters_per_s"] = c2["sinkhorn_iters_per_s"]
        out["roofline_sinkhorn"] = c2["roofline"]
        c5 = sinkhorn_leg(dev, "C5", 0.1)
        c5.update(c5_ode_leg(dev))
        out["c5"] = c5
        out["aux"] = aux_legs(dev)
    else:
        out["roofline"] = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
                           "traffic": None, "note": "reported at N = 1 with --full only"}
    # The driver's record keeps the scalar keys of `roofline` / `config` / `cpu_baseline` only (BENCH_r05: nested objects
    # and the top-level extras were dropped): the second half of BASELINE's metric ("+ Sinkhorn iters/sec") and the other
    # configs' figures are repeated there as flat scalars.  The HBM figure of C2 is the MATRIX-STREAMING
    # solver's; the points variant (no matrix bytes move) is an iterations/s figure only.
    rf = out["roofline"]
    rf.update({"ms_per_step_p95": out["ms_per_step_p95"], "ms_per_step_max": out["ms_per_step_max"],
               "regions": len(regions), "dense_fallbacks": fb_headline,
               "ms_per_step_sequential": out["ms_per_step_sequential"],
               "host_cpu_ms_per_step": host_cpu_ms})
    if public:
        rf.update({"public_api_ms_per_step_pipelined": public["ms_per_step_pipelined"],
                   "public_api_ms_per_step_pipelined_p95": public["ms_per_step_pipelined_p95"],
                   "public_api_ms_per_step_pipelined_max": public["ms_per_step_pipelined_max"],
                   "public_api_ms_per_step_sequential": public["ms_per_step_sequential"],
                   "public_api_dense_fallbacks": public["dense_fallbacks"]})
    if steady:
        rf["steady_state_ms_per_step"] = steady["ms_per_step"]
    if isinstance(rf.get("batch"), dict) and "frac" in rf["batch"]:
        rf.update({"batch_frac": rf["batch"]["frac"], "batch_achieved": rf["batch"]["achieved"],
                   "batch_ms_per_problem": rf["batch"]["ms_per_problem"]})
    if "c2" in out:
        c2, c5 = out["c2"], out["c5"]
        b2 = c2["roofline"]["bytes_per_iter"]
        rf.update({"sinkhorn_c2_it_s": c2["sinkhorn_iters_per_s"],
                   "sinkhorn_c2_streaming_it_s": c2["sinkhorn_iters_per_s_matrix_streaming"],
                   "sinkhorn_c2_streaming_gbs": b2 * c2["sinkhorn_iters_per_s_matrix_streaming"] / 1e9,
                   "sinkhorn_c2_streaming_frac": b2 * c2["sinkhorn_iters_per_s_matrix_streaming"] / 1e9 / HBM_PEAK_GBS,
                   "sinkhorn_c2_windows_spread": c2["spread_rel"],
                   "sinkhorn_c5_it_s": c5["sinkhorn_iters_per_s"], "sinkhorn_c5_gbs": c5["roofline"]["achieved"],
                   "sinkhorn_c5_frac": c5["roofline"]["frac"], "sinkhorn_c5_windows_spread": c5["spread_rel"],
                   "dopri5_ms": c5["dopri5_ms"], "dopri5_us_per_nfe": 1e3 * c5["dopri5_ms"] / max(1, c5["nfe"]),
                   "c1_solve_ms": out["c1"]["solve_ms"], "c1_sample_plan_ms": out["c1"]["sample_plan_ms"],
                   "transport_127x128_ms": out["aux"].get("transport_127x128_ms"),
                   "unbalanced_it_s": out["aux"].get("unbalanced_iters_per_s"),
                   "partial_it_s": out["aux"].get("partial_iters_per_s")})
        out["config"].update({"sinkhorn_c2": c2["config"], "sinkhorn_c5": c5["config"],
                              "c1": "B=256, d=2 exact OT (8gaussians -> moons)"})
    if args.full and world == 1 and not args.no_cpu_baseline:
        cb = cpu_baseline(B, d)
        out["cpu_baseline"] = cb
        # the per-config CPU figures next to the GPU ones they belong to
        if isinstance(cb.get("c1"), dict) and "c1" in out:
            out["c1"].update({k: v for k, v in cb["c1"].items() if k.startswith("cpu_")})
        skc = cb.get("sinkhorn_cpu") or {}
        if "c2" in out and isinstance(skc.get("c2_knopp"), dict):
            out["c2"]["cpu_iters_per_s"] = skc["c2_knopp"]["iters_per_s"]
        if "c5" in out and isinstance(skc.get("c5_knopp"), dict):
            out["c5"]["cpu_iters_per_s"] = skc["c5_knopp"]["iters_per_s"]
        out["parity"] = parity_leg(dev, ot)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
