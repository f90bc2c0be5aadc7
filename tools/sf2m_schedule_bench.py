"""Noise schedules sigma(t) for SF2M: three timings on the GPU (measurement tool; bench.py is the headline).

    python tools/sf2m_schedule_bench.py [--repeats 7] [--warmup 2] [--out profiles/sf2m_schedule.txt]

  matcher : ScheduledBridgeConditionalFlowMatcher(LinearDecreasingNoiseScheduler(0.1, 1.0)) at B = 4096, d = 100, one
            sample_location_and_conditional_flow call on the fused kernel against the same class on its eager
            composition on the same GPU (a subclass that restates one closed form: the path every customised matcher
            takes), without a coupling and with the exact one (the solve is in both figures).
  sampler : sdeint(method="euler") at B = 2048, d = 2, two 3-64-64-64-2 fields, ts = [0, 1], dt = 0.01 (100 steps),
            Philox noise — with the schedule, with a constant sigma (same kernel; the ratio is reported), with the
            schedule behind a plain callable (its values are evaluated in every call), and with the
            schedule on the eager stepping path the call took before schedules reached the kernels (the same f / g
            behind an object the fast test does not recognise).
A region is --batch calls back to back behind ONE device synchronise, its figure the region's time over --batch: time
per call in a stream of calls, host included.  After --warmup regions of each path: the median of --repeats
alternating regions, with min and max.  Kernel time alone and other shapes are NOT measured.  No GPU, no figure.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _region(fn, batch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batch):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / batch


def _alternate(paths, batch, repeats, warmup):
    """{name: (median, min, max)} ms per call over alternating regions"""
    for _ in range(warmup):
        for fn in paths.values():
            _region(fn, batch)
    ms = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            ms[k].append(_region(fn, batch))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def _row(name, r):
    return f"{name:34s} {r[0]:9.4f} {r[1]:9.4f} {r[2]:9.4f}"


def matcher(dev, repeats, warmup):
    import cfm_amd

    class Restated(cfm_amd.ScheduledBridgeConditionalFlowMatcher):
        def compute_sigma_t(self, t):
            return self.schedule.sigma_t(t)
    B, d = 4096, 100
    g = torch.Generator().manual_seed(0)
    x0, x1 = torch.randn(B, d, generator=g).to(dev), (torch.randn(B, d, generator=g) + 1.0).to(dev)
    lines = [f"# matcher: one sample_location_and_conditional_flow call, B = {B}, d = {d}, LinearDecreasing(0.1, 1.0); ms per call",
             f"{'path':34s} {'median':>9s} {'min':>9s} {'max':>9s}"]
    for coupled in (False, True):
        mk = lambda cls: cls(cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0))
        hip, eager = mk(cfm_amd.ScheduledBridgeConditionalFlowMatcher), mk(Restated)
        if coupled:
            call = lambda fm: (lambda: fm.sample_location_and_conditional_flow(x0, x1))
        else:
            call = lambda fm: (lambda: fm._sample(x0, x1, None, False))
        np.random.seed(0); torch.manual_seed(0)
        tag = "exact coupling" if coupled else "no coupling"
        r = _alternate({"hip": call(hip), "eager": call(eager)}, 10 if coupled else 50, repeats, warmup)
        lines.append(_row(f"{tag}: fused kernel", r["hip"]))
        lines.append(_row(f"{tag}: eager composition", r["eager"]))
        lines.append(f"{tag}: eager / fused = {r['eager'][0] / r['hip'][0]:.2f}")
    return lines


def sampler(dev, repeats, warmup):
    import cfm_amd
    import cfm_oracle as oracle
    from cfm_amd.sde import FlowScoreSDE, sdeint
    torch.manual_seed(0)
    f = cfm_amd.MLP(dim=2, time_varying=True, w=64).to(dev)
    sc = cfm_amd.MLP(dim=2, time_varying=True, w=64).to(dev)
    x0, _ = oracle.config_inputs("C1", B=2048)
    y0, ts = x0.to(dev), torch.linspace(0, 1, 2)
    schedule = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    sched, const = FlowScoreSDE(f, sc, sigma=schedule), FlowScoreSDE(f, sc, sigma=0.1)

    class Generic:                       # the same f and g behind an object sdeint steps in eager torch
        noise_type, sde_type = "diagonal", "ito"
        f, g = sched.f, sched.g
    plain = FlowScoreSDE(f, sc, sigma=lambda t: schedule(t))      # any callable: g(t_k) is evaluated in every call
    paths = {"sched": lambda: sdeint(sched, y0, ts, dt=0.01, fused=True),
             "const": lambda: sdeint(const, y0, ts, dt=0.01, fused=True),
             "plain": lambda: sdeint(plain, y0, ts, dt=0.01, fused=True)}
    r = _alternate(paths, 50, repeats, warmup)
    assert sched.last_path == "hip" and plain.last_path == "hip"
    e = _alternate({"sched": paths["sched"], "eager": lambda: sdeint(Generic(), y0, ts, dt=0.01)}, 3, repeats, warmup)
    lines = ["# sampler: sdeint(method='euler'), B = 2048, d = 2, two 3-64-64-64-2 fields, 100 steps, Philox noise; ms per call",
             f"{'path':34s} {'median':>9s} {'min':>9s} {'max':>9s}",
             _row("schedule, one launch", r["sched"]),
             _row("constant sigma, one launch", r["const"]),
             f"schedule / constant = {r['sched'][0] / r['const'][0]:.3f}  (same kernel; g(t_k) of a built-in schedule is kept per grid)",
             _row("any callable, one launch", r["plain"]),
             f"callable / constant = {r['plain'][0] / r['const'][0]:.3f}  (same kernel; 100 host evaluations of g per call)",
             _row("schedule, one launch (2nd run)", e["sched"]),
             _row("schedule, eager stepping path", e["eager"]),
             f"eager stepping / one launch = {e['eager'][0] / e['sched'][0]:.1f}"]
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sf2m_schedule_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = [f"# regions of calls behind one synchronise, divided; host clock, host included; median / min / max of "
             f"{a.repeats} alternating regions after {a.warmup} warm-up regions; kernel time alone and other shapes: not measured"]
    lines += matcher(dev, a.repeats, a.warmup) + sampler(dev, a.repeats, a.warmup)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
