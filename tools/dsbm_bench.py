"""DSBM (diffusion Schrodinger bridge matching): five timings on the GPU (measurement tool; bench.py is the headline).

    python tools/dsbm_bench.py [--repeats 7] [--warmup 2] [--out profiles/dsbm.txt]

  matcher : DSBMConditionalFlowMatcher(LinearDecreasingNoiseScheduler(0.1, 1.0)) at B = 4096, d = 100, no coupling, one
            sample_location_and_targets call on the fused kernel against the same class on its eager composition on the
            same GPU (a subclass that restates one closed form: the path every customised matcher takes).
  step    : DSBMStep against SF2MStep at B = 4096, d = 100, w = 64 in the same run (the same launches: about the same time
            is expected; the ratio is recorded, not asserted), and DSBMStep against the torch-ops autograd formulation
            (two MLPs on the PyTorch-ROCm path, torch.optim.Adam) at B = 256, d = 2, w = 64.  Each figure is forward, both
            losses, backward and the Adam update of both nets.
  odeint  : DSBMFlowSolver.odeint, euler, 101 points at B = 1024, d = 2, w = 64: the pair kernel against fused=False.
  sdeint  : single-field DSBMFlowSolver.sdeint, 100 steps at B = 2048, d = 2, w = 64, Philox noise, against the two-field
            FlowScoreSDE call on the same kernel.
A region is 20 calls back to back behind ONE device synchronise, its figure the region's time over 20: time per call in a
stream of calls, host included.  After --warmup regions of each path: the median of --repeats alternating regions, with
min and max.  Kernel time alone, LDS bank conflicts and other shapes are NOT measured.  No GPU, no figure.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

BATCH = 20


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
    return f"{name:44s} {r[0]:9.4f} {r[1]:9.4f} {r[2]:9.4f}"


HEAD = f"{'path':44s} {'median':>9s} {'min':>9s} {'max':>9s}"


def matcher(dev, repeats, warmup):
    import cfm_amd

    class Restated(cfm_amd.DSBMConditionalFlowMatcher):
        def compute_sigma_t(self, t):
            return self.schedule.sigma_t(t)
    B, d = 4096, 100
    g = torch.Generator().manual_seed(0)
    x0, x1 = torch.randn(B, d, generator=g).to(dev), (torch.randn(B, d, generator=g) + 1.0).to(dev)
    sched = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    hip, eager = cfm_amd.DSBMConditionalFlowMatcher(sched), Restated(sched)
    torch.manual_seed(0)
    r = _alternate({"hip": lambda: hip.sample_location_and_targets(x0, x1),
                    "eager": lambda: eager.sample_location_and_targets(x0, x1)}, BATCH, repeats, warmup)
    return [f"# matcher: one sample_location_and_targets call, B = {B}, d = {d}, LinearDecreasing(0.1, 1.0), no coupling; ms per call",
            HEAD, _row("fused kernel", r["hip"]), _row("eager composition", r["eager"]),
            f"eager / fused = {r['eager'][0] / r['hip'][0]:.2f}"]


def _batch(dev, B, d):
    g = torch.Generator().manual_seed(1)
    t = (0.05 + 0.9 * torch.rand(B, generator=g)).to(dev)
    xt, a, b = (torch.randn(B, d, generator=g).to(dev) for _ in range(3))
    fs, bs = (1 + t / (1 - t + 1e-6)) ** -1, (1 + (1 - t) / (t + 1e-6)) ** -1
    return t, xt, a, b, fs, bs


def step(dev, repeats, warmup):
    import cfm_amd
    lines = []
    # against SF2MStep: the same driver, the same launches
    B, d, w = 4096, 100, 64
    torch.manual_seed(0)
    nets = [cfm_amd.MLP(dim=d, w=w, time_varying=True).to(dev) for _ in range(4)]
    t, xt, a, b, fs, bs = _batch(dev, B, d)
    lam = 2 * torch.sqrt(t * (1 - t))
    dsbm = cfm_amd.DSBMStep(nets[0], nets[1], cfm_amd.FusedAdam([p for n in nets[:2] for p in n.parameters()], lr=1e-3))
    sf2m = cfm_amd.SF2MStep(nets[2], nets[3], cfm_amd.FusedAdam([p for n in nets[2:] for p in n.parameters()], lr=1e-3))
    r = _alternate({"dsbm": lambda: dsbm(t, xt, a, b, fs, bs), "sf2m": lambda: sf2m(t, xt, a, b, lam)}, BATCH, repeats, warmup)
    lines += [f"# step: forward + both losses + backward + Adam of two {d + 1}-{w}-{w}-{w}-{d} nets, B = {B}; ms per call", HEAD,
              _row("DSBMStep", r["dsbm"]), _row("SF2MStep", r["sf2m"]), f"DSBMStep / SF2MStep = {r['dsbm'][0] / r['sf2m'][0]:.3f}"]
    # against the torch-ops autograd formulation
    B, d, w = 256, 2, 64
    torch.manual_seed(0)
    nets = [cfm_amd.MLP(dim=d, w=w, time_varying=True).to(dev) for _ in range(4)]
    for n in nets[2:]:
        n.hip_training = False                                   # PyTorch-ROCm ops end to end
    t, xt, a, b, fs, bs = _batch(dev, B, d)
    dsbm = cfm_amd.DSBMStep(nets[0], nets[1], cfm_amd.FusedAdam([p for n in nets[:2] for p in n.parameters()], lr=1e-3))
    opt = torch.optim.Adam([p for n in nets[2:] for p in n.parameters()], lr=1e-3)

    def autograd():
        opt.zero_grad()
        x = torch.cat([xt, t[:, None]], dim=-1)
        fl = torch.mean(fs[:, None] * (nets[2](x) - a) ** 2)
        bl = torch.mean(bs[:, None] * (nets[3](x) - b) ** 2)
        (fl + bl).backward()
        opt.step()
    r = _alternate({"dsbm": lambda: dsbm(t, xt, a, b, fs, bs), "autograd": autograd}, BATCH, repeats, warmup)
    lines += [f"# step: the same at B = {B}, two {d + 1}-{w}-{w}-{w}-{d} nets, against torch ops + autograd + torch.optim.Adam; ms per call",
              HEAD, _row("DSBMStep", r["dsbm"]), _row("torch ops, autograd", r["autograd"]),
              f"autograd / DSBMStep = {r['autograd'][0] / r['dsbm'][0]:.2f}"]
    return lines


def samplers(dev, repeats, warmup):
    import cfm_amd
    from cfm_amd.sde import FlowScoreSDE, sdeint
    from cfm_amd.utils import torch_wrapper
    torch.manual_seed(0)
    f, b = (cfm_amd.MLP(dim=2, w=64, time_varying=True).to(dev) for _ in range(2))
    sched = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    s = cfm_amd.DSBMFlowSolver(torch_wrapper(f), 2, score_field=torch_wrapper(b), sigma=sched, ode_solver="euler", dt=0.01)
    x = torch.randn(1024, 2, device=dev)
    ts = torch.linspace(0, 1, 101)
    r = _alternate({"fused": lambda: s.odeint(x, ts), "stages": lambda: s.odeint(x, ts, fused=False)}, BATCH, repeats, warmup)
    assert s.last_path == "hip"
    lines = ["# odeint: euler, 101 points, B = 1024, d = 2, two 3-64-64-64-2 nets; ms per call", HEAD,
             _row("pair kernel, one launch", r["fused"]), _row("fused=False, launch per stage", r["stages"]),
             f"launch per stage / one launch = {r['stages'][0] / r['fused'][0]:.1f}"]
    y = torch.randn(2048, 2, device=dev)
    t2 = torch.linspace(0, 1, 2)
    two = FlowScoreSDE(f, b, sigma=sched)
    r = _alternate({"one": lambda: s.sdeint(y, t2), "two": lambda: sdeint(two, y, t2, dt=0.01)}, BATCH, repeats, warmup)
    assert s.last_path == "hip" and two.last_path == "hip"
    lines += ["# sdeint: euler, 100 steps, B = 2048, d = 2, 3-64-64-64-2 nets, Philox noise, one launch; ms per call", HEAD,
              _row("single field (DSBMFlowSolver)", r["one"]), _row("two fields (FlowScoreSDE)", r["two"]),
              f"single / two fields = {r['one'][0] / r['two'][0]:.3f}"]
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dsbm_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = [f"# regions of {BATCH} calls behind one synchronise, divided; host clock, host included; median / min / max of "
             f"{a.repeats} alternating regions after {a.warmup} warm-up regions; kernel time alone, LDS bank conflicts and "
             f"other shapes: not measured"]
    lines += matcher(dev, a.repeats, a.warmup) + step(dev, a.repeats, a.warmup) + samplers(dev, a.repeats, a.warmup)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
