"""Multi-marginal flow matching: time per call of TrajectoryFlowMatcher.sample_location_and_conditional_flow on the GPU
(measurement tool; bench.py is the headline).

    python tools/trajectory_bench.py [--repeats 9] [--warmup 2] [--batch 20] [--out FILE]

Shapes X [B, T, d]: (256, 5, 5), (256, 5, 100), (4096, 5, 100); interpolant linear and spline; with an exact coupling
(ExactOptimalTransportConditionalFlowMatcher) and without (ConditionalFlowMatcher); sigma = 0.1; training calls.
  new      : one TrajectoryFlowMatcher call (couplings of the call solved together, then one cfm_traj_xt_ut_f32 launch).
  baseline : linear — the per-interval loop over the public matcher calls the library had before (the single-cell
             notebook's form: one sample_location_and_conditional_flow per interval, then the per-row select of the
             row's interval in torch ops); spline — the same TrajectoryFlowMatcher call on its eager path on the same GPU
             (the path is forced by the knob the class uses itself: MAX_FUSED_KNOTS = 0).
A call is too short a window for a host clock, so a region is --batch calls back to back behind ONE device synchronise
and its figure is the region's time divided by --batch: time per call in a stream of calls, host included
(tools/cnf_train_bench.py's form).  After --warmup regions of each path the figure is the median of --repeats
alternating regions, with min and max.  The launches of one call of each path are counted with torch.profiler (kernel
events of one call after the timed regions) and listed by name.  No GPU, no figure: the tool raises.
"""
import argparse
import json
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


def _kernels_of(fn):
    """kernel launches of one call: {name: count}"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            name = e.name.split("(")[0].split("<")[0].replace("void ", "")
            out[name] = out.get(name, 0) + 1
    return out


def run_case(interp, coupled, B, T, d, repeats, warmup, batch, dev):
    import cfm_amd
    import cfm_amd.trajectory as tj
    sigma = 0.1
    g = torch.Generator().manual_seed(0)
    X = (torch.randn(B, T, d, generator=g) + 0.5 * torch.arange(T)[None, :, None]).to(dev)
    mk = (lambda: cfm_amd.ExactOptimalTransportConditionalFlowMatcher(sigma)) if coupled else \
         (lambda: cfm_amd.ConditionalFlowMatcher(sigma))
    tfm = cfm_amd.TrajectoryFlowMatcher(mk(), interp)
    fm = mk()
    rb = torch.arange(B, device=dev)

    def new():
        out = tfm.sample_location_and_conditional_flow(X)
        assert tfm.last_path == "hip", tfm.last_path
        return out

    def loop():          # the parent's interface: one public call per interval, then each row takes its interval
        ts = torch.randint(T - 1, size=(B,)).to(dev)
        t = torch.rand(B).to(dev)
        outs = [fm.sample_location_and_conditional_flow(X[:, k], X[:, k + 1], t=t) for k in range(T - 1)]
        xt = torch.stack([o[1] for o in outs])[ts, rb]
        ut = torch.stack([o[2] for o in outs])[ts, rb]
        return t + ts, xt, ut

    def eager():
        keep = tj.MAX_FUSED_KNOTS
        tj.MAX_FUSED_KNOTS = 0
        try:
            out = tfm.sample_location_and_conditional_flow(X)
        finally:
            tj.MAX_FUSED_KNOTS = keep
        assert tfm.last_path == "eager", tfm.last_path
        return out

    base = loop if interp == "linear" else eager

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batch

    np.random.seed(0); torch.manual_seed(0)
    for _ in range(warmup):
        region(new)
        region(base)
    a, b = [], []
    for _ in range(repeats):                     # alternating: both paths see the same neighbours on the machine
        a.append(region(new))
        b.append(region(base))
    try:
        kn, kb = _kernels_of(new), _kernels_of(base)
    except Exception as e:                       # a box without a working tracer still gives the timings
        kn, kb = {"profiler_failed: " + type(e).__name__: 0}, {}
    ma, mb = statistics.median(a), statistics.median(b)
    return dict(case=f"trajectory_{interp}_{'exact' if coupled else 'none'}", interpolant=interp,
                coupling="exact" if coupled else "none", B=B, T=T, d=d,
                new_ms=round(ma, 4), new_min_max=[round(min(a), 4), round(max(a), 4)],
                baseline="per_interval_public_calls" if interp == "linear" else "eager_path_same_gpu",
                baseline_ms=round(mb, 4), baseline_min_max=[round(min(b), 4), round(max(b), 4)],
                baseline_over_new=round(mb / ma, 2),
                new_launches=sum(kn.values()), new_traj_launches=sum(v for k, v in kn.items() if "traj_" in k),
                baseline_launches=sum(kb.values()), new_kernels=kn,
                repeats=repeats, warmup=warmup, calls_per_region=batch,
                what="ms per call; regions of calls_per_region calls behind one synchronise, divided; host clock, host "
                     "included; median of alternating regions; launches: kernel events of one call (torch.profiler)")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []
    for B, T, d in ((256, 5, 5), (256, 5, 100), (4096, 5, 100)):
        for interp in ("linear", "spline"):
            for coupled in (False, True):
                r = run_case(interp, coupled, B, T, d, a.repeats, a.warmup, a.batch, dev)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
