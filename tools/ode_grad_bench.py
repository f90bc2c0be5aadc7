"""Training-through-the-sampler timings on the GPU (measurement tool; bench.py is the headline).

    python tools/ode_grad_bench.py [--repeats 9] [--batch 20] [--out FILE]

One call = one ``DifferentiableNeuralODE.trajectory`` + a loss on ``traj[-1]`` + ``backward`` at the shape of the
reference's 2-D tutorials (examples/2D_tutorials/Flow_matching_tutorial.ipynb: d = 2, w = 64, 100 steps on
linspace(0, 1, 101)), at B = 256 and B = 4096, for ``euler``, ``midpoint`` and ``rk4``.  Two paths on the same GPU,
alternating region by region (the method of tools/cnf_train_bench.py):
  hip     : forward cfm_ode_fixed_mlp_f32, backward cfm_ode_fixed_grad_f32;
  generic : the same recurrence in differentiable torch ops, one MLP call per stage, autograd through all of them: the
            fused small-field path switched off.  It is all the library could do before the gradient kernel existed.
A call on the hip path is too short a window for a host clock, so a hip region is --batch calls back to back, as a
training loop issues them, behind ONE device synchronise, and its figure is the region's time divided by --batch: time
per call in a stream of calls, host included.  A generic region is one call.  After --warmup regions of each path the
figure is the median of --repeats regions (min and max are printed with it).  The gradients of the two paths on the
timed inputs are compared (max|g_hip - g_generic| / max|g_generic| over all parameter tensors) so that the figures are
of the same result.  No GPU, no figure: the tool raises.
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

import torch  # noqa: E402


def run_case(solver, B, d, w, steps, repeats, warmup, batch, dev):
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd.utils import torch_wrapper
    lib = _lib.load()
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    x = torch.randn(B, d, device=dev)
    target = torch.randn(B, d, device=dev)
    ts = torch.linspace(0, 1, steps + 1)
    node = cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver=solver)
    params = list(m.parameters())

    def region(fused):
        calls = batch if fused else 1
        lib.cfm_ode_set_fused(1 if fused else 0)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                for p in params:
                    p.grad = None
                loss = ((node.trajectory(x, ts)[-1] - target) ** 2).mean()
                loss.backward()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / calls
        finally:
            lib.cfm_ode_set_fused(1)
        assert node.last_path == ("hip" if fused else "generic"), node.last_path
        return ms, float(loss.detach()), [p.grad.detach().clone() for p in params]

    for _ in range(warmup):
        region(True)
        region(False)
    torch.cuda.synchronize()
    hip, gen = [], []
    for _ in range(repeats):                      # alternating: both paths see the same neighbours on the machine
        a = region(True)
        b = region(False)
        hip.append(a[0])
        gen.append(b[0])
    err = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(a[2], b[2]))
    h, g = statistics.median(hip), statistics.median(gen)
    return dict(case=f"ode_grad_{solver}_B{B}", B=B, d=d, w=w, steps=steps, solver=solver,
                hip_ms=round(h, 3), hip_min_max=[round(min(hip), 3), round(max(hip), 3)],
                generic_ms=round(g, 2), generic_min_max=[round(min(gen), 2), round(max(gen), 2)],
                x_generic=round(g / h, 1), loss_hip=a[1], loss_generic=b[1], grad_rel_diff=err,
                repeats=repeats, warmup=warmup, hip_calls_per_region=batch,
                what="ms per trajectory + loss + backward; hip: regions of hip_calls_per_region calls behind one "
                     "synchronise, divided; generic: one call per region; host clock, median of alternating regions")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="hip calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ode_grad_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []
    for B in (256, 4096):
        for solver in ("euler", "midpoint", "rk4"):
            r = run_case(solver, B, 2, 64, 100, a.repeats, a.warmup, a.batch, dev)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
