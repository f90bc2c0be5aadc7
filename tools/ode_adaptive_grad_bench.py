"""Training through the adaptive sampler: timings on the GPU (measurement tool; bench.py is the headline).

    python tools/ode_adaptive_grad_bench.py [--repeats 9] [--batch 20] [--out FILE]

One call = one ``AdaptiveDifferentiableNeuralODE.trajectory`` + a loss on ``traj[-1]`` + ``backward`` at the shape of the
reference's 2-D tutorials (examples/2D_tutorials/Flow_matching_tutorial.ipynb: d = 2, w = 64, atol = rtol = 1e-4), at
B = 256 and B = 4096, for ``dopri5`` and ``tsit5``, on the endpoint grid [0, 1] and on linspace(0, 1, 101).  Three figures
per case on the same GPU, alternating region by region (the method of tools/ode_grad_bench.py):
  hip     : forward cfm_ode_adaptive_rec_mlp_f32, backward cfm_ode_adaptive_grad_f32;
  generic : the same loop in differentiable torch ops, one MLP call per stage, autograd through all accepted steps: the
            fused small-field path switched off.  It is all the library could do before the gradient kernel existed;
  rk4     : DifferentiableNeuralODE(rk4) on its fused path at the nearest number of field evaluations (uniform steps; on
            the 101-point grid a multiple of 100 of them, so that every grid point is a step end).
A hip or rk4 region is --batch calls back to back behind ONE device synchronise, and its figure is the region's time
divided by --batch: time per call in a stream of calls, host included (the adaptive forward itself synchronises once per
call to read its counters back).  A generic region is one call.  After --warmup regions of each path the figure is the
median of --repeats regions (min and max are printed with it).  The gradients of the hip and generic paths on the timed
inputs are compared so that the figures are of the same result; their step counts are printed (the two paths may accept
different steps where a controller ratio sits within rounding of 1).  No GPU, no figure: the tool raises.
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


def run_case(solver, B, d, w, n_t, tol, repeats, warmup, batch, dev):
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd.utils import torch_wrapper
    lib = _lib.load()
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    x = torch.randn(B, d, device=dev)
    target = torch.randn(B, d, device=dev)
    ts = torch.linspace(0, 1, n_t)
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m), solver=solver, atol=tol, rtol=tol)
    params = list(m.parameters())

    def region(nd, grid, fused, calls, path):
        lib.cfm_ode_set_fused(1 if fused else 0)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                for p in params:
                    p.grad = None
                loss = ((nd.trajectory(x, grid)[-1] - target) ** 2).mean()
                loss.backward()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / calls
        finally:
            lib.cfm_ode_set_fused(1)
        assert nd.last_path == path, nd.last_path
        return ms, float(loss.detach()), [p.grad.detach().clone() for p in params]

    a = region(node, ts, True, 1, "hip")
    nfe, acc, att = node.nfe, node.n_accepted, node.n_steps
    steps = max(1, round(nfe / 4)) if n_t == 2 else 100 * max(1, round(nfe / 400))
    rk4 = cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver="rk4")
    ts4 = torch.linspace(0, 1, steps + 1)
    for _ in range(warmup):
        region(node, ts, True, batch, "hip")
        region(rk4, ts4, True, batch, "hip")
        region(node, ts, False, 1, "generic")
    gen_acc, gen_att = node.n_accepted, node.n_steps
    torch.cuda.synchronize()
    hip, fix, gen = [], [], []
    for _ in range(repeats):                      # alternating: all paths see the same neighbours on the machine
        a = region(node, ts, True, batch, "hip")
        c = region(rk4, ts4, True, batch, "hip")
        b = region(node, ts, False, 1, "generic")
        hip.append(a[0]); fix.append(c[0]); gen.append(b[0])
    err = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(a[2], b[2]))
    h, g, f = statistics.median(hip), statistics.median(gen), statistics.median(fix)
    return dict(case=f"ode_adaptive_grad_{solver}_B{B}_nt{n_t}", B=B, d=d, w=w, n_t=n_t, solver=solver, atol=tol, rtol=tol,
                nfe=nfe, n_accepted=acc, n_steps=att, generic_n_accepted=gen_acc, generic_n_steps=gen_att,
                hip_ms=round(h, 3), hip_min_max=[round(min(hip), 3), round(max(hip), 3)],
                generic_ms=round(g, 2), generic_min_max=[round(min(gen), 2), round(max(gen), 2)],
                x_generic=round(g / h, 1),
                rk4_steps=steps, rk4_nfe=4 * steps, rk4_ms=round(f, 3), rk4_min_max=[round(min(fix), 3), round(max(fix), 3)],
                hip_over_rk4=round(h / f, 2), hip_us_per_eval=round(1e3 * h / nfe, 2), rk4_us_per_eval=round(1e3 * f / (4 * steps), 2),
                loss_hip=a[1], loss_generic=b[1], loss_rk4=c[1], grad_rel_diff=err,
                repeats=repeats, warmup=warmup, calls_per_region=batch,
                what="ms per trajectory + loss + backward; hip and rk4: regions of calls_per_region calls behind one "
                     "synchronise, divided; generic: one call per region; host clock, median of alternating regions")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="hip / rk4 calls per timed region")
    ap.add_argument("--tol", type=float, default=1e-4, help="atol = rtol")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ode_adaptive_grad_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []
    for B in (256, 4096):
        for n_t in (2, 101):
            for solver in ("dopri5", "tsit5"):
                r = run_case(solver, B, 2, 64, n_t, a.tol, a.repeats, a.warmup, a.batch, dev)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
