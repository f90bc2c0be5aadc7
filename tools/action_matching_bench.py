"""Action-matching training step timings on the GPU (measurement tool; bench.py is the headline).

    python tools/action_matching_bench.py [--repeats 9] [--warmup 2] [--batch 20] [--out FILE]

One call = one ``cfm_amd.action_matching_loss`` + ``backward`` at the 2-D tutorial shape: B = 256, d = 2, w = 64
(``GradModel(MLP(dim=2, out_dim=1, time_varying=True))``, the model of examples/2D_tutorials/model-comparison-plotting.ipynb).
Two paths on the same GPU, alternating region by region:
  hip     : one cfm_action_matching_grad_f32 call (loss and all parameter gradients), plus the interpolant in torch ops;
  generic : the reference's formulation in differentiable torch ops (a double backward through autograd): the fused
            small-field path switched off.  It is what the library did before the kernel existed.
A region is --batch calls back to back, as a training loop issues them, behind ONE device synchronise; its figure is
the region's time divided by --batch: time per call in a stream of calls, host included.  After --warmup regions of
each path the figure is the median of --repeats regions (min and max are printed with it).  The gradients of the two
paths on the timed inputs are compared (max|g_hip - g_generic| / max|g_generic| over the parameter tensors) so that the
figures are of the same result.
Not measured: the kernel's time apart from the call (no profiler run), LDS bank conflicts (no counter run).
No GPU, no figure: the tool raises.
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


def run_case(B, d, w, repeats, warmup, batch, dev):
    import cfm_amd
    from cfm_amd import _lib
    lib = _lib.load()
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=d, out_dim=1, w=w, time_varying=True).to(dev)
    x0 = 1.5 * torch.randn(B, d, device=dev)
    x1 = 0.5 + torch.randn(B, d, device=dev)
    t = torch.rand(B, device=dev)
    params = list(m.parameters())

    def region(fused):
        lib.cfm_ode_set_fused(1 if fused else 0)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batch):
                for p in params:
                    p.grad = None
                loss = cfm_amd.action_matching_loss(m, x0, x1, t)
                loss.backward()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / batch
        finally:
            lib.cfm_ode_set_fused(1)
        path = cfm_amd.action_matching_loss.last_path
        assert path == ("hip" if fused else "generic"), path
        return ms, float(loss.detach()), [None if p.grad is None else p.grad.detach().clone() for p in params]

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
    err = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(a[2], b[2]) if q is not None)
    h, g = statistics.median(hip), statistics.median(gen)
    return dict(case="action_matching_train", B=B, d=d, w=w,
                hip_ms=round(h, 4), hip_min_max=[round(min(hip), 4), round(max(hip), 4)],
                generic_ms=round(g, 3), generic_min_max=[round(min(gen), 3), round(max(gen), 3)],
                x_generic=round(g / h, 1), loss_hip=a[1], loss_generic=b[1], grad_rel_diff=err,
                repeats=repeats, warmup=warmup, calls_per_region=batch,
                what="ms per loss + backward; regions of calls_per_region calls behind one synchronise, divided; host "
                     "clock, median of alternating regions; not measured: kernel time apart from the call, LDS bank "
                     "conflicts")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("action_matching_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    r = run_case(256, 2, 64, a.repeats, a.warmup, a.batch, dev)
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/action_matching_bench.py   (MI355X; action matching: MLP(dim=2, out_dim=1, w=64, "
                    "time_varying=True), B = 256)\n")
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
