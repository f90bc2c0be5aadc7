"""Action-matching (GradModel) sampling and density timings on the GPU (measurement tool; bench.py is the headline).

    python tools/grad_field_bench.py [--repeats 7] [--warmup 2] [--batch 20] [--out FILE]

The two solves examples/2D_tutorials/model-comparison-plotting.ipynb runs for its action-matching models
(GradModel(MLP(dim=2, out_dim=1, w=64, time_varying=True)): torchcfm/models/models.py:24-32):
  sample  : cell 4, B = 1024, Euler on linspace(0, 1, 101);
  density : cells 4 and 7, the 10 000-point grid, Euler on linspace(1, 0, 201), the augmented state with the exact trace.
Three paths per shape on the same GPU, alternating region by region:
  hip     : cfm_ode_fixed_gradmlp_f32 / cfm_ode_fixed_cnf_gradmlp_f32 (one launch per solve);
  generic : (a) what the library can do without these kernels: the fused small-field path switched off, GradModel.forward
            through autograd, stepped on the host by NeuralODE's generic path; for the density the trace comes from
            autograd's double backward, one pass per direction (the notebook's CNF + autograd_trace, restated below:
            the library's own generic CNF cannot trace a GradModel);
  mlp     : (b) the existing fused path on a plain MLP(dim=2, w=64) field at the same shape
            (cfm_ode_fixed_mlp_f32 / cfm_ode_fixed_cnf_mlp_f32).
A fused call takes well under a millisecond to a few milliseconds, too short a window for a host clock, so a hip or mlp
region is --batch calls back to back behind ONE device synchronise and its figure is the region's time divided by
--batch; a generic region is one call.  After --warmup regions of each path the figure is the median of --repeats
regions (min and max are printed with it).  us_per_eval = time per call / nfe.  The hip and generic results on the timed
inputs are compared (max|hip - generic| / max|generic| over the last frame) so that the figures are of the same result.
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


class AutogradCNF(torch.nn.Module):
    """model-comparison-plotting.ipynb cell 2 restated: [-tr(dv/dx), v] with the trace taken by one autograd pass per
    direction through the graph GradModel.forward keeps (create_graph=True)."""

    def __init__(self, grad_model):
        super().__init__()
        self.model = grad_model

    def forward(self, t, x):
        with torch.enable_grad():
            y = x[:, 1:].detach().requires_grad_(True)
            v = self.model(torch.cat([y, t.to(y.dtype).reshape(1, 1).expand(y.shape[0], 1)], 1))
            tr = 0.0
            for k in range(y.shape[1]):
                tr = tr + torch.autograd.grad(v[:, k].sum(), y, retain_graph=True)[0][:, k]
        return torch.cat([-tr[:, None], v.detach()], 1)


def run_case(name, B, n_t, augmented, repeats, warmup, batch, dev):
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd.models import GradModel
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    lib = _lib.load()
    torch.manual_seed(0)
    action = cfm_amd.MLP(dim=2, out_dim=1, w=64, time_varying=True).to(dev)
    plain = cfm_amd.MLP(dim=2, w=64, time_varying=True).to(dev)
    gm = GradModel(action)
    if augmented:
        side = int(round(B ** 0.5))
        g = torch.linspace(-4.0, 4.0, side, device=dev)
        pts = torch.stack(torch.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
        x0 = torch.cat([torch.zeros(pts.shape[0], 1, device=dev), pts], 1)
        ts = torch.linspace(1.0, 0.0, n_t)
        nodes = dict(hip=NeuralODE(cfm_amd.CNF(gm), solver="euler"), generic=NeuralODE(AutogradCNF(gm), solver="euler"),
                     mlp=NeuralODE(cfm_amd.CNF(plain), solver="euler"))
    else:
        x0 = torch.randn(B, 2, device=dev)
        ts = torch.linspace(0.0, 1.0, n_t)
        nodes = dict(hip=NeuralODE(torch_wrapper(gm), solver="euler"), generic=NeuralODE(torch_wrapper(gm), solver="euler"),
                     mlp=NeuralODE(torch_wrapper(plain), solver="euler"))
    want = dict(hip="hip", generic="generic", mlp="hip")

    def region(path):
        calls = 1 if path == "generic" else batch
        node = nodes[path]
        lib.cfm_ode_set_fused(0 if path == "generic" else 1)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                tr = node.trajectory(x0, ts)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / calls
        finally:
            lib.cfm_ode_set_fused(1)
        assert node.last_path == want[path] and node.nfe == n_t - 1, (path, node.last_path, node.nfe)
        return ms, tr[-1]

    for _ in range(warmup):
        for path in nodes:
            region(path)
    times = {path: [] for path in nodes}
    last = {}
    for _ in range(repeats):                      # alternating: the paths see the same neighbours on the machine
        for path in nodes:
            ms, last[path] = region(path)
            times[path].append(ms)
    med = {p: statistics.median(v) for p, v in times.items()}
    err = float((last["hip"] - last["generic"]).abs().max() / last["generic"].abs().max())
    nfe = n_t - 1
    return dict(case=name, B=int(x0.shape[0]), d=2, w=64, n_t=n_t, nfe=nfe, augmented=augmented,
                hip_ms=round(med["hip"], 4), hip_min_max=[round(min(times["hip"]), 4), round(max(times["hip"]), 4)],
                generic_ms=round(med["generic"], 2),
                generic_min_max=[round(min(times["generic"]), 2), round(max(times["generic"]), 2)],
                mlp_ms=round(med["mlp"], 4), mlp_min_max=[round(min(times["mlp"]), 4), round(max(times["mlp"]), 4)],
                hip_us_per_eval=round(1e3 * med["hip"] / nfe, 3), mlp_us_per_eval=round(1e3 * med["mlp"] / nfe, 3),
                generic_us_per_eval=round(1e3 * med["generic"] / nfe, 1),
                x_generic=round(med["generic"] / med["hip"], 1), x_mlp=round(med["hip"] / med["mlp"], 2),
                hip_vs_generic_rel_diff=err, repeats=repeats, warmup=warmup, fused_calls_per_region=batch,
                what="ms per solve; hip / mlp: regions of fused_calls_per_region calls behind one synchronise, divided; "
                     "generic: one call per region; host clock, median of alternating regions; x_generic = generic / "
                     "hip, x_mlp = hip / mlp (the gradient field against the plain field, same shape)")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="fused calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("grad_field_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []
    for name, B, n_t, aug in (("am_sample_euler101", 1024, 101, False), ("am_density_grid_euler201", 10000, 201, True)):
        r = run_case(name, B, n_t, aug, a.repeats, a.warmup, a.batch, dev)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
