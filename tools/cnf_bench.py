"""CNF density evaluation timings on the GPU: one JSON line per case (measurement tool; bench.py is the headline).

    python tools/cnf_bench.py [--repeats 7] [--out FILE]

Cases (the reference's density evaluations, examples/2D_tutorials/):
  mc_exact / mc_hutch : model-comparison-plotting.ipynb cells 4 / 7 — B = 10 000 grid points, d = 2, w = 64, Euler on
                        linspace(1, 0, 201); exact trace and Rademacher Hutchinson.
  mlcnf_exact         : Maximum_likelihood_CNF_tutorial.ipynb cell 4 — B = 256, d = 2, Euler on 101 points.
  c5_hutch / c5_exact : C5-shaped field (51-64-64-64-50), B = 8192, dopri5 atol = rtol = 1e-5 on [1, 0] (exact: reported
                        only).
Every time is device-synchronised, after warm-up, the median of --repeats runs.  Per case:
  ms, nfe, n_steps; plain_ms and x_plain (the plain trajectory of the same field and t_span: torch_wrapper(MLP));
  generic_ms and x_generic (the generic path on the same GPU: host-stepped stages, torch.func divergence; measured on a
  shortened grid and scaled per evaluation, see generic_basis); algorithmic GFLOP and TF/s against the 157.3 TF
  fp32-MFMA peak (these solves are latency bound, like the plain solver).
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

PEAK_TF = 157.3


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def flops_per_eval_row(d, w, estimator):
    primal = 2 * ((d + 1) * w + 2 * w * w + w * d)
    if estimator == "exact":
        tangent = d * (2 * 2 * w * w + 2 * w)          # per direction: W1, W2 products, the W3 row dot product
    else:
        tangent = 2 * (d * w + 2 * w * w + w * d) + 2 * d
    return primal + tangent


def run_case(name, d, w, B, solver, ts, estimator, repeats, dev, note=""):
    import cfm_amd
    from cfm_amd.ode import NeuralODE

    class FuncCNF(cfm_amd.CNF):
        """The CNF evaluated by torch.func only (the generic baseline): no field is handed to the kernels."""

        def hip_mlp(self, d):
            return None

    from cfm_amd.utils import torch_wrapper
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    x = torch.randn(B, d, device=dev)
    aug = torch.cat([torch.zeros(B, 1, device=dev), x], 1)
    eps = None if estimator == "exact" else torch.randint(0, 2, (B, d), device=dev).float() * 2 - 1
    tol = 1e-5
    node = NeuralODE(cfm_amd.CNF(m, estimator=estimator, noise=eps), solver=solver, atol=tol, rtol=tol)
    ms = timed(lambda: node.trajectory(aug, ts), repeats)
    assert node.last_path == "hip", node.last_path
    nfe, steps = node.nfe, node.n_steps
    plain = NeuralODE(torch_wrapper(m), solver=solver, atol=tol, rtol=tol)
    plain_ms = timed(lambda: plain.trajectory(x, ts), repeats)
    # generic path: the same CNF with the kernels out of the picture (no HIP attempt per evaluation) -> host-stepped
    # stages + torch.func divergence
    gnode = NeuralODE(FuncCNF(m, estimator=estimator, noise=eps), solver="euler")
    short = torch.linspace(float(ts[0]), float(ts[-1]), 6)
    g_ms = timed(lambda: gnode.trajectory(aug, short), 3, warmup=1)
    assert gnode.last_path == "generic"
    per_eval = g_ms / gnode.nfe
    generic_ms = per_eval * nfe
    gflop = flops_per_eval_row(d, w, estimator) * B * nfe / 1e9
    tfs = gflop / ms
    return dict(case=name, B=B, d=d, w=w, solver=solver, t_span=[float(ts[0]), float(ts[-1]), int(len(ts))],
                estimator=estimator, ms=round(ms, 3), nfe=nfe, n_steps=steps, plain_ms=round(plain_ms, 3),
                x_plain=round(ms / plain_ms, 2), generic_ms=round(generic_ms, 1), x_generic=round(generic_ms / ms, 1),
                generic_basis=f"{round(per_eval, 3)} ms per evaluation (Euler, 5 steps) x nfe",
                gflop=round(gflop, 2), tflops=round(tfs, 3), pct_peak=round(100 * tfs / PEAK_TF, 2),
                bound="latency (one persistent launch; GEMMs of 16 x 64 x 64)", note=note)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="mc_exact,mc_hutch,mlcnf_exact,c5_hutch,c5_exact")
    a = ap.parse_args(argv)
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cases = {
        "mc_exact": (2, 64, 10000, "euler", torch.linspace(1, 0, 201), "exact", ""),
        "mc_hutch": (2, 64, 10000, "euler", torch.linspace(1, 0, 201), "hutch_rademacher", ""),
        "mlcnf_exact": (2, 64, 256, "euler", torch.linspace(1, 0, 101), "exact", ""),
        "c5_hutch": (50, 64, 8192, "dopri5", torch.tensor([1.0, 0.0]), "hutch_rademacher", ""),
        "c5_exact": (50, 64, 8192, "dopri5", torch.tensor([1.0, 0.0]), "exact", "reported only"),
    }
    rows = []
    for name in a.cases.split(","):
        r = run_case(name, *cases[name][:6], a.repeats, dev, note=cases[name][6])
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:                                   # the lines as one JSON list
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
