"""Regularised CNF training step timings on the GPU (measurement tool; bench.py is the headline).

    python tools/cnf_reg_bench.py [--repeats 9] [--batch 20] [--out FILE]

One call = one loss + ``backward`` at the shape of tools/cnf_train_bench.py (B = 256, d = 2, w = 64, 100 Euler steps on
linspace(1, 0, 101), exact trace), for four penalty settings in one run:
  none : ``DifferentiableCNF.nll`` (cfm_ode_fixed_cnf_mlp_f32 + cfm_cnf_euler_grad_f32): what each penalty is added to;
  e    : ``RegularizedCNF(squared_l2_reg=0.01).loss``, reg + nll;
  f    : ``RegularizedCNF(jacobian_frobenius_reg=0.01).loss``;
  ef   : both.
Two paths on the same GPU, alternating region by region, on the protocol of cnf_train_bench.py:
  hip     : cfm_ode_euler_cnf_reg_mlp_f32 forward, cfm_cnf_reg_euler_grad_f32 backward; a region is --batch calls back to
            back behind ONE device synchronise, its figure the region's time divided by --batch (host included);
  generic : the same recurrence in differentiable torch ops (the fused small-field path switched off): all a user had
            before these kernels.  A region is one call.
After --warmup regions of each path the figure is the median of --repeats regions (min and max are printed with it).  The
gradients of the two paths on the timed inputs are compared so that the figures are of the same result.
Not measured: kernel time apart from the call, LDS bank conflicts, other shapes.  No GPU, no figure: the tool raises.
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

SETTINGS = {"none": (0.0, 0.0), "e": (0.01, 0.0), "f": (0.0, 0.01), "ef": (0.01, 0.01)}


def run_case(name, B, d, w, steps, repeats, warmup, batch, dev):
    import cfm_amd
    from cfm_amd import _lib
    lib = _lib.load()
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    x = torch.randn(B, d, device=dev)
    ce, cf = SETTINGS[name]
    cnf = cfm_amd.DifferentiableCNF(m) if name == "none" else cfm_amd.RegularizedCNF(m, squared_l2_reg=ce, jacobian_frobenius_reg=cf)
    params = list(m.parameters())

    def one_loss():
        if name == "none":
            return cnf.nll(x, steps=steps)
        reg, nll = cnf.loss(x, steps=steps)
        return reg + nll

    def region(fused):
        calls = batch if fused else 1
        lib.cfm_ode_set_fused(1 if fused else 0)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                for p in params:
                    p.grad = None
                loss = one_loss()
                loss.backward()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / calls
        finally:
            lib.cfm_ode_set_fused(1)
        assert cnf.last_path == ("hip" if fused else "generic"), cnf.last_path
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
    return dict(case=f"cnf_reg_{name}", B=B, d=d, w=w, steps=steps, penalties=name,
                hip_ms=round(h, 3), hip_min_max=[round(min(hip), 3), round(max(hip), 3)],
                generic_ms=round(g, 2), generic_min_max=[round(min(gen), 2), round(max(gen), 2)],
                x_generic=round(g / h, 1), loss_hip=a[1], loss_generic=b[1], grad_rel_diff=err,
                repeats=repeats, warmup=warmup, hip_calls_per_region=batch,
                what="ms per loss + backward; hip: regions of hip_calls_per_region calls behind one synchronise, divided; "
                     "generic: one call per region; host clock, median of alternating regions")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="hip calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cnf_reg_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []
    for name in SETTINGS:
        r = run_case(name, 256, 2, 64, 100, a.repeats, a.warmup, a.batch, dev)
        if rows:
            r["x_none_hip"] = round(r["hip_ms"] / rows[0]["hip_ms"], 2)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
