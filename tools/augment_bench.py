"""The augmented sampler's timings on the GPU (measurement tool; bench.py is the headline).

    python tools/augment_bench.py [--repeats 20] [--batch 20] [--out profiles/augmented_sampler.txt]

One call = ``FlowSolver(torch_wrapper(m), 2, ode_solver="euler", augmentations=AugmentationModule(l1_reg=1, l2_reg=1,
squared_l2_reg=1)).odeint(x0, linspace(0, 1, 101))`` at B = 1024, d = 2, w = 64: the runner's validation loop
(cfm_module.py:441-505), mode 2 (no trace), mask L1 | L2 | squared_L2.  Three paths in one run, alternating region by
region so that each sees the same neighbours on the machine:
  hip   : one launch of cfm_ode_euler_cnf_reg_mlp_f32; a region is --batch calls back to back behind ONE device
          synchronise, its figure the region's time divided by --batch (host included);
  plain : the un-augmented solve of the same net and grid (``NeuralODE(torch_wrapper(m), solver="euler").trajectory``: the
          fused Euler of cfm_ode_fixed_mlp_f32), the same regions: what the three integrals are added to.  The ratio is
          reported, not gated;
  eager : the augmented callable stepped in torch ops on the same GPU (the fused small-field path switched off): all a user
          had before this kernel.  A region is one call.
After --warmup regions of each path the figure is the median of --repeats regions; min and max are printed with it, and
the tool says whether hip is faster than eager by more than the two spreads together.  The last rows of the two
augmented paths are compared so that the figures are of the same result.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="hip / plain calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: no GPU, no measurement")
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, d, w, n_t = 1024, 2, 64, 101
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    x0 = torch.randn(B, d, device=dev)
    ts = torch.linspace(0, 1, n_t)
    am = cfm_amd.AugmentationModule(l1_reg=1, l2_reg=1, squared_l2_reg=1)
    aug = cfm_amd.FlowSolver(torch_wrapper(m), d, ode_solver="euler", augmentations=am)
    plain = NeuralODE(torch_wrapper(m), solver="euler")

    def region(solver, calls, fused, path):
        solve = solver.odeint if solver is aug else solver.trajectory
        lib.cfm_ode_set_fused(1 if fused else 0)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                out = solve(x0, ts)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / calls
        finally:
            lib.cfm_ode_set_fused(1)
        assert solver.last_path == path, solver.last_path
        return ms, out

    paths = {"hip": (aug, a.batch, True, "hip"), "plain": (plain, a.batch, True, "hip"), "eager": (aug, 1, False, "eager")}
    for _ in range(a.warmup):
        for v in paths.values():
            region(*v)
    times = {k: [] for k in paths}
    last = {}
    for _ in range(a.repeats):
        for k, v in paths.items():
            ms, out = region(*v)
            times[k].append(ms)
            last[k] = out
    err = float((last["hip"][1][-1] - last["eager"][1][-1]).abs().max() / last["eager"][1][-1].abs().max())
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    row = dict(case="augmented_sampler", B=B, d=d, w=w, n_t=n_t, mode=2, mask=13,
               hip_ms=round(med["hip"], 4), hip_min_max=[round(min(times["hip"]), 4), round(max(times["hip"]), 4)],
               plain_ms=round(med["plain"], 4), plain_min_max=[round(min(times["plain"]), 4), round(max(times["plain"]), 4)],
               eager_ms=round(med["eager"], 2), eager_min_max=[round(min(times["eager"]), 2), round(max(times["eager"]), 2)],
               x_plain=round(med["hip"] / med["plain"], 3), x_eager=round(med["eager"] / med["hip"], 1),
               faster_than_eager_by_more_than_the_spreads=bool(med["eager"] - med["hip"] > spread["eager"] + spread["hip"]),
               aug_rel_diff_hip_eager=err, repeats=a.repeats, warmup=a.warmup, calls_per_region=a.batch,
               what="ms per odeint call, host included; hip and plain: regions of calls_per_region calls behind one "
                    "synchronise, divided; eager: one call per region; host clock, median of alternating regions")
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
