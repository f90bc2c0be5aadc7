"""The log-ratio column's price on the one-launch SDE sampler, on the GPU (measurement tool; bench.py is the headline).

    python tools/sde_logqp_bench.py [--repeats 20] [--batch 20] [--method euler] [--out profiles/sde_logqp.txt]

One call = ``sdeint(FlowScoreSDE(v, s, sigma=0.5), x0, linspace(0, 1, 101), method=..., dt=0.01)`` at B = 2048, d = 2,
w = 64: 100 steps, every one a trajectory point (the most output the column can be asked for), Philox noise.  Three
paths in one run, alternating region by region so that each sees the same neighbours on the machine:
  logqp : ``logqp=True`` on the one-launch kernel (flag bit 1 of cfm_sde_em_mlp_f32 / cfm_sde_srk_mlp_f32); a region is
          --batch calls back to back behind ONE device synchronise, its figure the region's time divided by --batch
          (host included: packing the records and qw, the seed draw, the launch);
  plain : ``logqp=False``, the same regions: what the column is added to.  The ratio is reported, not gated;
  eager : the same scheme and integrand stepped in torch ops on the same GPU (the nets as plain callables, so that nothing
          routes them to the HIP paths), ``logqp=True``: all a user had before.  A region is one call.
After --warmup regions of each path the figure is the median of --repeats regions; min and max are printed with it, and
the tool says whether logqp is faster than eager by more than the two spreads together.  Both log-ratios are compared on
one given noise tensor so that the figures are of the same result.
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
    ap.add_argument("--batch", type=int, default=20, help="logqp / plain calls per timed region")
    ap.add_argument("--method", default="euler", choices=("euler", "srk"))
    ap.add_argument("--out", default=None, help="append the result line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sde_logqp_bench: no GPU, no measurement")
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd.sde import FlowScoreSDE, _grid, sdeint
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, d, w, n_t, dt = 2048, 2, 64, 101, 0.01
    torch.manual_seed(0)
    v = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    s = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    x0 = torch.randn(B, d, device=dev)
    ts = torch.linspace(0, 1, n_t, dtype=torch.float64)      # (a float32 grid has intervals above dt: they would be split)
    n_steps = len(_grid(ts, dt))
    assert n_steps == n_t - 1, n_steps
    hip =FlowScoreSDE(v, s, sigma=0.5)
    eager = FlowScoreSDE(v.net, s.net, sigma=0.5)

    def region(sde, calls, logqp, path):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = sdeint(sde, x0, ts, method=a.method, dt=dt, logqp=logqp)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / calls
        assert sde.last_path == path, sde.last_path
        return ms, out

    paths = {"logqp": (hip, a.batch, True, "hip"), "plain": (hip, a.batch, False, "hip"), "eager": (eager, 1, True, "eager")}
    for _ in range(a.warmup):
        for p in paths.values():
            region(*p)
    times = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, p in paths.items():
            times[k].append(region(*p)[0])
    # the same result: both log-ratios on one noise tensor
    xi =torch.randn((n_steps, 2, B, d) if a.method == "srk" else (n_steps, B, d), device=dev)
    lr_hip = sdeint(hip, x0, ts, method=a.method, dt=dt, noise=xi, logqp=True)[1]
    lr_eager = sdeint(eager, x0, ts, method=a.method, dt=dt, noise=xi, logqp=True)[1]
    err = float((lr_hip - lr_eager).abs().max() / lr_eager.abs().max())
    med = {k: statistics.median(t) for k, t in times.items()}
    spread = {k: max(t) - min(t) for k, t in times.items()}
    row = dict(case="sde_logqp", method=a.method, B=B, d=d, w=w, n_steps=n_steps, n_out=n_steps,
               logqp_ms=round(med["logqp"], 4), logqp_min_max=[round(min(times["logqp"]), 4), round(max(times["logqp"]), 4)],
               plain_ms=round(med["plain"], 4), plain_min_max=[round(min(times["plain"]), 4), round(max(times["plain"]), 4)],
               eager_ms=round(med["eager"], 2), eager_min_max=[round(min(times["eager"]), 2), round(max(times["eager"]), 2)],
               x_plain=round(med["logqp"] / med["plain"], 3), x_eager=round(med["eager"] / med["logqp"], 1),
               faster_than_eager_by_more_than_the_spreads=bool(med["eager"] - med["logqp"] > spread["eager"] + spread["logqp"]),
               logratio_rel_diff_hip_eager=err, repeats=a.repeats, warmup=a.warmup, calls_per_region=a.batch,
               what="ms per sdeint call, host included; logqp and plain: regions of calls_per_region calls behind one "
                    "synchronise, divided; eager: one call per region; host clock, median of alternating regions")
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
