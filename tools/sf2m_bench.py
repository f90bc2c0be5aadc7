"""The [SF]2M training step, timed and counted (results: profiles/sf2m_step.txt).

    python tools/sf2m_bench.py time [--out FILE]                 # the three forms at both shapes, alternating
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sf2m_bench.py run sf2m|regression|eager --steps 50
    python tools/sf2m_bench.py launches DIR --steps 50           # launches per step out of such a capture

Forms, each at (B, d, w) = (256, 2, 64) and (4096, 784, 512), time-varying nets:
  (a) sf2m        cfm_amd.SF2MStep + one FusedAdam over both nets — cfm_mlp_sf2m_step_f32 + cfm_adam_step_f32;
  (b) eager       the notebook's lines (SF2M_tutorial.ipynb cell 3) on what the library offered before this step:
                  cfm_amd.MLP's autograd path for both nets, eager cat / mul / add / pow / mean, one FusedAdam over both;
  (c) regression  cfm_amd.RegressionStep(model) + FusedAdam: ONE net's step, the yardstick for "two nets in the
                  launches of one".
Method: 20 warm-up steps per form, then REGIONS regions per form, the forms alternating region by region; a region is
STEPS steps between two device events.  Reported per form: the median region (per step), the smallest and the largest,
and the spread (largest - smallest) / median.  Measurement infrastructure; not part of the product path."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 2, 64), (4096, 784, 512)]
SIGMA = 0.5


def make_forms(B, d, w, dev):
    import torch
    import cfm_amd
    torch.manual_seed(0)
    t = torch.rand(B, device=dev); xt = torch.randn(B, d, device=dev); ut = torch.randn(B, d, device=dev)
    eps = torch.randn(B, d, device=dev); lam = 2 * torch.sqrt(t * (1 - t)) / SIGMA

    def nets():
        return (cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev), cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev))

    fa, sa = nets()
    step_a = cfm_amd.SF2MStep(fa, sa, cfm_amd.FusedAdam(list(fa.parameters()) + list(sa.parameters()), lr=1e-3))
    fb, sb = nets()
    opt_b = cfm_amd.FusedAdam(list(fb.parameters()) + list(sb.parameters()), lr=1e-3)
    fc, _ = nets()
    step_c = cfm_amd.RegressionStep(fc, cfm_amd.FusedAdam(fc.parameters(), lr=1e-3))

    def sf2m():
        step_a(t, xt, ut, eps, lam)

    def eager():
        opt_b.zero_grad(set_to_none=True)
        vt = fb(torch.cat([xt, t[:, None]], dim=-1))
        st = sb(torch.cat([xt, t[:, None]], dim=-1))
        flow_loss = torch.mean((vt - ut) ** 2)
        score_loss = torch.mean((lam[:, None] * st + eps) ** 2)
        loss = flow_loss + score_loss
        loss.backward(); opt_b.step()

    def regression():
        step_c(t, xt, ut)

    return {"sf2m": sf2m, "eager": eager, "regression": regression}


def cmd_time(args):
    import torch
    from cfm_amd import _lib
    _lib.load(); dev = _lib.require_gpu()
    lines = [f"# tools/sf2m_bench.py time: {args.regions} regions of STEPS steps per form, forms alternating; us per step",
             f"# {torch.cuda.get_device_name(dev)}, torch {torch.__version__}"]
    for (B, d, w) in SHAPES:
        forms = make_forms(B, d, w, dev)
        steps = args.steps_small if B <= 256 else args.steps_large
        for f in forms.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(args.regions):
            for k, f in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    f()
                e1.record(); e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / steps)
        lines.append(f"shape B={B} d={d} w={w} ({d + 1}-{w}-{w}-{w}-{d}), {steps} steps per region")
        med = {}
        for k, v in times.items():
            med[k] = statistics.median(v)
            lines.append(f"  {k:<11s} median {med[k]:9.1f}   min {min(v):9.1f}   max {max(v):9.1f}   spread {(max(v) - min(v)) / med[k] * 100:5.1f} %")
        spread = {k: max(v) - min(v) for k, v in times.items()}
        lines.append(f"  (a) < (b) by more than the spread: {med['sf2m']:.1f} vs {med['eager']:.1f}, spreads {spread['sf2m']:.1f} / {spread['eager']:.1f}: "
                     f"{'HELD' if med['sf2m'] + max(spread['sf2m'], spread['eager']) < med['eager'] else 'NOT held'}")
        lines.append(f"  (a) <= 2 x (c) + spread of (c): {med['sf2m']:.1f} vs {2 * med['regression'] + spread['regression']:.1f}: "
                     f"{'HELD' if med['sf2m'] <= 2 * med['regression'] + spread['regression'] else 'NOT held'}")
        lines.append(f"  (a) / (c) = {med['sf2m'] / med['regression']:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


def cmd_run(args):
    """exactly --steps steps of ONE form at the small shape, no warm-up: every kernel of a step is launched --steps times"""
    import torch
    from cfm_amd import _lib
    _lib.load(); dev = _lib.require_gpu()
    f = make_forms(*SHAPES[0], dev)[args.form]
    for _ in range(args.steps):
        f()
    torch.cuda.synchronize()


def cmd_launches(args):
    """kernel_stats of a capture -> launches per step: a kernel's calls // steps (set-up kernels run once and drop out)"""
    files = glob.glob(os.path.join(args.dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_stats.csv under {args.dir}")
    total = 0
    for path in files:
        with open(path) as fh:
            for r in csv.DictReader(fh):
                name, calls = r.get("Name") or r.get("kernel"), int(r.get("Calls") or r.get("calls"))
                if calls // args.steps:
                    print(f"  {calls // args.steps:3d} x {name[:110]}")
                    total += calls // args.steps
    print(f"launches per step: {total}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("time")
    p.add_argument("--regions", type=int, default=15)
    p.add_argument("--steps-small", type=int, default=1000)
    p.add_argument("--steps-large", type=int, default=100)
    p.add_argument("--out", default=None)
    p = sub.add_parser("run")
    p.add_argument("form", choices=["sf2m", "eager", "regression"])
    p.add_argument("--steps", type=int, default=50)
    p = sub.add_parser("launches")
    p.add_argument("dir")
    p.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    {"time": cmd_time, "run": cmd_run, "launches": cmd_launches}[args.cmd](args)


if __name__ == "__main__":
    main()
