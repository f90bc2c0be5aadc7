"""ICNN optimal-transport timings on the GPU (measurement tool; bench.py is the headline).

    python tools/icnn_bench.py [--repeats 9] [--warmup 2] [--batch 20] [--out FILE]

The runner's shape: ``ICNN(dim=2, dimh=64, num_hidden_layers=4)`` for f and g, at B = 256 and at B = 4096.  Four
operations, one call each: G_STEP (``icnn_g_loss`` + ``backward``), F_STEP (``icnn_f_loss`` + ``backward``), W2
(``icnn_w2(..., return_loss=True)``) and TRANSPORT (``ICNN.transport``).  Two paths on the same GPU, alternating region by
region:
  hip     : one cfm_icnn_f32 call per operation (csrc/icnn.hip: 4, 3, 3 and 1 launches);
  generic : the reference's formulation in torch ops (autograd.grad(create_graph=True) and a double backward for the
            g-step): the fused small-field path switched off.
G_STEP is also set beside ``action_matching_loss`` + ``backward`` at the same B (MLP(dim=2, out_dim=1, w=64,
time_varying=True)): the library's other fused double backward, as a yardstick.
A region is --batch calls back to back behind ONE device synchronise; its figure is the region's time divided by --batch:
time per call in a stream of calls, host included.  After --warmup regions of each path the figure is the median of
--repeats regions (min and max are printed with it).  The results of the two paths on the timed inputs are compared
(max|hip - generic| / max|generic| over the outputs) so that the figures are of the same result.
Not measured: the kernels' time apart from the call (no profiler run), LDS bank conflicts (no counter run).
No GPU, no figure: the tool raises.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

WHAT = ("ms per call (G_STEP, F_STEP and the yardstick: loss + backward; W2 and TRANSPORT: the call alone); regions of calls_per_region calls behind one synchronise, divided; host clock, "
        "median of alternating regions; not measured: kernel time apart from the call, LDS bank conflicts")


def _ops(f, g, x, y):
    import cfm_amd

    def step(fn, net):
        def call():
            for p in net.parameters():
                p.grad = None
            fn(f, g, x, y, reg=0.1).backward()
            return [p.grad for p in net.parameters()], fn.last_path
        return call

    def w2():
        return list(cfm_amd.icnn_w2(f, g, x, y, return_loss=True)), cfm_amd.icnn_w2.last_path

    def transport():
        return [f.transport(x)], cfm_amd.ICNN.transport.last_path

    return {"G_STEP": step(cfm_amd.icnn_g_loss, g), "F_STEP": step(cfm_amd.icnn_f_loss, f), "W2": w2, "TRANSPORT": transport}


def _time(call, lib, fused, batch):
    lib.cfm_ode_set_fused(1 if fused else 0)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batch):
            out, path = call()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / batch
    finally:
        lib.cfm_ode_set_fused(1)
    return ms, [o.detach().clone() for o in out], path


def run_case(B, repeats, warmup, batch, dev):
    import cfm_amd
    from cfm_amd import _lib
    lib = _lib.load()
    torch.manual_seed(0)
    d, H, L = 2, 64, 4
    f, g = cfm_amd.ICNN(d, H, L).to(dev), cfm_amd.ICNN(d, H, L).to(dev)
    x, y = 1.5 * torch.randn(B, d, device=dev), 0.5 + torch.randn(B, d, device=dev)
    rows = []
    for name, call in _ops(f, g, x, y).items():
        for _ in range(warmup):
            _time(call, lib, True, batch)
            _time(call, lib, False, batch)
        hip, gen = [], []
        for _ in range(repeats):                  # alternating: both paths see the same neighbours on the machine
            a = _time(call, lib, True, batch)
            b = _time(call, lib, False, batch)
            hip.append(a[0])
            gen.append(b[0])
        assert (a[2], b[2]) == ("hip", "generic"), (a[2], b[2])
        err = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for p, q in zip(a[1], b[1]))
        h, gm = statistics.median(hip), statistics.median(gen)
        rows.append(dict(case="icnn_" + name, B=B, d=d, dimh=H, L=L, hip_ms=round(h, 4),
                         hip_min_max=[round(min(hip), 4), round(max(hip), 4)], generic_ms=round(gm, 3),
                         generic_min_max=[round(min(gen), 3), round(max(gen), 3)], x_generic=round(gm / h, 1),
                         rel_diff=err, repeats=repeats, warmup=warmup, calls_per_region=batch, what=WHAT))
    # the yardstick: the action-matching loss + backward at the same B
    m = cfm_amd.MLP(dim=d, out_dim=1, w=64, time_varying=True).to(dev)
    x0, t = 1.5 * torch.randn(B, d, device=dev), torch.rand(B, device=dev)

    def am():
        for p in m.parameters():
            p.grad = None
        cfm_amd.action_matching_loss(m, x0, y, t).backward()
        return [p.grad for p in m.parameters()], cfm_amd.action_matching_loss.last_path
    for _ in range(warmup):
        _time(am, lib, True, batch)
    ams = [_time(am, lib, True, batch) for _ in range(repeats)]
    assert ams[-1][2] == "hip"
    v = [r[0] for r in ams]
    rows.append(dict(case="action_matching_train_yardstick", B=B, d=d, w=64, hip_ms=round(statistics.median(v), 4),
                     hip_min_max=[round(min(v), 4), round(max(v), 4)], repeats=repeats, warmup=warmup, calls_per_region=batch,
                     what=WHAT))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("icnn_bench: no GPU, no measurement")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []
    for B in (256, 4096):
        for r in run_case(B, a.repeats, a.warmup, a.batch, dev):
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/icnn_bench.py   (MI355X; ICNN(dim=2, dimh=64, num_hidden_layers=4) for f and g; B = 256 and 4096)\n")
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
