"""Time per solve and per function evaluation of every NeuralODE solver at the C5 sampling shape (B = 8192,
51-64-64-64-50 SELU field, t_span = linspace(0, 1, 100), atol = rtol = 1e-4), with the method of bench.py's c5_ode_leg:
one process, one warm-up solve, the median of 5 wall-clock times on a stream of its own.

    python tools/ode_solvers_bench.py [--out profiles/ode_solvers.txt]
    python tools/ode_solvers_bench.py --ab OTHER_CHECKOUT [--rounds 5]

--ab: the no-regression measurement for dopri5.  bench.py's own c5_ode_leg (the `dopri5_ms` of `bench.py --full`) runs
in a fresh child process alternately in OTHER_CHECKOUT (built) and in this tree, `--rounds` times each; printed are
every run, the two medians and the other checkout's run-to-run spread (max - min of its medians).
Measurement infrastructure."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = ("euler", "midpoint", "rk4", "dopri5", "tsit5")
_LEG = ("import json, torch, bench; dev = torch.device('cuda:0'); torch.cuda.set_device(dev); "
        "r = bench.c5_ode_leg(dev); print('LEG ' + json.dumps({k: r[k] for k in ('dopri5_ms', 'dopri5_ms_all', 'nfe', 'step_attempts')}))")


def solvers_table():
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import cfm_amd
    import cfm_oracle as oracle
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    x0, _ = oracle.config_inputs("C5")
    torch.manual_seed(0)
    model = cfm_amd.MLP(dim=50, time_varying=True, w=64).to(dev)
    ts = torch.linspace(0, 1, 100)
    x = x0.to(dev)
    lines = ["# C5 sampling shape: B = 8192, field 51-64-64-64-50, t_span = linspace(0, 1, 100), atol = rtol = 1e-4",
             "# one warm-up solve, median of 5 (all 5 listed), one process",
             f"{'solver':9s} {'ms':>8s} {'nfe':>6s} {'step_attempts':>14s} {'us/nfe':>8s}   ms_all"]
    with torch.cuda.stream(torch.cuda.Stream()):
        for solver in SOLVERS:
            node = NeuralODE(torch_wrapper(model), solver=solver, atol=1e-4, rtol=1e-4)
            node.trajectory(x, ts)
            torch.cuda.synchronize()
            assert node.last_path == "hip"
            times = []
            for _ in range(5):
                t0 = time.perf_counter()
                node.trajectory(x, ts)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            ms = float(np.median(times))
            lines.append(f"{solver:9s} {ms:8.3f} {node.nfe:6d} {node.n_steps:14d} {1e3 * ms / max(1, node.nfe):8.3f}   "
                         + " ".join(f"{t:.3f}" for t in times))
    return lines


def leg(tree):
    r = subprocess.run([sys.executable, "-c", _LEG], cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"c5_ode_leg failed in {tree} (exit {r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])


def ab(other, rounds):
    import statistics
    runs = {"other": [], "this": []}
    lines = [f"# dopri5_ms of bench.py's c5_ode_leg, fresh process per run, alternating: other checkout / this tree, {rounds} rounds"]
    for i in range(rounds):
        for tag, tree in (("other", other), ("this", ROOT)):
            r = leg(tree)
            runs[tag].append(r["dopri5_ms"])
            lines.append(f"round {i} {tag:5s} dopri5_ms {r['dopri5_ms']:.3f}  all {r['dopri5_ms_all']}  nfe {r['nfe']}  "
                         f"step_attempts {r['step_attempts']}")
    mo, mt = statistics.median(runs["other"]), statistics.median(runs["this"])
    spread = max(runs["other"]) - min(runs["other"])
    lines.append(f"median other {mo:.3f} ms   median this {mt:.3f} ms   difference {mt - mo:+.3f} ms   "
                 f"other's run-to-run spread {spread:.3f} ms   within spread: {mt - mo <= spread}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", metavar="OTHER_CHECKOUT", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    lines = ab(os.path.abspath(a.ab), a.rounds) if a.ab else solvers_table()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.ab else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
