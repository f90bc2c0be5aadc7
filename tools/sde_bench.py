"""Time of the one-launch SF2M samplers, `euler` and `srk`, at the shape the project quotes (bench.py's sde_em leg:
B = 2048, d = 2, two 3-64-64-64-2 fields, ts = [0, 1], dt = 0.01 -> 100 steps, Philox noise).

    python tools/sde_bench.py [--out profiles/sde_srk.txt]
    python tools/sde_bench.py --ab OTHER_CHECKOUT [--rounds 5] [--out profiles/sde_srk.txt]

Every figure comes from a fresh child process: 20 warm-up calls, then `--windows` windows of `--reps` sdeint calls
each between two device events (a window is a fraction of a second); printed are the median window, the smallest and
the largest, per call, and the time per field-pair evaluation (euler: 1 per step, srk: 3 per step).
--ab: the no-regression measurement for `euler`: the same child runs alternately on OTHER_CHECKOUT (built) and on this
tree, `--rounds` times each; printed are every run, the two medians and the other checkout's run-to-run spread.
Measurement infrastructure."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVALS = {"euler": 1, "srk": 3}
STEPS = 100


def one(method, tree, reps, windows):
    for p in (tree, os.path.join(tree, "oracle")):
        sys.path.insert(0, p)
    import torch
    import cfm_amd
    import cfm_oracle as oracle
    from cfm_amd.sde import FlowScoreSDE, sdeint
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    f = cfm_amd.MLP(dim=2, time_varying=True, w=64).to(dev)
    sc = cfm_amd.MLP(dim=2, time_varying=True, w=64).to(dev)
    x0, _ = oracle.config_inputs("C1", B=2048)
    y0, ts = x0.to(dev), torch.linspace(0, 1, 2)
    sde = FlowScoreSDE(f, sc, sigma=0.1)
    for _ in range(20):
        sdeint(sde, y0, ts, method=method, dt=0.01, fused=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            sdeint(sde, y0, ts, method=method, dt=0.01, fused=True)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    print("ONE " + json.dumps({"method": method, "ms": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}))


def child(method, tree, reps, windows):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", method, "--tree", tree, "--reps", str(reps),
                        "--windows", str(windows)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"sde_bench child ({method}, {tree}) failed (exit {r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("ONE ")][-1][4:])


def table(reps, windows):
    lines = [f"# one-launch SF2M samplers: B = 2048, d = 2, two 3-64-64-64-2 fields, {STEPS} steps, Philox noise",
             f"# fresh process per row; 20 warm-up calls; {windows} windows of {reps} sdeint calls between device events; ms per call",
             f"{'method':7s} {'median':>8s} {'min':>8s} {'max':>8s} {'evals':>6s} {'us/eval':>8s}"]
    res = {}
    for m in ("euler", "srk"):
        r = res[m] = child(m, ROOT, reps, windows)
        n = EVALS[m] * STEPS
        lines.append(f"{m:7s} {r['ms']:8.4f} {r['min']:8.4f} {r['max']:8.4f} {n:6d} {1e3 * r['ms'] / n:8.3f}")
    ratio = (res["srk"]["ms"] / EVALS["srk"]) / (res["euler"]["ms"] / EVALS["euler"])
    lines.append(f"srk / euler: {res['srk']['ms'] / res['euler']['ms']:.3f} per call, {ratio:.3f} per field-pair evaluation")
    return lines


def ab(other, rounds, reps, windows):
    runs = {"other": [], "this": []}
    lines = [f"# euler, fresh process per run, alternating: other checkout / this tree, {rounds} rounds; ms per call (median window)"]
    for i in range(rounds):
        for tag, tree in (("other", other), ("this", ROOT)):
            r = child("euler", tree, reps, windows)
            runs[tag].append(r["ms"])
            lines.append(f"round {i} {tag:5s} {r['ms']:.4f}  (min {r['min']:.4f} max {r['max']:.4f})")
    mo, mt = statistics.median(runs["other"]), statistics.median(runs["this"])
    spread = max(runs["other"]) - min(runs["other"])
    lines.append(f"median other {mo:.4f} ms   median this {mt:.4f} ms   difference {mt - mo:+.4f} ms   "
                 f"other's run-to-run spread {spread:.4f} ms   within spread: {mt - mo <= spread}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", metavar="OTHER_CHECKOUT", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a.one, os.path.abspath(a.tree), a.reps, a.windows)
    lines = ab(os.path.abspath(a.ab), a.rounds, a.reps, a.windows) if a.ab else table(a.reps, a.windows)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.ab else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
