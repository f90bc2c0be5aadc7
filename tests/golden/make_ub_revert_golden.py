"""Regenerates tests/golden/ub_revert_cases.npz: two small inputs on which the unbalanced Sinkhorn-Knopp loop of the
oracle (oracle/cfm_oracle.py: sinkhorn_knopp_unbalanced) meets a numerical error IN THE MIDDLE of the loop and returns
the previous iterate — one stopping at an even iteration, one at an odd one (the device loop keeps (u, v) in two
ping-pong buffers and picks the one to return by the parity of the iteration it stopped at).

    python tests/golden/make_ub_revert_golden.py

Seeded search, NumPy only: seed s draws B0, B1 in 2..8, 1-D clouds scaled by 10..40, reg_m = 10^(3..6); reg = 1.  A
seed is kept when
  * the oracle returns status 1 at an iteration >= 1;
  * the oracle with every sum taken in the reversed order stops at the same iteration, and its plan agrees to 1e-11 of
    the largest entry (so the stop does not hang on a rounding and the 1e-9 bound of the test checks the kernel);
  * the returned plan is finite with a positive largest entry.
The first kept seed of each parity is recorded: x0, x1 and their fp32 cost matrix M (the test hands M itself to the
solver: a last-bit difference of a device-built matrix could move the iteration), reg, reg_m, the iteration, the seed.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ub_shape_cases as cases  # noqa: E402

SEEDS = 4000
REG = 1.0


def draw(seed):
    rng = np.random.default_rng(seed)
    B0, B1 = int(rng.integers(2, 9)), int(rng.integers(2, 9))
    scale = float(rng.uniform(10.0, 40.0))
    reg_m = float(10.0 ** rng.uniform(3.0, 6.0))
    x0, x1 = cases.revert_cloud(B0, B1, scale, seed)
    return x0, x1, reg_m


def admissible(x0, x1, reg_m):
    M = cases.host_cost(x0, x1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        G, log = cases.unbalanced_ref(M, REG, reg_m)
        if log["status"] != 1 or log["iters"] < 1:
            return None
        Gr, logr = cases.unbalanced_ref(M, REG, reg_m, reverse=True)
    if (logr["iters"], logr["status"]) != (log["iters"], 1):
        return None
    if not np.isfinite(G).all() or not G.max() > 0.0 or cases.rel_gap(Gr, G) > cases.RTOL_REVERSED:
        return None
    return log["iters"]


def main():
    found, kept = {}, 0
    for seed in range(SEEDS):
        x0, x1, reg_m = draw(seed)
        it = admissible(x0, x1, reg_m)
        if it is None:
            continue
        kept += 1
        par = "odd" if it & 1 else "even"
        if par not in found:
            found[par] = (x0, x1, reg_m, it, seed)
    print(f"{kept} of {SEEDS} seeds kept")
    out = {}
    for par in ("even", "odd"):
        x0, x1, reg_m, it, seed = found[par]
        print(f"{par}: seed {seed}, {x0.shape[0]} x {x1.shape[0]}, reg_m {reg_m:.6g}, stops at iteration {it}")
        out[f"{par}_x0"], out[f"{par}_x1"], out[f"{par}_M"] = x0, x1, cases.host_cost(x0, x1)
        out[f"{par}_reg"], out[f"{par}_reg_m"] = np.float64(REG), np.float64(reg_m)
        out[f"{par}_iters"], out[f"{par}_seed"] = np.int64(it), np.int64(seed)
    np.savez(os.path.join(HERE, "ub_revert_cases.npz"), **out)


if __name__ == "__main__":
    main()
