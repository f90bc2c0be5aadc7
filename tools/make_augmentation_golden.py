"""Writes tests/golden/augmentation_integrands.json: the five integrands of AugmentationModule as the reference's own
classes return them, in float64, for the seeded net and points of tests/augment_restate.golden_case.

    python tools/make_augmentation_golden.py --reference /path/to/conditional-flow-matching

The reference file (runner/src/models/components/augmentation.py) imports only torch and runs on a CPU.  It is loaded
from the checkout given on the command line; this tool is the only file of the repository that reads the reference
tree, and no test does: the tests read the fixture.

log_prob is minus ``autograd_trace(dx, x)``, the function ``CNFReg`` calls.  ``CNFReg.forward`` itself adds ``0 * x``
([B] + [B, d]) and so only broadcasts where B == d; the other four are the classes' ``forward``."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_restate as ar  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "augmentation_integrands.json"))
    args = ap.parse_args()
    path = os.path.join(args.reference, "runner", "src", "models", "components", "augmentation.py")
    spec = importlib.util.spec_from_file_location("reference_augmentation", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    Ws, bs, x, times = ar.golden_case()
    W = [torch.tensor(np.asarray(w, np.float64)) for w in Ws]
    b = [torch.tensor(np.asarray(q, np.float64)) for q in bs]

    def net(t, y):
        h = torch.cat([y, torch.full_like(y[:, :1], float(t))], 1)
        for l in range(3):
            h = torch.nn.functional.selu(h @ W[l].T + b[l])
        return h @ W[3].T + b[3]

    class Ctx:
        pass

    regs = {"L1": ref.L1Reg(), "L2": ref.L2Reg(), "squared_L2": ref.SquaredL2Reg(),
            "jacobian_frobenius": ref.JacobianFrobeniusReg()}
    out = {"seed": 11, "times": list(times), "x": np.asarray(x, np.float64).tolist(), "integrands": []}
    for t in times:
        y = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
        dx = net(t, y)
        row = {"log_prob": (-ref.autograd_trace(dx, y)).detach().tolist()}
        for name, reg in regs.items():
            row[name] = reg(t, y, dx, Ctx).detach().tolist()
        out["integrands"].append(row)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
