"""Writes tests/golden/icnn_reference.json: the reference's own ICNN class under float64 autograd on the seeded case of
tests/icnn_restate.golden_case (d = 2, dimh = 8, L = 4, B = 6, both signs in Wzs, reg = 0.1).

    python tools/make_icnn_golden.py --reference /path/to/conditional-flow-matching

The reference file (runner/src/models/components/icnn_model.py) imports only torch and runs on a CPU.  It is loaded from
the checkout given on the command line; this tool is the only file of the repository that reads it, and no test does:
the tests read the fixture.  Only the reference's ICNN class is used; the three objectives are written here from their
formulas and differentiated by float64 autograd: the g-loss through the input gradient's own graph,
with f's parameters held constant."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icnn_restate as ir  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "icnn_reference.json"))
    args = ap.parse_args()
    path = os.path.join(args.reference, "runner", "src", "models", "components", "icnn_model.py")
    spec = importlib.util.spec_from_file_location("reference_icnn_model", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    Pf, Pg, x, y, reg = ir.golden_case()
    d, H, L = x.shape[1], Pf["Wzs.0.bias"].shape[0], 4
    nets = []
    for P in (Pf, Pg):
        net = ref.ICNN(dim=d, dimh=H, num_hidden_layers=L).double()
        net.load_state_dict({k: torch.tensor(v) for k, v in P.items()}, strict=True)
        nets.append(net)
    f, g = nets
    xt = torch.tensor(x, requires_grad=True)
    yt = torch.tensor(y, requires_grad=True)

    def input_gradient(net, pts, keep_graph):
        """the net's transport map at pts, with a graph of its own when the caller differentiates through it"""
        return torch.autograd.grad(net(pts).sum(), pts, create_graph=keep_graph)[0]

    def negative_part_penalty(net):
        halves = torch.zeros(len(net.Wzs), dtype=torch.float64)
        for k, layer in enumerate(net.Wzs):
            halves[k] = 0.5 * torch.relu(-layer.weight).square().sum()
        return reg * halves.sum()

    def parameter_gradients(loss, net):
        gs = torch.autograd.grad(loss, list(net.parameters()), allow_unused=True)
        return {k: (torch.zeros_like(p) if q is None else q).tolist() for (k, p), q in zip(net.named_parameters(), gs)}

    out_f = f(xt)
    grad_f = input_gradient(f, xt, False)
    p = input_gradient(g, yt, True)                       # depends on g's parameters
    f_at_p = f(p)
    y_dot_p = (yt * p).sum(dim=1, keepdim=True)
    f_at_x = f(xt)
    # issue section 1: g_loss = mean(f(p) - y.p) + penalty(g), gradients on g; f_loss = mean(f(x) - f(p)) + penalty(f)
    # with p a constant, gradients on f; w2 = mean(f(p) - f(x) - y.p + |x|^2 / 2 + |y|^2 / 2)
    g_loss = (f_at_p - y_dot_p).mean() + negative_part_penalty(g)
    g_grads = parameter_gradients(g_loss, g)
    f_loss = (f_at_x - f(p.detach())).mean() + negative_part_penalty(f)
    f_grads = parameter_gradients(f_loss, f)
    half_x2, half_y2 = 0.5 * xt.square().sum(dim=1, keepdim=True), 0.5 * yt.square().sum(dim=1, keepdim=True)
    w2_terms = (f_at_p - f_at_x - y_dot_p + half_x2 + half_y2).mean(), (f_at_x - f_at_p).mean(), (f_at_p - y_dot_p).mean()

    out = {
        "dim": d, "dimh": H, "num_hidden_layers": L, "reg": reg,
        "keys": [[k, list(p.shape)] for k, p in f.state_dict().items()],
        "f": {k: np.asarray(v).tolist() for k, v in Pf.items()}, "g": {k: np.asarray(v).tolist() for k, v in Pg.items()},
        "x": x.tolist(), "y": y.tolist(),
        "f_out": out_f.detach()[:, 0].tolist(), "f_transport": grad_f.tolist(), "g_transport": p.detach().tolist(),
        "f_loss": float(f_loss.detach()), "g_loss": float(g_loss.detach()),
        "w2": [float(v.detach()) for v in w2_terms],
        "f_grads": f_grads, "g_grads": g_grads,
    }
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
