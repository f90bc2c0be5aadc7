"""Writes tests/golden/cnf_reg_field.npz: the reference's augmented vector field with the CNF term and the two
regularisers, recorded in float64 (build container only: the reference tree must be present).

    python tests/golden/make_cnf_reg_golden.py

The reference's runner/src/models/components/augmentation.py is loaded by path, unmodified, and
AugmentedVectorField(net, [CNFReg(), SquaredL2Reg(), JacobianFrobeniusReg()], d) is evaluated on
torchcfm.models.MLP(dim=d, w=16, time_varying=True) (loaded by path too) behind the (t, x) -> net([x, t]) adapter that
torchcfm.utils.torch_wrapper is.  Per case: the MLP's weights and biases, x [B, d], t, and the [B, 3 + d] output
(-tr J, |v|^2, ||J||_F / d, v).  Nothing else is taken from the reference."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import ref_import  # noqa: E402

CASES = [(2, 5, 0.3), (3, 4, 0.7)]          # (d, B, t)


def _load(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_import.REFERENCE_ROOT, *rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _TimeAdapter(torch.nn.Module):
    """torchcfm.utils.torch_wrapper: (t, x) -> model(cat([x, t.repeat(B)[:, None]], 1))"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, t, x, *args, **kwargs):
        return self.model(torch.cat([x, t.repeat(x.shape[0])[:, None]], 1))


def main():
    aug = _load("ref_augmentation", "runner", "src", "models", "components", "augmentation.py")
    models = _load("ref_torchcfm_models", "torchcfm", "models", "models.py")

    class CNFReg(aug.CNFReg):
        """CNFReg.forward (augmentation.py:132-134) returns ``-trace + 0 * x``: a [B] trace plus a [B, d] zero, which
        broadcasts only when B == d and then no longer stacks with the other regularisers' [B] columns.  The term is
        there to tie x into the graph and carries no value; this is the same forward without it, on the reference's own
        trace estimator."""

        def forward(self, t, x, dx, context):
            return -self.trace_estimator(dx, x)
    aug.CNFReg = CNFReg
    out = {}
    torch.set_default_dtype(torch.float64)
    for c, (d, B, t) in enumerate(CASES):
        torch.manual_seed(100 + c)
        net = models.MLP(dim=d, w=16, time_varying=True)
        field = aug.AugmentedVectorField(_TimeAdapter(net), [aug.CNFReg(), aug.SquaredL2Reg(), aug.JacobianFrobeniusReg()], d)
        x = torch.randn(B, d)
        state = torch.cat([torch.zeros(B, 3), x], 1)
        got = field(torch.tensor(t), state).detach()
        assert got.shape == (B, 3 + d), got.shape
        lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
        for l, lin in enumerate(lins):
            out[f"c{c}_W{l}"] = lin.weight.detach().numpy()
            out[f"c{c}_b{l}"] = lin.bias.detach().numpy()
        out[f"c{c}_x"] = x.numpy()
        out[f"c{c}_t"] = np.float64(t)
        out[f"c{c}_out"] = got.numpy()
    path = os.path.join(HERE, "cnf_reg_field.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
