"""Regenerates tests/golden/dsbm_cases.npz: the DSBM (diffusion Schrodinger bridge matching) batch and training loop of the
reference's runner, restated in float64.

    python tests/golden/make_dsbm_golden.py

``run:LINE`` cites the reference's ``runner/src/models/cfm_module.py``.  Its Lightning module (DSBMLitModule, run:1183-1227)
is not importable without Lightning and hydra, so — as ``cfm_amd/schedule.py`` restates the schedules — the lines are
restated here with torch alone, independently of the package under test:

    calc_mu_sigma        run:834-841      mu_t = x0 + (x1 - x0) F(t) / F(1);  sigma_t = sqrt(F(t) - F(t)^2 / F(1))
    x                    run:856          x = mu_t + sigma_t eps
    the two targets      run:1192-1199    x1 - x0 - g sqrt(t / (1 - t + 1e-6)) eps;  x0 - x1 - g sqrt((1 - t) / (t + 1e-6)) eps
    the two scalings     run:1215-1216    (1 + g^2 t / (1 - t + 1e-6)) ** -1;  (1 + g^2 (1 - t) / (t + 1e-6)) ** -1
    the two losses       run:1221-1227    mean(scaling[:, None] * (net([x, t]) - target) ** 2), summed for the backward
    the nets             torchcfm/models/models.py:10-21  (Linear-SELU x 3 + Linear on [x, t])
    the schedules        runner/src/models/components/schedule.py  (constant; linearly decreasing variance)

Per case (schedule, B = 256, d = 2, w = 64), seeded:
  * both nets' initial fp32 state dicts (fwd_*, bwd_*);
  * batch 0's inputs in float64 (x0, x1, t, eps: fp32 values, upcast) and its float64 outputs (``b0_*64``);
  * for each of 5 steps t, xt, both targets and both scalings as fp32 (``b{k}_*``), computed in float64 and rounded once;
  * the float64 losses and float64 parameter gradients of step 0 (fp32 inputs and weights, upcast);
  * the float64 five-step sequences of both losses under torch.optim.Adam(lr=1e-3) over both nets.
t is drawn from U[0.05, 0.95]: the targets' noise coefficients reach 1e3 g at the ends, where a float32 step cannot be
held to 1e-5.  The loop is also run in float32 and must stay within 1e-5 (relative) of the float64 sequences: the
recorded batches are therefore well conditioned enough that a float32 implementation can be held to the tests' bound.
"""
import copy
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (schedule kind, schedule parameters, seed)
CASES = {"const1": ("constant", (1.0,), 21), "lin": ("linear", (0.1, 1.0), 22)}
B, D, W, STEPS = 256, 2, 64, 5
T_LO, T_HI = 0.05, 0.95


def g_of(kind, par, t):
    """the diffusion g(t) (schedule.py of the runner): constant sigma; sqrt of the linearly decreasing variance"""
    if kind == "constant":
        return par[0] * torch.ones_like(t)
    smin, smax = par
    return torch.sqrt(t * smin + (1 - t) * smax)


def F_of(kind, par, t):
    """F(t) = int_0^t g^2"""
    if kind == "constant":
        return par[0] ** 2 * t
    smin, smax = par
    return smax * t + t ** 2 * ((smin - smax) / 2)


def mlp(d, w):
    """torchcfm/models/models.py:10-21 at time_varying=True, under the same parameter names (net.0 ... net.6)"""
    m = torch.nn.Module()
    m.net = torch.nn.Sequential(torch.nn.Linear(d + 1, w), torch.nn.SELU(), torch.nn.Linear(w, w), torch.nn.SELU(),
                                torch.nn.Linear(w, w), torch.nn.SELU(), torch.nn.Linear(w, d))
    return m


def bridge(kind, par, x0, x1, t, eps):
    """run:834-841, :856, :1192-1199, :1215-1216 in the dtype of the inputs: (xt, forward_target, backward_target,
    forward_scaling, backward_scaling)"""
    tx = t.reshape(-1, *([1] * (x0.dim() - 1)))
    ft_, fone = F_of(kind, par, tx), F_of(kind, par, torch.ones((), dtype=t.dtype))
    mu_t = x0 + (x1 - x0) * ft_ / fone
    sigma_t = torch.sqrt(ft_ - ft_ ** 2 / fone)
    x = mu_t + sigma_t * eps
    g = g_of(kind, par, tx)
    forward_target = x1 - x0 - (g * torch.sqrt(tx / (1 - tx + 1e-6))) * eps
    backward_target = x0 - x1 - (g * torch.sqrt((1 - tx) / (tx + 1e-6))) * eps
    g1 = g_of(kind, par, t)
    forward_scaling = (1 + g1 ** 2 * t / (1 - t + 1e-6)) ** -1
    backward_scaling = (1 + g1 ** 2 * (1 - t) / (t + 1e-6)) ** -1
    return x, forward_target, backward_target, forward_scaling, backward_scaling


def losses(fwd, bwd, t, xt, ft, bt, fs, bs):
    """run:1221-1223"""
    x = torch.cat([xt, t[:, None]], dim=-1)
    forward_loss = torch.mean(fs[:, None] * (fwd.net(x) - ft) ** 2)
    backward_loss = torch.mean(bs[:, None] * (bwd.net(x) - bt) ** 2)
    return forward_loss, backward_loss


def loop(fwd, bwd, batches, dtype):
    fwd, bwd = copy.deepcopy(fwd).to(dtype), copy.deepcopy(bwd).to(dtype)
    params = list(fwd.parameters()) + list(bwd.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    seq, grads0 = [], None
    for k, b in enumerate(batches):
        opt.zero_grad()
        fl, bl = losses(fwd, bwd, *[x.to(dtype) for x in b])
        (fl + bl).backward()
        if k == 0:
            grads0 = [p.grad.detach().clone() for p in params]
        opt.step()
        seq.append((float(fl.detach()), float(bl.detach())))
    return np.asarray(seq, dtype=np.float64), grads0


def make_case(name, kind, par, seed, out):
    torch.manual_seed(seed)
    fwd, bwd = mlp(D, W), mlp(D, W)
    batches = []
    for k in range(STEPS):
        x0 = torch.randn(B, D)
        x1 = torch.randn(B, D) * 0.5 + torch.tensor([2.0, -1.0])[:D]
        t = T_LO + (T_HI - T_LO) * torch.rand(B)
        eps = torch.randn(B, D)
        res64 = bridge(kind, par, x0.double(), x1.double(), t.double(), eps.double())
        if k == 0:
            for nm, v in zip(("x0", "x1", "t", "eps"), (x0, x1, t, eps)):
                out[f"{name}_b0_{nm}64"] = v.double().numpy()
            for nm, v in zip(("xt", "ft", "bt", "fs", "bs"), res64):
                out[f"{name}_b0_{nm}64"] = v.numpy()
        batches.append((t,) + tuple(v.float() for v in res64))
    seq64, g64 = loop(fwd, bwd, batches, torch.float64)
    seq32, _ = loop(fwd, bwd, batches, torch.float32)
    dev = float(np.max(np.abs(seq32 - seq64) / np.abs(seq64)))
    print(f"{name}: {kind}{par} B={B} d={D} w={W}: fp32 loop vs float64: {dev:.2e}; losses {seq64[0]} -> {seq64[-1]}")
    assert dev <= 1e-5, dev
    for tag, net in (("fwd", fwd), ("bwd", bwd)):
        for k, v in net.state_dict().items():
            out[f"{name}_{tag}_{k}"] = v.detach().numpy().astype(np.float32)
    for k, b in enumerate(batches):
        for nm, v in zip(("t", "xt", "ft", "bt", "fs", "bs"), b):
            out[f"{name}_b{k}_{nm}"] = v.numpy().astype(np.float32)
    names = [f"fwd_{k}" for k, _ in fwd.named_parameters()] + [f"bwd_{k}" for k, _ in bwd.named_parameters()]
    for nm, g in zip(names, g64):
        out[f"{name}_grad0_{nm}"] = g.numpy().astype(np.float64)
    out[f"{name}_losses"] = seq64                                   # [STEPS, 2]: forward, backward
    out[f"{name}_meta"] = np.asarray([B, D, W] + list(par), dtype=np.float64)


def main():
    out = {}
    for name, (kind, par, seed) in CASES.items():
        make_case(name, kind, par, seed, out)
    path = os.path.join(HERE, "dsbm_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} kB")


if __name__ == "__main__":
    main()
