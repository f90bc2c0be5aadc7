"""CPU: the gradient of the plain fixed-step solves.  The float64 restatement (tests/ode_grad_restate.py) is pinned by
finite differences and by the reverse sweep written out without autograd (what the kernel runs); then
DifferentiableNeuralODE's generic path is pinned against it, and the C ABI carries the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cfm_amd
import cnf_restate as cr
import ode_grad_restate as og
from cfm_amd import _lib
from cfm_amd.utils import torch_wrapper

DOWN = np.linspace(1.0, 0.0, 5).astype(np.float32)                                # decreasing, uniform
UP = np.array([0.0, 0.07, 0.3, 0.35, 0.81, 1.0], np.float32)                      # increasing, non-uniform
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfm_gfx950.h")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("scheme", og.SCHEMES)
def test_written_out_sweep_equals_autograd_through_the_restatement(scheme, ts):
    """G on all slices.  Bound: float64 over a few thousand operations per element, summed in another order than
    autograd's: 1e-12 of max|g| per tensor."""
    d, w, B = 3, (16, 9, 12), 7
    Ws, bs = cr.mlp_params(d, w, seed=8)
    g = np.random.default_rng(21)
    x = g.normal(size=(B, d))
    G = g.normal(size=(len(ts), B, d))
    _, gp64, gx64 = og.grads_for_upstream(Ws, bs, x, ts, G, scheme)
    gp, gx = og.reverse_sweep(Ws, bs, x, ts, G, scheme)
    for n, (a, b) in enumerate(zip(gp + [gx], gp64 + [gx64])):
        print(f"{scheme} tensor {n}: {_rel(a, b):.2e}")
        assert _rel(a, b) <= 1e-12


@pytest.mark.parametrize("scheme", og.SCHEMES)
def test_restatement_gradient_is_the_finite_difference_of_its_loss(scheme):
    d, w, B = 2, 16, 8
    Ws, bs = cr.smooth_mlp_params(d, w, seed=3)
    g = np.random.default_rng(5)
    x = torch.tensor(g.normal(size=(B, d)) * 0.8)
    G = torch.tensor(g.normal(size=(len(DOWN), B, d)))
    params = og.as_params(Ws, bs)

    def loss(ps):
        return (og.solve(ps, x, DOWN, scheme) * G).sum()
    grads = torch.autograd.grad(loss(params), params)
    step = 1e-5
    for k in range(5):
        dirs = [torch.tensor(g.normal(size=tuple(p.shape))) for p in params]
        with torch.no_grad():
            up = loss([p + step * u for p, u in zip(params, dirs)])
            dn = loss([p - step * u for p, u in zip(params, dirs)])
        fd = float(up - dn) / (2 * step)
        an = float(sum((q * u).sum() for q, u in zip(grads, dirs)))
        print(f"{scheme} direction {k}: fd {fd:.12e} autograd {an:.12e} rel {abs(fd - an) / abs(an):.2e}")
        assert abs(fd - an) <= 1e-6 * abs(an)


def test_restatement_at_one_point_and_last_slice_only():
    """n_t = 1: no step, the gradient of sum(G * x) is G[0] and no parameter moves; G on the last slice only is the
    endpoint loss."""
    Ws, bs = cr.mlp_params(2, 16, seed=4)
    g = np.random.default_rng(3)
    x, G = g.normal(size=(5, 2)), g.normal(size=(1, 5, 2))
    gp, gx = og.reverse_sweep(Ws, bs, x, np.array([0.3], np.float32), G, "rk4")
    assert np.array_equal(gx, G[0]) and all(np.all(q == 0.0) for q in gp)
    G = np.zeros((len(UP), 5, 2)); G[-1] = g.normal(size=(5, 2))
    _, gp64, gx64 = og.grads_for_upstream(Ws, bs, x, UP, G, "rk4")
    gp, gx = og.reverse_sweep(Ws, bs, x, UP, G, "rk4")
    for a, b in zip(gp + [gx], gp64 + [gx64]):
        assert _rel(a, b) <= 1e-12


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("scheme", og.SCHEMES)
def test_generic_path_equals_the_restatement(scheme, ts):
    d, w, B = 3, (33, 64, 48), 6
    Ws, bs = cr.mlp_params(d, w, seed=2)
    g = np.random.default_rng(11)
    xa = g.normal(size=(B, d))
    G = g.normal(size=(len(ts), B, d))
    traj64, gp64, gx64 = og.grads_for_upstream(Ws, bs, xa, ts, G, scheme)
    m = cr.make_mlp(Ws, bs, dtype=torch.float64)
    node = cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver=scheme)
    x = torch.tensor(xa, requires_grad=True)
    t_eval, traj = node(x, torch.tensor(ts))
    assert node.last_path == "generic" and traj.dtype == torch.float64 and tuple(traj.shape) == (len(ts), B, d)
    ps = [p for l in m._linears() for p in (l.weight, l.bias)]
    got = torch.autograd.grad((traj * torch.tensor(G)).sum(), ps + [x])
    assert _rel(traj.detach().numpy(), traj64) <= 1e-12
    for a, b in zip(got, gp64 + [gx64]):
        assert _rel(a.numpy(), b) <= 1e-12


def test_adaptive_solvers_are_refused():
    m = cfm_amd.MLP(dim=2, time_varying=True, w=16)
    for solver in ("dopri5", "tsit5"):
        with pytest.raises(NotImplementedError, match="euler.*midpoint.*rk4"):
            cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver=solver)
    with pytest.raises(NotImplementedError):
        cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver="heun")
    with pytest.raises(ValueError):
        cfm_amd.DifferentiableNeuralODE(torch_wrapper(m)).trajectory(torch.zeros(3, 2), torch.tensor([0.0, 0.5, 0.2]))


def test_header_and_binding_carry_the_new_entries():
    text = open(HEADER).read()
    for name, nargs in (("cfm_ode_fixed_grad_f32", 15), ("cfm_ode_fixed_grad_available", 2)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is ctypes.c_int
    assert re.search(r"#define CFM_OP_ODE_GRAD\s+12\b", text) and _lib.OP_ODE_GRAD == 12
    assert "#define CFM_ABI_VERSION 3" in text and _lib.ABI_VERSION == 3


def test_workspace_and_query_need_no_gpu():
    lib = _lib.load()
    for B, n_t in ((1, 1), (48, 9), (4101, 101), (100000, 2)):
        n = lib.cfm_workspace_bytes(_lib.OP_ODE_GRAD, B, n_t, 0)
        assert n > 0 and n % 256 == 0
        assert n == lib.cfm_workspace_bytes(_lib.OP_CNF_GRAD, B, n_t, 0)      # the same layout
    assert lib.cfm_workspace_bytes(_lib.OP_ODE_GRAD, 0, 5, 0) == 0

    def ask(*dims):
        return lib.cfm_ode_fixed_grad_available((ctypes.c_int * len(dims))(*dims), len(dims) - 1)
    assert ask(3, 64, 64, 64, 2) == 0 and ask(64, 33, 1, 48, 63) == 0
    assert ask(3, 65, 64, 64, 2) == -1 and ask(65, 64, 64, 64, 64) == -1 and ask(3, 64, 64, 2) == -1
    assert ask(3, 64, 0, 64, 2) == -1 and ask(3, 64, 64, 64, 3) == -1 and ask(1, 8, 8, 8, 0) == -1
    lib.cfm_ode_set_fused(0)
    try:
        assert ask(3, 64, 64, 64, 2) == -1
    finally:
        lib.cfm_ode_set_fused(1)
    assert ask(3, 64, 64, 64, 2) == 0
