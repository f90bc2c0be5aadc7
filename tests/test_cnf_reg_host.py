"""CPU: the regularised CNF solve (state [l, (e), (f), y]).  The float64 restatement (tests/cnf_reg_restate.py) is pinned
by the reference's own augmented field (tests/golden/cnf_reg_field.npz) and by finite differences of its own loss; the
written-out reverse sweep with the kernel's seeds is pinned by autograd through the restatement; RegularizedCNF's
generic path, split and loss are pinned by the restatement and by restatements of AugmentationModule.forward and
CNFLitModule.step."""
import os

import numpy as np
import pytest
import torch

import cfm_amd
import cnf_reg_restate as rr
import cnf_restate as cr
import cnf_train_restate as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnf_reg_field.npz")
DOWN = np.linspace(1.0, 0.0, 5)
UP = np.array([0.0, 0.07, 0.3, 0.35, 0.81, 1.0])
MASKS = {1: (0.3, 0.0), 2: (0.0, 0.7), 3: (0.3, 0.7)}          # reg_mask -> (squared_l2_reg, jacobian_frobenius_reg)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _inputs(d, w, B, mask, seed, hutch=False):
    Ws, bs = cr.mlp_params(d, w, seed)
    g = np.random.default_rng(seed)
    r = rr.n_reg(mask)
    xa = np.concatenate([g.normal(size=(B, 1 + r)) * 0.1, g.normal(size=(B, d))], 1)
    G = 0.5 + g.normal(size=(B, 1 + r + d))
    eps = g.normal(size=(B, d)) if hutch else None
    return Ws, bs, xa, G, eps


# ---- the reference's field ----
@pytest.mark.parametrize("case", [0, 1])
def test_restatement_is_the_reference_s_augmented_field(case):
    z = np.load(GOLDEN)
    Ws = [z[f"c{case}_W{l}"] for l in range(4)]
    bs = [z[f"c{case}_b{l}"] for l in range(4)]
    x, t, want = z[f"c{case}_x"], float(z[f"c{case}_t"]), z[f"c{case}_out"]
    assert want.shape == (len(x), 3 + x.shape[1]) and want.dtype == np.float64
    v, div, e, f = rr.field_all(tr.as_params(Ws, bs, False), torch.tensor(x), t)
    got = torch.cat([-div[:, None], e[:, None], f[:, None], v], 1).numpy()
    err = np.abs(got - want).max()
    print(f"case {case}: max abs difference {err:.2e}")
    assert err <= 1e-12


# ---- the mathematics ----
@pytest.mark.parametrize("mask", [1, 2, 3])
def test_restatement_gradient_is_the_finite_difference_of_its_loss(mask):
    d, w, B = 2, 16, 8
    Ws, bs = cr.smooth_mlp_params(d, w, seed=3)
    g = np.random.default_rng(5)
    r = rr.n_reg(mask)
    xa = torch.tensor(np.concatenate([np.zeros((B, 1 + r)), g.normal(size=(B, d)) * 0.8], 1))
    G = torch.tensor(0.5 + g.normal(size=(B, 1 + r + d)))
    params = tr.as_params(Ws, bs)
    loss = (rr.euler_solve(params, xa, DOWN, mask) * G).sum()
    grads = torch.autograd.grad(loss, params)
    step = 1e-5
    for k in range(5):
        dirs = [torch.tensor(g.normal(size=tuple(p.shape))) for p in params]
        with torch.no_grad():
            up = (rr.euler_solve([p + step * u for p, u in zip(params, dirs)], xa, DOWN, mask) * G).sum()
            dn = (rr.euler_solve([p - step * u for p, u in zip(params, dirs)], xa, DOWN, mask) * G).sum()
        fd = float(up - dn) / (2 * step)
        an = float(sum((q * u).sum() for q, u in zip(grads, dirs)))
        print(f"mask {mask} direction {k}: fd {fd:.12e} autograd {an:.12e} rel {abs(fd - an) / abs(an):.2e}")
        assert abs(fd - an) <= 1e-6 * abs(an)


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("mask,hutch", [(1, False), (2, False), (3, False), (1, True)])
@pytest.mark.parametrize("shape", [(2, 16, 7), (3, (9, 16, 5), 4), (1, 8, 5)], ids=str)
def test_written_out_reverse_sweep_is_autograd_through_the_restatement(shape, mask, hutch, ts):
    d, w, B = shape
    Ws, bs, xa, G, eps = _inputs(d, w, B, mask, seed=11, hutch=hutch)
    _, gp, gx = rr.grads_for_upstream(Ws, bs, xa, ts, G, mask, eps)
    hp, hx = rr.reverse_sweep(Ws, bs, xa, ts, G, mask, eps)
    for n, a, b in zip(["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dx"], hp + [hx], gp + [gx]):
        assert _rel(a, b) <= 1e-12, (n, _rel(a, b))


def test_columns_l_and_y_are_those_of_the_unregularised_restatement():
    Ws, bs, xa, G, eps = _inputs(2, 16, 6, 3, seed=2)
    params = tr.as_params(Ws, bs, False)
    out = rr.euler_solve(params, torch.tensor(xa), UP, 3)
    ref = tr.euler_solve(params, torch.tensor(xa[:, [0, 3, 4]]), UP)
    assert torch.equal(out[:, 3:], ref[:, 1:])
    assert float((out[:, 0] - ref[:, 0]).abs().max()) <= 1e-14          # the trace read off the full columns: other sums
    assert float((out[:, 1] - torch.tensor(xa[:, 1])).min()) > 0 and float((out[:, 2] - torch.tensor(xa[:, 2])).min()) > 0


# ---- RegularizedCNF: the generic path ----
def _cnf(Ws, bs, mask, dtype=torch.float64, **kw):
    m = cr.make_mlp(Ws, bs, dtype=dtype)
    e, f = MASKS[mask]
    return m, cfm_amd.RegularizedCNF(m, squared_l2_reg=e, jacobian_frobenius_reg=f, **kw)


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("mask,estimator", [(1, "exact"), (2, "exact"), (3, "exact"), (1, "hutch_gaussian"), (3, "hutch_gaussian")])
def test_generic_path_is_the_restatement_in_float64(mask, estimator, ts):
    d, w, B = 2, 16, 7
    Ws, bs, xa, G, eps = _inputs(d, w, B, mask, seed=4, hutch=estimator != "exact")
    m, cnf = _cnf(Ws, bs, mask, estimator=estimator, noise=None if eps is None else torch.tensor(eps))
    x = torch.tensor(xa, requires_grad=True)
    out = cnf.solve(x, torch.tensor(ts))
    assert cnf.last_path == "generic" and out.shape == (B, 1 + rr.n_reg(mask) + d)
    lins = m._linears()
    ps = [p for l in lins for p in (l.weight, l.bias)]
    got = torch.autograd.grad((out * torch.tensor(G)).sum(), ps + [x])
    want_out, gp, gx = rr.grads_for_upstream(Ws, bs, xa, ts, G, mask, eps)
    assert _rel(out.detach().numpy(), want_out) <= 1e-12
    for a, b in zip(got, gp + [gx]):
        assert _rel(a.numpy(), b) <= 1e-10


def test_names_coefficients_and_column_order():
    Ws, bs = cr.mlp_params(2, 16, 1)
    m = cr.make_mlp(Ws, bs)
    both = cfm_amd.RegularizedCNF(m, squared_l2_reg=0.1, jacobian_frobenius_reg=0.2)
    assert both.names == ["log_prob", "squared_L2", "jacobian_frobenius"] and both.reg_mask == 3
    assert torch.equal(both.coeffs, torch.tensor([1.0, 0.1, 0.2]))
    assert cfm_amd.RegularizedCNF(m, squared_l2_reg=0.1).names == ["log_prob", "squared_L2"]
    only_f = cfm_amd.RegularizedCNF(m, jacobian_frobenius_reg=0.2)
    assert only_f.names == ["log_prob", "jacobian_frobenius"] and only_f.reg_mask == 2
    none = cfm_amd.RegularizedCNF(m)
    assert none.names == ["log_prob"] and none.reg_mask == 0 and isinstance(none, cfm_amd.DifferentiableCNF)
    with pytest.raises(ValueError):
        cfm_amd.RegularizedCNF(m, squared_l2_reg=-1.0)
    with pytest.raises(ValueError):
        both.solve(torch.zeros(3, 3), torch.tensor([1.0, 0.0]))          # [B, 3 + d] needs at least 4 columns
    # column order: e sits before f, y behind both
    x = torch.cat([torch.zeros(4, 3), torch.randn(4, 2)], 1)
    out = both.solve(x, torch.tensor([0.0, 0.5, 1.0]))
    oe = cfm_amd.RegularizedCNF(m, squared_l2_reg=0.1).solve(x[:, [0, 1, 3, 4]], torch.tensor([0.0, 0.5, 1.0]))
    of = only_f.solve(x[:, [0, 2, 3, 4]], torch.tensor([0.0, 0.5, 1.0]))
    assert torch.allclose(out[:, [0, 1, 3, 4]], oe, rtol=0, atol=1e-6) and torch.allclose(out[:, [0, 2, 3, 4]], of, rtol=0, atol=1e-6)


def test_without_penalties_it_is_the_parent_class():
    Ws, bs = cr.mlp_params(2, 16, 1)
    m = cr.make_mlp(Ws, bs, dtype=torch.float64)
    x = torch.randn(5, 3, dtype=torch.float64)
    ts = torch.tensor(DOWN)
    assert torch.equal(cfm_amd.RegularizedCNF(m).solve(x, ts), cfm_amd.DifferentiableCNF(m).solve(x, ts))
    dl, reg, z = cfm_amd.RegularizedCNF(m).split(x)
    assert reg.shape == (1,) and float(reg) == 0.0 and torch.equal(dl, x[:, :1]) and torch.equal(z, x[:, 1:])


def test_what_goes_generic_on_the_cpu_and_in_float64():
    Ws, bs = cr.mlp_params(2, 16, 1)
    for dtype in (torch.float32, torch.float64):
        m, cnf = _cnf(Ws, bs, 3, dtype=dtype)
        cnf.solve(torch.zeros(3, 5, dtype=dtype), torch.tensor([1.0, 0.5, 0.0]))
        assert cnf.last_path == "generic"
    from cfm_amd.models import GradModel
    m = GradModel(cfm_amd.MLP(dim=2, out_dim=1, time_varying=True, w=16))
    cnf = cfm_amd.RegularizedCNF(m, squared_l2_reg=0.5)
    x = torch.randn(3, 4)
    out = cnf.solve(x, torch.tensor([1.0, 0.5]))
    assert cnf.last_path == "generic" and out.shape == (3, 4) and bool(torch.isfinite(out).all())
    v = m(torch.cat([x[:, 2:], torch.ones(3, 1)], 1)).detach()          # one step: y - v / 2, e + (-1/2) |v|^2
    assert torch.allclose(out[:, 2:].detach(), x[:, 2:] - 0.5 * v, rtol=0, atol=1e-6)
    assert torch.allclose(out[:, 1].detach(), x[:, 1] - 0.5 * (v * v).sum(1), rtol=0, atol=1e-6)
    assert all(p.grad is None for p in m.parameters())
    out.sum().backward()
    assert all(p.grad is not None for p in list(m.parameters())[:-1])  # the action's last bias has no gradient


# ---- split and loss against the reference's own statements ----
def _augmentation_forward(x, coeffs, aug_dims):
    """AugmentationModule.forward with cnf_estimator == "exact" (augmentation.py:206-210)"""
    delta_logprob, aug, x = x[:, :1], x[:, 1:aug_dims], x[:, aug_dims:]
    reg = aug * coeffs[1:].to(aug)
    if aug_dims == 1:
        reg = torch.zeros(1).type_as(x)
    return delta_logprob, reg, x


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_split_and_loss_are_the_reference_s(mask):
    """CNFLitModule.step for a single time point (cfm_module.py:1420-1454): one solve from t = 1 to t = 0, logprob =
    prior.log_prob(x) - delta_logprob with delta_logprob [B, 1] against a [B] prior term (a [B, B] broadcast whose mean
    is mean(prior) - mean(delta)), losses = [-mean(logprob)], regs = [-reg], and the means of the stacks."""
    from torch.distributions import MultivariateNormal
    d, B, steps = 2, 6, 4
    Ws, bs = cr.mlp_params(d, 16, 8)
    m, cnf = _cnf(Ws, bs, mask)
    g = np.random.default_rng(3)
    x = torch.tensor(g.normal(size=(B, d)))
    reg, nll = cnf.loss(x, steps=steps)
    coeffs = torch.tensor([1.0] + [c for c in MASKS[mask] if c > 0])
    a = 1 + rr.n_reg(mask)
    state = rr.euler_solve(tr.as_params(Ws, bs, False), torch.cat([torch.zeros(B, a, dtype=torch.float64), x], 1),
                           np.linspace(1.0, 0.0, steps + 1), mask)
    dl, rg, z = _augmentation_forward(state, coeffs, a)
    got = cnf.split(state)
    for p, q in zip(got, (dl, rg, z)):
        assert torch.equal(p, q)
    prior = MultivariateNormal(torch.zeros(d, dtype=torch.float64), torch.eye(d, dtype=torch.float64))
    logprob = prior.log_prob(z) - dl
    want_nll = torch.mean(torch.stack([-torch.mean(logprob)]))
    want_reg = torch.mean(torch.stack([-rg]))
    assert abs(float(nll) - float(want_nll)) <= 1e-12 * abs(float(want_nll))
    assert abs(float(reg) - float(want_reg)) <= 1e-12 * abs(float(want_reg))
    assert float(reg) > 0           # backward in time the integrals are negative, the reference negates them
