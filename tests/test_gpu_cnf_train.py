"""GPU: DifferentiableCNF on the HIP path (forward cfm_ode_fixed_cnf_mlp_f32 at Euler, backward cfm_cnf_euler_grad_f32)
against the float64 restatement of tests/cnf_train_restate.py, plus the properties the training loop relies on."""
import numpy as np
import pytest
import torch

import cfm_amd
import cnf_restate as cr
import cnf_train_restate as tr

pytestmark = pytest.mark.gpu

BOUND = 1e-5           # the project's fp32 bound: max|g_hip - g_64| / max|g_64| per gradient tensor
SHAPES = [(2, 64, 48, 8), (5, 48, 19, 5), (1, 16, 33, 3), (2, 64, 37, 8), (2, 64, 1, 4)]      # (d, w, B, steps)


def _grid(direction, steps):
    if direction == "down":
        return np.linspace(1.0, 0.0, steps + 1).astype(np.float32)
    w = 1.0 + 0.6 * np.sin(1.7 * np.arange(steps) + 0.3)          # 0 -> 1, non-uniform
    return np.concatenate([[0.0], np.cumsum(w) / w.sum()]).astype(np.float32)


def _case(d, w, B, steps, hutch, direction, seed=1, g_mean=0.5):
    """fp32 inputs (as float64 for the reference) and the reference gradients.  The rows within 1e-5 of a SELU kink
    somewhere along the float64 trajectory are dropped before anything runs: an fp32 evaluation may take the other
    branch there.  The random upstream gradient has mean g_mean.  With the default 0.5 no gradient tensor is a cancelled
    sum, and the bound (relative to max|g_64| of the tensor) is a scale for every one of them; g_mean = 0 is
    test_zero_mean_upstream_at_d1 below, which says what happens to the one-element db3 then."""
    Ws, bs = cr.mlp_params(d, w, seed)
    g = np.random.default_rng(seed)
    xa = np.concatenate([g.normal(size=(B, 1)) * 0.1, g.normal(size=(B, d))], 1).astype(np.float32)
    G = (g_mean + g.normal(size=(B, d + 1))).astype(np.float32)
    eps = g.normal(size=(B, d)).astype(np.float32) if hutch else None
    ts = _grid(direction, steps)
    keep = tr.kink_free_rows(Ws, bs, xa, ts, eps, tol=1e-5)
    dropped = int((~keep).sum())
    assert dropped <= B / 4, f"{dropped} of {B} rows within 1e-5 of a kink"
    xa, G = xa[keep], G[keep]
    eps = None if eps is None else eps[keep]
    out64, gp64, gx64 = tr.grads_for_upstream(Ws, bs, xa, ts, G, eps)
    return Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped


def _hip_grads(Ws, bs, xa, G, eps, ts, estimator):
    dev = torch.device("cuda")
    m = cr.make_mlp(Ws, bs, device=dev)
    cnf = cfm_amd.DifferentiableCNF(m, estimator=estimator, noise=None if eps is None else torch.tensor(eps, device=dev))
    x = torch.tensor(xa, device=dev, requires_grad=True)
    out = cnf.solve(x, torch.tensor(ts))
    lins = m._linears()
    ps = [p for l in lins for p in (l.weight, l.bias)]
    g = torch.autograd.grad((out * torch.tensor(G, device=dev)).sum(), ps + [x])
    return cnf, m, out.detach(), [q.detach().cpu().double().numpy() for q in g]


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


NAMES = ["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dx"]


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_w%d_B%d_n%d" % s)
def test_kernel_gradient_against_float64(shape, estimator, direction):
    d, w, B, steps = shape
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped = _case(d, w, B, steps, estimator != "exact", direction)
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, estimator)
    assert cnf.last_path == "hip"
    errs = {n: _rel(a, b) for n, a, b in zip(NAMES, got, gp64 + [gx64])}
    print(f"{shape} {estimator} {direction}: dropped {dropped}; " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.all(np.isfinite(out.cpu().numpy()))
    for k, v in errs.items():
        assert v <= BOUND, (k, v, errs)


ROUNDING = 2.0 ** -24       # one fp32 rounding, relative


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
def test_zero_mean_upstream_at_d1(estimator, direction):
    """The d = 1 case with a ZERO-mean random G.  db3 has one element there, sum_n h_n sum_rows a_{n+1}, and with a
    zero-mean G that sum cancels: on the increasing grid with the exact trace it is 0.0057 while the rows' terms add up
    to 20 in magnitude.  max|g_64| is then no scale for the error: torch's own fp32 autograd through the restatement is
    4.0e-5 of it from float64 on these inputs (computed on the CPU), and the kernel measured 1.3e-5 on the GPU, i.e.
    7e-8 absolute on terms of magnitude 20.  Rule: per tensor, with S = max over its elements of sum_rows |the row's
    contribution in float64|, the error may be the larger of the bound of every other test, 1e-5 max|g_64|, and
    2^-24 S: one fp32 rounding of every row's term, which no fp32 summation order avoids.  The second figure is the
    larger one only where S > 168 max|g_64|; the test asserts that this is never the case for a tensor other than db3,
    so every other tensor is held to 1e-5 as everywhere else."""
    d, w, B, steps = 1, 16, 33, 3
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped = _case(d, w, B, steps, estimator != "exact", direction, g_mean=0.0)
    S = [np.zeros_like(q) for q in gp64]
    for r in range(len(xa)):
        Gr = np.zeros_like(G)
        Gr[r] = G[r]
        for acc, q in zip(S, tr.grads_for_upstream(Ws, bs, xa, ts, Gr, eps)[1]):
            acc += np.abs(q)
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, estimator)
    assert cnf.last_path == "hip"
    for n, a, b, acc in zip(NAMES, got, gp64 + [gx64], S + [None]):
        scale = float(np.abs(b).max())
        err = float(np.abs(a - b).max())
        floor = 0.0 if acc is None else ROUNDING * float(acc.max())
        print(f"d1 zero-mean {estimator} {direction}: {n} err/max|g| {err / scale:.2e} max|g| {scale:.3e} "
              f"2^-24 S {floor:.2e} = {floor / scale:.2e} max|g|")
        if n != "db3":
            assert floor <= BOUND * scale, (n, floor, scale)
        assert err <= max(BOUND * scale, floor), (n, err, scale, floor)


@pytest.mark.parametrize("estimator", ["exact", "hutch_rademacher"])
def test_forward_value_is_the_sampler_s_bit_for_bit(estimator):
    from cfm_amd.ode import NeuralODE
    dev = torch.device("cuda")
    Ws, bs = cr.mlp_params(2, 64, 2)
    m = cr.make_mlp(Ws, bs, device=dev)
    torch.manual_seed(4)
    x = torch.randn(37, 3, device=dev)
    e = None if estimator == "exact" else (torch.randint(0, 2, (37, 2), device=dev).float() * 2 - 1)
    ts = torch.linspace(1, 0, 9)
    cnf = cfm_amd.DifferentiableCNF(m, estimator=estimator, noise=e)
    out = cnf.solve(x, ts)
    node = NeuralODE(cfm_amd.CNF(m, estimator=estimator, noise=e), solver="euler")
    want = node.trajectory(x, ts)[-1]
    assert cnf.last_path == "hip" and node.last_path == "hip"
    assert torch.equal(out.detach(), want)


def test_two_backward_calls_give_the_same_bits():
    Ws, bs, xa, G, eps, ts, *_ = _case(2, 64, 37, 8, True, "down")
    a = _hip_grads(Ws, bs, xa, G, eps, ts, "hutch_gaussian")[3]
    b = _hip_grads(Ws, bs, xa, G, eps, ts, "hutch_gaussian")[3]
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


def test_fused_path_off_runs_generic_and_agrees():
    from cfm_amd import _lib
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, _ = _case(2, 64, 37, 8, False, "down")
    hip = _hip_grads(Ws, bs, xa, G, eps, ts, "exact")
    assert hip[0].last_path == "hip"
    lib = _lib.load()
    lib.cfm_ode_set_fused(0)
    try:
        gen = _hip_grads(Ws, bs, xa, G, eps, ts, "exact")
    finally:
        lib.cfm_ode_set_fused(1)
    assert gen[0].last_path == "generic"
    for n, a, b, ref in zip(NAMES, hip[3], gen[3], gp64 + [gx64]):
        assert float(np.abs(a - b).max() / np.abs(ref).max()) <= BOUND, n


def _one_step(make_opt, path_off):
    """Parameters after one optimiser step on the NLL from fixed weights.  Adam's first step is lr g / (|g| + eps): with
    eps = 1e-3 its slope in g is at most lr / eps = 1, so a gradient error of 1e-5 max|g| moves a parameter by no more
    than that (with the default eps = 1e-8 the step is sign(g) and any element near zero would flip it)."""
    from cfm_amd import _lib
    dev = torch.device("cuda")
    Ws, bs = cr.mlp_params(2, 64, 5)
    m = cr.make_mlp(Ws, bs, device=dev)
    torch.manual_seed(9)
    x = torch.randn(48, 2, device=dev)
    opt = make_opt(m.parameters())
    cnf = cfm_amd.DifferentiableCNF(m)
    lib = _lib.load()
    if path_off:
        lib.cfm_ode_set_fused(0)
    try:
        opt.zero_grad()
        loss = cnf.nll(x, steps=8)
        loss.backward()
    finally:
        lib.cfm_ode_set_fused(1)
    assert cnf.last_path == ("generic" if path_off else "hip")
    opt.step()
    return [p.detach().cpu().double().numpy() for p in m.parameters()]


@pytest.mark.parametrize("which", ["adam", "fused_adam"])
def test_one_optimiser_step_matches_the_generic_path(which):
    kw = dict(lr=1e-3, eps=1e-3)
    mk = (lambda ps: torch.optim.Adam(ps, **kw)) if which == "adam" else (lambda ps: cfm_amd.FusedAdam(ps, **kw))
    want = _one_step(lambda ps: torch.optim.Adam(ps, **kw), path_off=True)
    got = _one_step(mk, path_off=False)
    for a, b in zip(got, want):
        assert float(np.abs(a - b).max() / np.abs(b).max()) <= 1e-5


def test_twenty_steps_of_the_tutorial_loop_lower_the_loss():
    from cfm_amd.utils import sample_moons
    dev = torch.device("cuda")
    torch.manual_seed(0)
    np.random.seed(0)
    m = cfm_amd.MLP(dim=2, time_varying=True).to(dev)
    cnf = cfm_amd.DifferentiableCNF(m)
    opt = torch.optim.Adam(m.parameters())
    held = sample_moons(64).to(dev)
    with torch.no_grad():
        before = float(cnf.nll(held, steps=8))
    for _ in range(20):
        opt.zero_grad()
        loss = cnf.nll(sample_moons(64).to(dev), steps=8)
        loss.backward()
        opt.step()
        assert cnf.last_path == "hip"
    with torch.no_grad():
        after = float(cnf.nll(held, steps=8))
    print(f"held-out NLL {before:.4f} -> {after:.4f}")
    assert np.isfinite(after) and after < before
