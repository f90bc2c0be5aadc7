"""CPU: the gradient of the Euler CNF solve.  The float64 restatement (tests/cnf_train_restate.py) is pinned by finite
differences, then DifferentiableCNF's generic path is pinned against it and against the tutorial's own formulation
(examples/2D_tutorials/Maximum_likelihood_CNF_tutorial.ipynb cell 3: jacrev / vjp under vmap through nn.Sequential)."""
import numpy as np
import pytest
import torch

import cfm_amd
import cnf_restate as cr
import cnf_train_restate as tr

DOWN = np.linspace(1.0, 0.0, 5)                                # decreasing, uniform
UP = np.array([0.0, 0.07, 0.3, 0.35, 0.81, 1.0])               # increasing, non-uniform
ESTIMATORS = ("exact", "hutch_gaussian", "hutch_rademacher")


def _probe(estimator, B, d, seed):
    g = np.random.default_rng(seed)
    if estimator == "exact":
        return None
    if estimator == "hutch_gaussian":
        return g.normal(size=(B, d))
    return g.integers(0, 2, (B, d)).astype(np.float64) * 2 - 1


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _model_grads(m, loss, extra=()):
    lins = m._linears()
    ps = [p for l in lins for p in (l.weight, l.bias)]
    g = torch.autograd.grad(loss, ps + list(extra), allow_unused=True)
    return [np.zeros(tuple(p.shape)) if q is None else q.detach().cpu().double().numpy() for p, q in zip(ps + list(extra), g)]


# ---- the mathematics: finite differences of the restatement's own loss ----
@pytest.mark.parametrize("hutch", [False, True])
def test_restatement_gradient_is_the_finite_difference_of_its_loss(hutch):
    d, w, B = 2, 16, 8
    Ws, bs = cr.smooth_mlp_params(d, w, seed=3)
    g = np.random.default_rng(5)
    x = torch.tensor(g.normal(size=(B, d)) * 0.8)
    eps = torch.tensor(g.normal(size=(B, d))) if hutch else None
    params = tr.as_params(Ws, bs)
    loss = tr.nll(params, x, DOWN, eps)
    grads = torch.autograd.grad(loss, params)
    step = 1e-5
    for k in range(5):
        dirs = [torch.tensor(g.normal(size=tuple(p.shape))) for p in params]
        with torch.no_grad():
            up = tr.nll([p + step * u for p, u in zip(params, dirs)], x, DOWN, eps)
            dn = tr.nll([p - step * u for p, u in zip(params, dirs)], x, DOWN, eps)
        fd = float(up - dn) / (2 * step)
        an = float(sum((q * u).sum() for q, u in zip(grads, dirs)))
        print(f"direction {k}: fd {fd:.12e} autograd {an:.12e} rel {abs(fd - an) / abs(an):.2e}")
        assert abs(fd - an) <= 1e-6 * abs(an)


# ---- the reverse sweep the kernel runs, written out in float64 numpy, against autograd through the restatement ----
def _hand_sweep(Ws, bs, x_aug, ts, G, eps):
    """DESIGN.md 4.9 step by step: primal forward from y_n, per direction the tangents forward and their cotangents
    back, then the primal reverse.  No autograd anywhere.  Returns ([dW0, db0, ..., dW3, db3], d/dx_aug)."""
    W = [np.asarray(w, np.float64) for w in Ws]
    b = [np.asarray(v, np.float64) for v in bs]
    x_aug, G = np.asarray(x_aug, np.float64), np.asarray(G, np.float64)
    d = x_aug.shape[1] - 1
    Wy = [W[0][:, :d], W[1], W[2]]                       # what a tangent goes through (no time component)

    def hidden(y, t):
        hs, s, q = [np.concatenate([y, np.full((len(y), 1), t)], 1)], [], []
        for l in range(3):
            z = hs[l] @ W[l].T + b[l]
            neg = tr.SCALE * tr.ALPHA * np.exp(np.minimum(z, 0.0))
            s.append(np.where(z > 0, tr.SCALE, neg))
            q.append(np.where(z > 0, 0.0, neg))
            hs.append(np.where(z > 0, tr.SCALE * z, tr.SCALE * tr.ALPHA * np.expm1(np.minimum(z, 0.0))))
        return hs, s, q

    ys = [x_aug[:, 1:]]
    for n in range(len(ts) - 1):
        ys.append(ys[n] + (float(ts[n + 1]) - float(ts[n])) * (hidden(ys[n], float(ts[n]))[0][3] @ W[3].T + b[3]))
    c, a = G[:, 0], G[:, 1:].copy()
    dW, db = [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b]
    pairs = [(eps, eps)] if eps is not None else [(np.tile(np.eye(d)[k], (len(a), 1)),) * 2 for k in range(d)]
    for n in reversed(range(len(ts) - 1)):
        h = float(ts[n + 1]) - float(ts[n])
        hs, s, q = hidden(ys[n], float(ts[n]))
        sb = [np.zeros_like(v) for v in s]
        for tau, omega in pairs:
            T, U = [np.asarray(tau, np.float64)], []
            for l in range(3):
                U.append(T[l] @ Wy[l].T)
                T.append(s[l] * U[l])
            seed = -(h * c)[:, None] * np.asarray(omega, np.float64)          # d(-h c div)/d(W3 T3)
            dW[3] += seed.T @ T[3]
            Tb = seed @ W[3]
            for l in (2, 1, 0):
                sb[l] += Tb * U[l]
                Ub = s[l] * Tb
                dW[l][:, :T[l].shape[1]] += Ub.T @ T[l]
                Tb = Ub @ Wy[l]
        hb = (h * a) @ W[3]
        dW[3] += (h * a).T @ hs[3]
        db[3] += (h * a).sum(0)
        for l in (2, 1, 0):
            zb = hb * s[l] + sb[l] * q[l]
            dW[l] += zb.T @ hs[l]
            db[l] += zb.sum(0)
            hb = zb @ W[l]
        a = a + hb[:, :d]
    return [g for pair in zip(dW, db) for g in pair], np.concatenate([c[:, None], a], 1)


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
def test_written_out_sweep_equals_autograd_through_the_restatement(estimator, ts):
    """Bound: float64 (2^-53 relative per operation) over a few thousand operations per element, summed in another
    order than autograd's: 1e-12 of max|g| per tensor."""
    d, w, B = 3, 16, 7
    Ws, bs = cr.mlp_params(d, w, seed=8)
    g = np.random.default_rng(21)
    xa = np.concatenate([g.normal(size=(B, 1)), g.normal(size=(B, d))], 1)
    G = g.normal(size=(B, d + 1))
    eps = _probe(estimator, B, d, 23)
    _, gp64, gx64 = tr.grads_for_upstream(Ws, bs, xa, ts, G, eps)
    gp, gx = _hand_sweep(Ws, bs, xa, ts, G, eps)
    for n, (a, b) in enumerate(zip(gp + [gx], gp64 + [gx64])):
        print(f"tensor {n}: {_rel(a, b):.2e}")
        assert _rel(a, b) <= 1e-12


# ---- the tutorial's formulation, float64 ----
def _func_divergence(net, y, t, eps):
    """div of y -> net([y, t]) per row by torch.func through the module, the way cell 3 of the tutorial takes it: the
    diagonal of the per-sample reverse-mode Jacobian summed (exact), or one vector-Jacobian product against the row's
    probe, dotted with the probe again (Hutchinson)."""
    tcol = torch.full((1,), float(t), dtype=y.dtype)

    def one_row(p):
        return net(torch.cat([p, tcol]))

    if eps is None:
        jac = torch.vmap(torch.func.jacrev(one_row))(y)                 # [B, d, d]
        return jac.diagonal(dim1=1, dim2=2).sum(1)

    def probed(p, e):
        return (torch.func.vjp(one_row, p)[1](e)[0] * e).sum()
    return torch.vmap(probed)(y, eps)


def _notebook_solve(net, x_aug, ts, eps):
    """Euler steps of [l, y] with l' = -div, y' = net([y, t]) on the batch: the state layout of this library."""
    l, y = x_aug[:, 0], x_aug[:, 1:]
    for n in range(len(ts) - 1):
        h = float(ts[n + 1]) - float(ts[n])
        tcol = torch.full((y.shape[0], 1), float(ts[n]), dtype=y.dtype)
        v = net(torch.cat([y, tcol], 1))
        l = l - h * _func_divergence(net, y, ts[n], eps)
        y = y + h * v
    return torch.cat([l[:, None], y], 1)


def _sequential(Ws, bs):
    layers = []
    for k, (W, b) in enumerate(zip(Ws, bs)):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        lin.weight.data = torch.tensor(np.asarray(W, np.float64))
        lin.bias.data = torch.tensor(np.asarray(b, np.float64))
        layers.append(lin)
        if k < 3:
            layers.append(torch.nn.SELU())
    return torch.nn.Sequential(*layers)


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_generic_path_equals_restatement_and_notebook(estimator, ts):
    d, w, B = 2, 16, 6
    Ws, bs = cr.mlp_params(d, w, seed=2)
    g = np.random.default_rng(11)
    xa = np.concatenate([g.normal(size=(B, 1)), g.normal(size=(B, d))], 1)
    G = g.normal(size=(B, d + 1))
    eps = _probe(estimator, B, d, 13)
    out64, gp64, gx64 = tr.grads_for_upstream(Ws, bs, xa, ts, G, eps)

    m = cr.make_mlp(Ws, bs, dtype=torch.float64)
    cnf = cfm_amd.DifferentiableCNF(m, estimator=estimator, noise=None if eps is None else torch.tensor(eps))
    x = torch.tensor(xa, requires_grad=True)
    out = cnf.solve(x, torch.tensor(ts))
    assert cnf.last_path == "generic" and out.dtype == torch.float64
    got = _model_grads(m, (out * torch.tensor(G)).sum(), [x])
    assert _rel(out.detach().numpy(), out64) <= 1e-12
    for a, b in zip(got, gp64 + [gx64]):
        assert _rel(a, b) <= 1e-10

    net = _sequential(Ws, bs)
    xn = torch.tensor(xa, requires_grad=True)
    outn = _notebook_solve(net, xn, ts, None if eps is None else torch.tensor(eps))
    gn = torch.autograd.grad((outn * torch.tensor(G)).sum(), [p for p in net.parameters()] + [xn])
    for a, b in zip(got, gn):
        assert _rel(a, b.numpy()) <= 1e-10


@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
def test_generic_path_equals_restatement_at_mixed_widths(estimator):
    """Hidden widths (33, 64, 48): no two layers share a shape, so an exchanged pair of extents in the helpers
    (cnf_restate.mlp_params / make_mlp) or in the restatement would not pass.  The written-out sweep is the third
    statement of the same gradient."""
    d, w, B = 3, (33, 64, 48), 6
    Ws, bs = cr.mlp_params(d, w, seed=2)
    assert [W.shape for W in Ws] == [(33, d + 1), (64, 33), (48, 64), (d, 48)]
    assert [b.shape for b in bs] == [(33,), (64,), (48,), (d,)]
    g = np.random.default_rng(11)
    xa = np.concatenate([g.normal(size=(B, 1)), g.normal(size=(B, d))], 1)
    G = g.normal(size=(B, d + 1))
    eps = _probe(estimator, B, d, 13)
    out64, gp64, gx64 = tr.grads_for_upstream(Ws, bs, xa, UP, G, eps)
    assert [q.shape for q in gp64[0::2]] == [W.shape for W in Ws]

    m = cr.make_mlp(Ws, bs, dtype=torch.float64)
    assert [tuple(l.weight.shape) for l in m._linears()] == [W.shape for W in Ws]
    cnf = cfm_amd.DifferentiableCNF(m, estimator=estimator, noise=None if eps is None else torch.tensor(eps))
    x = torch.tensor(xa, requires_grad=True)
    out = cnf.solve(x, torch.tensor(UP))
    assert cnf.last_path == "generic" and out.dtype == torch.float64
    got = _model_grads(m, (out * torch.tensor(G)).sum(), [x])
    assert _rel(out.detach().numpy(), out64) <= 1e-12
    for a, b in zip(got, gp64 + [gx64]):
        assert _rel(a, b) <= 1e-10
    gp, gx = _hand_sweep(Ws, bs, xa, UP, G, eps)
    for a, b in zip(gp + [gx], gp64 + [gx64]):
        assert _rel(a, b) <= 1e-12


def test_int_width_helper_keeps_its_bits():
    """mlp_params(d, w) with an int is the seeded MLP(dim=d, time_varying=True, w=w), as before it took triples; the
    triple (w, w, w) creates the same layers in the same order, so it is the same net."""
    torch.manual_seed(7)
    want = [p.detach().numpy().copy() for p in cfm_amd.MLP(dim=3, time_varying=True, w=16).parameters()]
    after = torch.rand(1)
    Ws, bs = cr.mlp_params(3, 16, seed=7)
    assert torch.equal(torch.rand(1), after)
    Wt, bt = cr.mlp_params(3, (16, 16, 16), seed=7)
    for k in range(4):
        assert np.array_equal(Ws[k], want[2 * k]) and np.array_equal(bs[k], want[2 * k + 1])
        assert np.array_equal(Wt[k], Ws[k]) and np.array_equal(bt[k], bs[k])
    # make_mlp consumes the generator as it did: one MLP(w = the first hidden width) worth of initialisation
    Wm, bm = cr.mlp_params(3, (16, 5, 9), seed=7)
    draws = []
    for make in (lambda: cfm_amd.MLP(dim=3, time_varying=True, w=16), lambda: cr.make_mlp(Wt, bt), lambda: cr.make_mlp(Wm, bm)):
        torch.manual_seed(3)
        make()
        draws.append(torch.rand(1))
    assert torch.equal(draws[0], draws[1]) and torch.equal(draws[0], draws[2])


def test_nll_is_the_tutorial_loss():
    d, w, B = 2, 16, 6
    Ws, bs = cr.mlp_params(d, w, seed=4)
    x = np.random.default_rng(2).normal(size=(B, d))
    m = cr.make_mlp(Ws, bs, dtype=torch.float64)
    cnf = cfm_amd.DifferentiableCNF(m)
    loss = cnf.nll(torch.tensor(x), steps=4)
    params = tr.as_params(Ws, bs)
    want = tr.nll(params, torch.tensor(x), DOWN)
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    for a, b in zip(_model_grads(m, loss), torch.autograd.grad(want, params)):
        assert _rel(a, b.numpy()) <= 1e-10
    # the default grid is float32 for a float32 model, and the loss is finite
    m32 = cr.make_mlp(Ws, bs)
    l32 = cfm_amd.DifferentiableCNF(m32).nll(torch.tensor(x, dtype=torch.float32), steps=4)
    assert l32.dtype == torch.float32 and abs(float(l32.detach()) - float(want.detach())) <= 1e-4 * abs(float(want.detach()))


# ---- a random upstream gradient and its two special cases ----
def test_upstream_without_l_is_the_plain_euler_gradient_and_zero_gives_zeros():
    d, w, B = 3, 16, 5
    Ws, bs = cr.mlp_params(d, w, seed=6)
    g = np.random.default_rng(17)
    xa = np.concatenate([np.zeros((B, 1)), g.normal(size=(B, d))], 1)
    G = g.normal(size=(B, d + 1))
    G[:, 0] = 0.0
    m = cr.make_mlp(Ws, bs, dtype=torch.float64)
    cnf = cfm_amd.DifferentiableCNF(m)
    x = torch.tensor(xa, requires_grad=True)
    got = _model_grads(m, (cnf.solve(x, torch.tensor(UP)) * torch.tensor(G)).sum(), [x])

    # the plain Euler solve of y' = v, nothing else
    net = _sequential(Ws, bs)
    y0 = torch.tensor(xa[:, 1:], requires_grad=True)
    y = y0
    for n in range(len(UP) - 1):
        tcol = torch.full((B, 1), float(UP[n]), dtype=torch.float64)
        y = y + (float(UP[n + 1]) - float(UP[n])) * net(torch.cat([y, tcol], 1))
    want = torch.autograd.grad((y * torch.tensor(G[:, 1:])).sum(), list(net.parameters()) + [y0])
    for a, b in zip(got[:-1], want[:-1]):
        assert _rel(a, b.numpy()) <= 1e-10
    assert _rel(got[-1][:, 1:], want[-1].numpy()) <= 1e-10
    assert np.all(got[-1][:, 0] == 0.0)

    x = torch.tensor(xa, requires_grad=True)
    zero = _model_grads(m, (cnf.solve(x, torch.tensor(UP)) * torch.zeros(B, d + 1, dtype=torch.float64)).sum(), [x])
    for a in zero:
        assert np.all(a == 0.0)


# ---- refusals ----
def test_other_solvers_and_estimators_are_refused():
    m = cfm_amd.MLP(dim=2, time_varying=True, w=16)
    for solver in ("dopri5", "rk4", "midpoint", "tsit5"):
        with pytest.raises(NotImplementedError, match="Euler"):
            cfm_amd.DifferentiableCNF(m, solver=solver)
    with pytest.raises(NotImplementedError):
        cfm_amd.DifferentiableCNF(m, estimator="hutch_cauchy")


def test_wrong_probe_shape_is_refused():
    m = cfm_amd.MLP(dim=2, time_varying=True, w=16)
    x = torch.zeros(4, 3)
    for shape in ((2,), (1, 2), (4, 1), (4, 3)):
        cnf = cfm_amd.DifferentiableCNF(m, estimator="hutch_gaussian", noise=torch.ones(shape))
        with pytest.raises(ValueError, match="probe"):
            cnf.solve(x, torch.linspace(1, 0, 3))


def test_probe_is_drawn_once_per_solve_and_kept():
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=2, time_varying=True, w=16)
    cnf = cfm_amd.DifferentiableCNF(torch_wrapper_of(m), estimator="hutch_rademacher")
    x = torch.randn(5, 2)
    loss = cnf.nll(x, steps=3)
    e = cnf.last_noise
    assert tuple(e.shape) == (5, 2) and set(e.unique().tolist()) <= {-1.0, 1.0}
    fixed = cfm_amd.DifferentiableCNF(m, estimator="hutch_rademacher", noise=e)
    assert float(fixed.nll(x, steps=3).detach()) == float(loss.detach())


def torch_wrapper_of(m):
    from cfm_amd.utils import torch_wrapper
    return torch_wrapper(m)


def test_double_backward_of_the_hip_function_is_refused():
    if not torch.cuda.is_available():
        pytest.skip("the HIP autograd function needs a GPU")
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=2, time_varying=True, w=16).cuda()
    cnf = cfm_amd.DifferentiableCNF(m)
    loss = cnf.nll(torch.randn(8, 2, device="cuda"), steps=3)
    assert cnf.last_path == "hip"
    g = torch.autograd.grad(loss, list(m.parameters()), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        sum(q.sum() for q in g).backward()
