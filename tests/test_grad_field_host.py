"""CPU: the float64 restatement of the action-matching field (tests/grad_field_restate.py) against torch.autograd, the
no-grad repair of GradModel, the reverse-time identity the kernels rely on, and the dispatch envelope (no GPU needed)."""
import numpy as np
import pytest
import torch

import grad_field_restate as G

WIDTHS = [(64, 64, 64), (33, 33, 33), (64, 17, 40)]


def _x(B, d, seed):
    return 2.0 * np.random.default_rng(seed).standard_normal((B, d))


@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("d", [1, 2, 5])
def test_restatement_equals_autograd(d, widths):
    Ws, bs = G.action_params(d, widths, seed=d)
    x = _x(37, d, 10 + d)
    for t in (0.0, 0.37):
        v, lap = G.grad_field(Ws, bs, t, x, laplacian=True)
        va, lapa = G.autograd_field(Ws, bs, t, x, laplacian=True)
        assert np.abs(v - va).max() <= 1e-12 * np.abs(va).max(), (d, widths, t)
        assert np.abs(lap - lapa).max() <= 1e-12 * np.abs(lapa).max(), (d, widths, t)
        assert np.array_equal(v, G.grad_field(Ws, bs, t, x))
        # the magnitudes of the Hessian's terms bound its diagonal
        diag, mag = G.laplacian_terms(Ws, bs, t, x)
        assert np.all(np.abs(lap) <= diag * (1 + 1e-12)) and np.all(diag <= mag * (1 + 1e-12))


def test_time_column_negation_identity():
    """-v(-t, x) and -lap(-t, x) of the action net with W0[:, d] and W3 negated are v(t, x) and lap(t, x): what lets a
    decreasing t_span run as the forward solve of the negated net."""
    for d, widths in ((2, (64, 64, 64)), (5, (64, 17, 40))):
        Ws, bs = G.action_params(d, widths, seed=3)
        Wn, bn = G.negated_action_params(Ws, bs)
        x = _x(29, d, 4)
        v, lap = G.grad_field(Ws, bs, 0.37, x, laplacian=True)
        vn, lapn = G.grad_field(Wn, bn, -0.37, x, laplacian=True)
        assert np.array_equal(-vn, v) and np.array_equal(-lapn, lap)


def test_smooth_action_stays_off_the_kinks():
    Ws, bs = G.smooth_action_params(2, 64, seed=0)
    g = np.random.default_rng(1)
    x = g.uniform(-3, 3, (4096, 2))
    for t in (-1.0, -0.3, 0.0, 0.6, 1.0):
        _, zs = G._forward(Ws, bs, t, x)
        assert all(z.max() <= -0.15 for z in zs)


def test_gradmodel_under_no_grad_returns_the_gradient():
    """NeuralODE.trajectory runs under no_grad; the parent's GradModel raised there."""
    from cfm_amd.models import GradModel
    Ws, bs = G.action_params(2, (64, 64, 64), seed=0)
    gm = GradModel(G.make_action(Ws, bs, dtype=torch.float64))
    x = _x(11, 2, 5)
    inp = torch.from_numpy(np.concatenate([x, np.full((11, 1), 0.37)], 1))
    with torch.no_grad():
        out = gm(inp)
    assert not out.requires_grad and not inp.requires_grad
    ref = G.autograd_field(Ws, bs, 0.37, x)
    assert np.abs(out.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    # a time column that varies over the batch
    tt = np.linspace(0, 1, 11)
    with torch.no_grad():
        out = gm(torch.from_numpy(np.concatenate([x, tt[:, None]], 1)))
    ref = np.stack([G.grad_field(Ws, bs, tt[i], x[i:i + 1])[0] for i in range(11)])
    assert np.abs(out.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


def test_gradmodel_with_grad_keeps_create_graph():
    from cfm_amd.models import GradModel
    Ws, bs = G.action_params(2, (64, 64, 64), seed=1)
    gm = GradModel(G.make_action(Ws, bs, dtype=torch.float64))
    x = _x(7, 2, 6)
    inp = torch.from_numpy(np.concatenate([x, np.full((7, 1), 0.2)], 1))
    v = gm(inp)
    assert v.requires_grad
    lap = sum(torch.autograd.grad(v[:, k].sum(), inp, retain_graph=True)[0][:, k] for k in range(2))
    _, ref = G.grad_field(Ws, bs, 0.2, x, laplacian=True)
    assert np.abs(lap.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


def test_generic_trajectory_steps_the_repaired_field_on_the_cpu():
    """float64 CPU input: NeuralODE's generic path (under no_grad) against the restatement's Euler solve."""
    import cfm_oracle as oracle
    from cfm_amd.models import GradModel
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    Ws, bs = G.action_params(2, (64, 64, 64), seed=2, out_scale=8.0)
    node = NeuralODE(torch_wrapper(GradModel(G.make_action(Ws, bs, dtype=torch.float64))), solver="euler")
    x = _x(9, 2, 7)
    ts = torch.linspace(0, 1, 6)
    tr = node.trajectory(torch.from_numpy(x), ts).numpy()
    assert node.last_path == "generic" and node.nfe == 5
    ref = oracle.euler_trajectory(G.field_np(Ws, bs), x, ts.numpy())
    assert np.abs(tr - ref).max() <= 1e-12 * np.abs(ref).max()


def test_hip_action_envelope():
    import cfm_amd
    from cfm_amd.cnf import CNF
    from cfm_amd.models import GradModel
    ok = GradModel(cfm_amd.MLP(dim=2, out_dim=1, w=64, time_varying=True))
    assert ok.hip_action(2) is ok.action and ok.hip_action(3) is None and ok.hip_action(0) is None
    assert GradModel(G.make_action(*G.action_params(5, (64, 17, 40), 0))).hip_action(5) is not None
    assert GradModel(G.make_action(*G.action_params(63, (8, 8, 8), 0))).hip_action(63) is not None
    assert GradModel(G.make_action(*G.action_params(64, (8, 8, 8), 0))).hip_action(64) is None       # d + 1 > 64
    assert GradModel(cfm_amd.MLP(dim=2, out_dim=1, w=128, time_varying=True)).hip_action(2) is None
    assert GradModel(cfm_amd.MLP(dim=2, out_dim=2, w=64, time_varying=True)).hip_action(2) is None
    assert GradModel(cfm_amd.MLP(dim=3, out_dim=1, w=64, time_varying=False)).hip_action(2) is None
    assert GradModel(cfm_amd.MLP(dim=2, out_dim=1, w=64, time_varying=True).double()).hip_action(2) is None
    assert GradModel(torch.nn.Linear(3, 1)).hip_action(2) is None
    # CNF: the exact trace only
    assert CNF(ok, "exact").hip_grad(2) is ok.action and CNF(ok, "hutch_gaussian").hip_grad(2) is None
    assert CNF(ok, "exact").hip_mlp(2) is None
    assert CNF(cfm_amd.MLP(dim=2, w=64, time_varying=True)).hip_grad(2) is None
