"""CPU: the float64 restatement of the action-matching loss and gradient (tests/action_matching_restate.py) against
torch.autograd on the reference's formulation and against central differences of its own loss; the generic path of
cfm_amd.action_matching_loss against the restatement."""
import numpy as np
import pytest
import torch

import action_matching_restate as R

DS = [1, 2, 5, 63]
CASES = [(d, w) for d in DS for w in R.WIDTHS]
IDS = ["d%d_w%s" % (d, "-".join(map(str, w))) for d, w in CASES]


def _case(d, widths, B=9, seed=3):
    Ws, bs = R.action_params(d, widths, seed)
    x0, x1, t, xt = R.draw(B, d, seed + 100)
    return Ws, bs, x0, x1, xt, t


@pytest.mark.parametrize("d,widths", CASES, ids=IDS)
def test_sweeps_equal_autograd_on_the_reference_formulation(d, widths):
    Ws, bs, x0, x1, xt, t = _case(d, widths)
    loss, grads = R.sweeps(Ws, bs, x0, x1, xt, t)
    lref, gref = R.autograd_loss_and_grads(Ws, bs, x0, x1, xt, t)
    assert abs(loss - lref) <= 1e-12 * max(1.0, abs(lref))
    assert gref[7] is None or not np.any(gref[7])           # autograd: the loss does not depend on b3
    assert grads[7].shape == (1,) and grads[7][0] == 0.0    # an exact zero
    for n, a, b in zip(R.NAMES[:7], grads, gref):
        assert a.shape == b.shape, n
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (n, np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("d,widths", CASES, ids=IDS)
def test_sweeps_equal_central_differences_of_their_own_loss(d, widths):
    """Central differences at h = 1e-6 on five elements of every tensor.  The loss is smooth between kinks (the case is the first
    seed whose pre-activations all stay 1e-4 away from one; a step of 1e-6 in one parameter moves a pre-activation by
    1e-6 times an activation or a weight, all below 10 here), its third derivative along a coordinate is O(1),
    so the truncation h^2 / 6 ~ 2e-13 is below the rounding 2^-53 |loss| / h ~ 1e-10; the bound is ten times that."""
    for seed in range(3, 40):
        Ws, bs, x0, x1, xt, t = _case(d, widths, seed=seed)
        if R.min_abs_preactivation(Ws, bs, x0, x1, xt, t).min() > 1e-4:
            break
    else:
        raise AssertionError("no seed below 40 keeps every pre-activation 1e-4 away from a kink")
    loss, grads = R.sweeps(Ws, bs, x0, x1, xt, t)
    W64 = [np.asarray(w, np.float64) for w in Ws]
    b64 = [np.asarray(v, np.float64) for v in bs]
    tensors = [p for l in range(4) for p in (W64[l], b64[l])]
    g = np.random.default_rng(5)
    h = 1e-6
    for n, p, gr in zip(R.NAMES, tensors, grads):
        flat = p.reshape(-1)
        for e in g.choice(flat.size, size=min(5, flat.size), replace=False):
            keep = flat[e]
            flat[e] = keep + h
            up = R.restated_loss(W64, b64, x0, x1, xt, t)
            flat[e] = keep - h
            dn = R.restated_loss(W64, b64, x0, x1, xt, t)
            flat[e] = keep
            fd = (up - dn) / (2 * h)
            assert abs(fd - gr.reshape(-1)[e]) <= 1e-9 * max(1.0, abs(loss)), (n, e, fd, gr.reshape(-1)[e])


@pytest.mark.parametrize("d,widths", [(2, (64, 64, 64)), (5, (33, 33, 33)), (1, (64, 17, 40))])
@pytest.mark.parametrize("wrap", [False, True])
def test_generic_path_on_cpu_float64_equals_the_restatement(d, widths, wrap):
    import cfm_amd
    from cfm_amd.models import GradModel
    Ws, bs, x0, x1, xt, t = _case(d, widths)
    m = R.make_action(Ws, bs, dtype=torch.float64)
    action = GradModel(m) if wrap else m
    T = lambda v: torch.from_numpy(np.asarray(v, np.float64))   # noqa: E731
    loss = cfm_amd.action_matching_loss(action, T(x0), T(x1), T(t), xt=T(xt))
    assert cfm_amd.action_matching_loss.last_path == "generic"
    assert loss.dim() == 0 and loss.dtype == torch.float64
    loss.backward()
    lref, gref = R.sweeps(Ws, bs, x0, x1, xt, t)
    assert abs(float(loss.detach()) - lref) <= 1e-12 * max(1.0, abs(lref))
    lins = m._linears()
    ps = [p for l in lins for p in (l.weight, l.bias)]
    for n, p, b in zip(R.NAMES[:7], ps, gref):
        assert np.abs(p.grad.numpy() - b).max() <= 1e-12 * np.abs(b).max(), n
    assert ps[7].grad is None or not bool(ps[7].grad.any())


def test_default_xt_is_the_reference_interpolant_and_t_may_be_a_column():
    import cfm_amd
    Ws, bs, x0, x1, xt, t = _case(2, (64, 64, 64))
    m = R.make_action(Ws, bs, dtype=torch.float64)
    T = lambda v: torch.from_numpy(np.asarray(v, np.float64))   # noqa: E731
    a = cfm_amd.action_matching_loss(m, T(x0), T(x1), T(t))
    tt = T(t)[:, None]
    b = cfm_amd.action_matching_loss(m, T(x0), T(x1), tt, xt=tt * T(x1) + (1 - tt) * T(x0))
    assert float(a.detach()) == float(b.detach())
    with pytest.raises(ValueError):
        cfm_amd.action_matching_loss(m, T(x0), T(x1), T(t)[:-1])
    with pytest.raises(ValueError):
        cfm_amd.action_matching_loss(m, T(x0), T(x1)[:-1], T(t))


def test_a_float32_cpu_call_is_generic_and_trains_with_adam():
    import cfm_amd
    torch.manual_seed(0)
    m = cfm_amd.MLP(dim=2, out_dim=1, time_varying=True)
    x0, x1, t = torch.randn(16, 2), torch.randn(16, 2) + 0.5, torch.rand(16)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in m.parameters()]
    loss = cfm_amd.action_matching_loss(m, x0, x1, t)
    assert cfm_amd.action_matching_loss.last_path == "generic"
    loss.backward()
    opt.step()
    moved = [not torch.equal(p.detach(), q) for p, q in zip(m.parameters(), before)]
    assert all(moved[:7]) and not moved[7]
