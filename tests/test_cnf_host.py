"""CPU: reverse-time integration on the generic path, the CNF module's layout / sign / estimators against a
restatement of the reference's CNF, and the argument checks (no GPU needed)."""
import numpy as np
import pytest
import torch

import cfm_oracle as oracle
import cnf_restate as R


class _NetField(torch.nn.Module):
    """f(t, x) = MLP.net([x, t]) on the CPU (the module graph: no HIP inference path involved)."""

    def __init__(self, m, sign=1.0):
        super().__init__()
        self.m, self.sign = m, sign

    def forward(self, t, x):
        tt = torch.as_tensor(t, dtype=x.dtype).reshape(1, 1).expand(x.shape[0], 1)
        if self.sign < 0:
            return -self.m.net(torch.cat([x, -tt], 1))
        return self.m.net(torch.cat([x, tt], 1))


def _mlp64(d=2, w=16, seed=3):
    Ws, bs = R.mlp_params(d, w, seed)
    return R.make_mlp(Ws, bs, dtype=torch.float64), Ws, bs


def test_generic_dopri5_reverse_time_returns_every_frame():
    """A decreasing t_span: one frame per point, equal to the forward solve of -f(-s, .) on -t_span."""
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64()
    torch.manual_seed(0)
    x = torch.randn(33, 2, dtype=torch.float64)
    ts = torch.linspace(1, 0, 5)
    node = NeuralODE(_NetField(m), solver="dopri5", atol=1e-6, rtol=1e-6)
    tr = node.trajectory(x, ts)
    assert tr.shape == (5, 33, 2)
    assert node.last_path == "generic"
    fwd = NeuralODE(_NetField(m, sign=-1.0), solver="dopri5", atol=1e-6, rtol=1e-6)
    tf = fwd.trajectory(x, -ts)
    assert torch.equal(tr, tf)
    assert (node.n_steps, node.nfe) == (fwd.n_steps, fwd.nfe)


def test_generic_euler_reverse_time_equals_transformed_system():
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64()
    x = torch.randn(9, 2, dtype=torch.float64)
    ts = torch.linspace(1, 0, 11)
    a = NeuralODE(_NetField(m), solver="euler").trajectory(x, ts)
    b = NeuralODE(_NetField(m, sign=-1.0), solver="euler").trajectory(x, -ts)
    assert a.shape == (11, 9, 2) and torch.equal(a, b)


@pytest.mark.parametrize("ts", [[0.0, 0.5, 0.4, 1.0], [1.0, 1.0, 0.0], [0.0, 0.3, 0.3]])
def test_non_monotone_t_span_raises_value_error(ts):
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64()
    for solver in ("euler", "dopri5"):
        with pytest.raises(ValueError):
            NeuralODE(_NetField(m), solver=solver).trajectory(torch.zeros(3, 2, dtype=torch.float64), torch.tensor(ts))


def test_unknown_estimator_raises():
    import cfm_amd
    m, _, _ = _mlp64()
    with pytest.raises(NotImplementedError):
        cfm_amd.CNF(m, estimator="hutch_laplace")


def test_cnf_layout_and_sign_float64():
    """Layout [B, 1 + d] and sign of model-comparison's CNF (column 0 = -tr J, then v), against the float64 field and
    its jacrev trace built independently in tests/cnf_restate.py."""
    import cfm_amd
    m, Ws, bs = _mlp64(d=3, w=24)
    torch.manual_seed(1)
    x = torch.randn(40, 4, dtype=torch.float64)
    t = 0.37
    ours = cfm_amd.CNF(m)(torch.tensor(t, dtype=torch.float64), x)
    ref = R.aug_field_np(Ws, bs)(t, x.numpy())
    assert ours.shape == (40, 4) and ours.dtype == torch.float64
    assert np.allclose(ours.numpy(), ref, rtol=1e-12, atol=1e-12)
    assert np.all(np.sign(ours[:, 0].numpy()) == -np.sign(R.divergence_f64(Ws, bs, t, x[:, 1:].numpy())[0]))


def test_hutchinson_with_basis_probes_sums_to_exact():
    import cfm_amd
    m, _, _ = _mlp64(d=3, w=24)
    torch.manual_seed(2)
    x = torch.randn(25, 4, dtype=torch.float64)
    t = torch.tensor(0.8, dtype=torch.float64)
    exact = cfm_amd.CNF(m)(t, x)
    acc = torch.zeros(25, dtype=torch.float64)
    for k in range(3):
        e = torch.zeros(25, 3, dtype=torch.float64); e[:, k] = 1
        out = cfm_amd.CNF(m, estimator="hutch_gaussian", noise=e)(t, x)
        assert torch.equal(out[:, 1:], exact[:, 1:])
        acc += out[:, 0]
    assert torch.allclose(acc, exact[:, 0], rtol=1e-12, atol=1e-12)


def test_probe_is_fixed_for_a_solve_and_exposed():
    import cfm_amd
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64(d=2, w=16)
    cnf = cfm_amd.CNF(m, estimator="hutch_rademacher")
    x = torch.cat([torch.zeros(7, 1, dtype=torch.float64), torch.randn(7, 2, dtype=torch.float64)], 1)
    torch.manual_seed(4)
    a = NeuralODE(cnf, solver="euler").trajectory(x, torch.linspace(1, 0, 4))
    e = cnf.last_noise
    assert e.shape == (7, 2) and set(e.unique().tolist()) <= {-1.0, 1.0}
    b = NeuralODE(cfm_amd.CNF(m, estimator="hutch_rademacher", noise=e), solver="euler").trajectory(x, torch.linspace(1, 0, 4))
    assert torch.equal(a, b)


def test_log_likelihood_generic_matches_oracle_dopri5_float64():
    """log p(x) on the generic path (CPU, float64) against the oracle's dopri5 on the reverse augmented field."""
    import cfm_amd
    m, Ws, bs = _mlp64(d=2, w=16)
    torch.manual_seed(5)
    x = torch.randn(12, 2, dtype=torch.float64)
    lp, z = cfm_amd.log_likelihood(m, x, atol=1e-6, rtol=1e-6, return_z=True)
    ts = np.array([1.0, 0.0], dtype=np.float32)
    y0 = np.concatenate([np.zeros((12, 1)), x.numpy()], 1)
    ref = oracle.dopri5_trajectory(R.reverse(R.aug_field_np(Ws, bs)), y0, -ts, 1e-6, 1e-6)[-1]
    z_ref = ref[:, 1:]
    lp_ref = -0.5 * (z_ref ** 2).sum(1) - np.log(2 * np.pi) - ref[:, 0]
    assert np.abs(z.numpy() - z_ref).max() <= 1e-6 * max(1.0, np.abs(z_ref).max())
    assert np.abs(lp.numpy() - lp_ref).max() <= 1e-6 * max(1.0, np.abs(lp_ref).max())


@pytest.mark.parametrize("shape", [(1, 2), (6, 2), (7, 3), (14,)])
def test_probe_of_the_wrong_shape_raises(shape):
    """A probe is one [B, d] draw: anything else (meant to broadcast, or from another batch) is refused before any
    evaluation (the kernels read one probe per row and column)."""
    import cfm_amd
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64(d=2, w=16)
    x = torch.cat([torch.zeros(7, 1, dtype=torch.float64), torch.randn(7, 2, dtype=torch.float64)], 1)
    cnf = cfm_amd.CNF(m, estimator="hutch_gaussian", noise=torch.ones(shape, dtype=torch.float64))
    with pytest.raises(ValueError):
        cnf(torch.tensor(0.5, dtype=torch.float64), x)
    for solver in ("euler", "dopri5"):
        with pytest.raises(ValueError):
            NeuralODE(cnf, solver=solver).trajectory(x, torch.linspace(1, 0, 3))
