"""CPU: cfm_amd.TrajectoryFlowMatcher on its eager path (CPU tensors) — multi-marginal flow matching on X [B, T, d],
runner/src/models/cfm_module.py:142-199, :225-242 (linear) and :1352-1409 (natural cubic spline).

linear : bit-equal to the NumPy float32 restatement (tests/trajectory_restate.py) with t_select, t, eps given.
spline : against scipy.interpolate.CubicSpline(bc_type="natural") in float64; per tensor max|got - scipy| / max|scipy|
         <= 1e-5 in float32 and <= 1e-12 in float64.
The couplings need the GPU, so the matchers here do not couple: ConditionalFlowMatcher, and the SB path with its
``ot_sampler`` set to None (what the reference's ``self.ot_sampler is not None`` tests)."""
import numpy as np
import pytest
import torch

import cfm_amd
import trajectory_restate as rs
from cfm_amd.trajectory import TrajectoryFlowMatcher, natural_spline_map


def _sb(sigma):
    fm = cfm_amd.SchrodingerBridgeConditionalFlowMatcher(sigma=sigma)
    fm.ot_sampler = None
    return fm


def _t_select(B, T, leave, seed):
    """every admissible interval, the one in front of the left-out slice (the halved one) first"""
    ks = [k for k in range(T - 1) if not (leave > 0 and k == leave)]
    if leave > 0:
        ks = [leave - 1] + ks
    g = np.random.RandomState(seed)
    return torch.from_numpy(np.concatenate([np.asarray(ks), g.choice(ks, size=B - len(ks))]).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize("variant", ["icfm", "sb"])
@pytest.mark.parametrize("L", [-1, 1, "T-2"])
@pytest.mark.parametrize("training", [True, False])
def test_linear_eager_is_bit_equal_to_the_restatement(variant, L, training):
    B, T, d = 37, 5, 3
    L = T - 2 if L == "T-2" else L
    torch.manual_seed(3)
    X = torch.randn(B, T, d)
    sigma = 0.3
    fm = cfm_amd.ConditionalFlowMatcher(sigma) if variant == "icfm" else _sb(sigma)
    tfm = TrajectoryFlowMatcher(fm, "linear", leaveout_timepoint=L)
    leave = L if (training and L > 0) else 0
    ts = _t_select(B, T, leave, 5)
    t, eps = torch.rand(B), torch.randn(B, d)
    t_net, xt, ut, e, (t_loc, t_sel) = tfm.sample_location_and_conditional_flow(
        X, training=training, return_noise=True, return_interval=True, t_select=ts, t=t, eps=eps)
    assert tfm.last_path == "eager"
    assert t_net.dtype == xt.dtype == ut.dtype == torch.float32 and xt.shape == ut.shape == (B, d) and t_net.shape == (B,)
    assert torch.equal(e, eps) and torch.equal(t_loc, t) and torch.equal(t_sel, ts)
    sig_t = (sigma * torch.sqrt(t * (1 - t))).numpy() if variant == "sb" else None
    wx, wu, wt = rs.linear(X.numpy(), ts.numpy(), t.numpy(), eps.numpy(), sigma, variant, leave, sigma_t=sig_t)
    assert np.array_equal(xt.numpy(), wx) and np.array_equal(ut.numpy(), wu) and np.array_equal(t_net.numpy(), wt)
    if leave:
        h = (ts + 1 == leave).numpy()
        assert h.any() and not h.all()
        # the halved rows span two slices: target halved, local time doubled (run:235-237)
        assert np.array_equal(t_net.numpy()[h], (t.numpy()[h] * np.float32(2)) + ts.numpy()[h].astype(np.float32))
        if variant == "icfm":
            assert np.array_equal(ut.numpy()[h], (X[:, leave + 1] - X[:, leave - 1]).numpy()[h] / np.float32(2))
    elif variant == "icfm":
        rb = torch.arange(B)
        assert torch.equal(ut, X[rb, ts + 1] - X[rb, ts])


def test_linear_flattens_trailing_dims_and_keeps_float64_and_grad():
    torch.manual_seed(0)
    X = torch.randn(6, 3, 2, 4, dtype=torch.float64, requires_grad=True)
    tfm = TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.1))
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X)
    assert xt.shape == ut.shape == (6, 2, 4) and xt.dtype == ut.dtype == t_net.dtype == torch.float64
    assert tfm.last_path == "eager"
    (xt.sum() + ut.sum()).backward()
    assert X.grad is not None and torch.isfinite(X.grad).all()


def test_subclassed_matcher_goes_through_its_override():
    class Mine(cfm_amd.ConditionalFlowMatcher):
        def compute_conditional_flow(self, x0, x1, t, xt):
            return 3 * (x1 - x0)

    X = torch.randn(5, 3, 2)
    tfm = TrajectoryFlowMatcher(Mine(0.0))
    ts = torch.tensor([0, 1, 0, 1, 1])
    _, _, ut = tfm.sample_location_and_conditional_flow(X, t_select=ts)
    rb = torch.arange(5)
    assert torch.equal(ut, 3 * (X[rb, ts + 1] - X[rb, ts])) and tfm.last_path == "eager"


# ------------------------------------------------------------------------------------------------------------ spline
def test_restatement_polynomial_form_is_scipys_own_evaluation():
    from scipy.interpolate import CubicSpline
    g = np.random.RandomState(0)
    X = g.randn(4, 6, 2)
    i = np.array([0, 2, 1, 3]); u = np.array([0.0, 0.3, 0.999, 0.5])
    xt, ut, t_net, traj = rs.spline(X, i, u, np.zeros((4, 2)), 0.0, leave=2)
    tau = np.array(rs.knots(6, 2), dtype=float)
    assert np.array_equal(traj, X[:, rs.knots(6, 2)])
    for b in range(4):
        cs = CubicSpline(tau, traj[b], bc_type="natural")
        assert np.allclose(xt[b], cs(t_net[b]), rtol=0, atol=1e-13) and np.allclose(ut[b], cs(t_net[b], 1), rtol=0, atol=1e-13)


@pytest.mark.parametrize("dtype,bound", [(torch.float32, 1e-5), (torch.float64, 1e-12)])
@pytest.mark.parametrize("T,L", [(2, -1), (3, -1), (32, -1), (6, 2), (4, 1), (33, 31), (40, -1)])
def test_spline_eager_against_scipy(dtype, bound, T, L):
    B, d = 19, 3
    torch.manual_seed(T)
    X = torch.randn(B, T, d, dtype=dtype)
    sigma = 0.2
    tfm = TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(sigma), "spline", leaveout_timepoint=L)
    leave = L if L > 0 else 0
    Tp = T - (1 if leave else 0)
    g = np.random.RandomState(T)
    head = [0, Tp - 2] + ([leave - 1] if leave else [])           # first and last interval, and the one across the gap
    ts = torch.from_numpy(np.concatenate([head, np.arange(Tp - 1), g.randint(0, Tp - 1, size=B)])[:B].astype(np.int64))
    u = torch.rand(B, dtype=dtype)
    u[0], u[1] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))      # u = 0, and u just under 1
    eps = torch.randn(B, d, dtype=dtype)
    t_net, xt, ut, (u_out, i_out) = tfm.sample_location_and_conditional_flow(X, return_interval=True, t_select=ts, t=u, eps=eps)
    assert tfm.last_path == "eager" and xt.dtype == dtype
    assert torch.equal(u_out, u) and torch.equal(i_out, ts)
    wx, wu, wt, _ = rs.spline(X.numpy(), ts.numpy(), u.numpy(), eps.numpy(), sigma, leave)
    figs = {n: rs.rel(a.numpy(), w) for n, a, w in (("xt", xt, wx), ("ut", ut, wu), ("t_net", t_net, wt))}
    print(f"spline eager {dtype} T={T} L={L}: {figs}")
    assert all(v <= bound for v in figs.values()), figs
    if leave:       # the interval across the gap has width 2 and no further rescaling
        gap = ts.numpy() == leave - 1
        assert gap.any()
        assert np.allclose(t_net.numpy()[gap], (leave - 1) + 2 * u.numpy()[gap], rtol=1e-6 if dtype == torch.float32 else 1e-14)
    if Tp == 2:     # two knots: the straight line; compare with the linear formula
        x0, x1, uu = X[:, 0].double(), X[:, -1].double(), u.double()[:, None]
        assert rs.rel(xt.numpy(), (uu * x1 + (1 - uu) * x0 + sigma * eps.double()).numpy()) <= bound
        assert rs.rel(ut.numpy(), (x1 - x0).numpy()) <= bound


def test_spline_not_training_keeps_every_slice():
    X = torch.randn(7, 5, 2, dtype=torch.float64)
    tfm = TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.0), "spline", leaveout_timepoint=2)
    ts = torch.tensor([0, 1, 2, 3, 3, 2, 1]); u = torch.rand(7, dtype=torch.float64)
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X, training=False, t_select=ts, t=u)
    wx, wu, wt, _ = rs.spline(X.numpy(), ts.numpy(), u.numpy(), np.zeros((7, 2)), 0.0, leave=0)
    assert rs.rel(xt.numpy(), wx) <= 1e-12 and rs.rel(ut.numpy(), wu) <= 1e-12 and rs.rel(t_net.numpy(), wt) <= 1e-12
    with pytest.raises(ValueError):          # while training there are only T' - 1 = 3 knot intervals
        tfm.sample_location_and_conditional_flow(X, training=True, t_select=ts, t=u)


@pytest.mark.parametrize("tau", [list(range(2)), list(range(3)), list(range(32)), [0, 1, 3, 4, 5], [0, 2, 3], [0, 1, 2, 4],
                                 [0.0, 0.5, 2.0, 2.25, 7.0]])
def test_second_derivative_map_is_scipys(tau):
    g = np.random.RandomState(len(tau))
    y = g.randn(len(tau), 5)
    S = natural_spline_map(tau)
    want = rs.second_derivatives(tau, y)
    assert S.shape == (len(tau), len(tau)) and S.dtype == np.float64
    assert np.abs(S @ y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(S.sum(1)).max() <= 1e-12 and not S[0].any() and not S[-1].any()
    assert natural_spline_map(tau) is S                                   # cached per knot vector


# -------------------------------------------------------------------------------------------------------- draw order
@pytest.mark.parametrize("interp", ["linear", "spline"])
@pytest.mark.parametrize("L", [-1, 2])
@pytest.mark.parametrize("training", [True, False])
def test_draw_order_is_randint_then_rand_on_the_cpu_generator(interp, L, training):
    B, T, d = 64, 5, 2
    X = torch.randn(B, T, d)
    tfm = TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.1), interp, leaveout_timepoint=L)
    np.random.seed(11)
    state = np.random.get_state()
    torch.manual_seed(42)
    t_net, xt, ut, eps, (t_loc, t_sel) = tfm.sample_location_and_conditional_flow(X, training=training, return_noise=True,
                                                                                  return_interval=True)
    torch.manual_seed(42)
    leave = L if (training and L > 0) else 0
    if interp == "linear":
        want = torch.randint(T - 2 if leave else T - 1, size=(B,))
        if leave:
            want[want >= leave] += 1
            assert not bool((t_sel == leave).any())               # interval L is never selected while training
            assert bool((t_sel == leave - 1).any()) and bool((t_sel > leave).any())
    else:
        want = torch.randint((T - 1 if leave else T) - 1, size=(B,))
    want_t = torch.rand(B)
    want_eps = torch.randn(B, d)
    assert torch.equal(t_sel, want) and torch.equal(t_loc, want_t) and torch.equal(eps, want_eps)
    # without a coupling the NumPy stream is untouched
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    X = torch.randn(8, 5, 2)
    with pytest.raises(ValueError) as ei:
        TrajectoryFlowMatcher(cfm_amd.TargetConditionalFlowMatcher(0.1))
    for name in ("ConditionalFlowMatcher", "ExactOptimalTransportConditionalFlowMatcher", "SchrodingerBridgeConditionalFlowMatcher"):
        assert name in str(ei.value)
    with pytest.raises(ValueError):
        TrajectoryFlowMatcher(cfm_amd.VariancePreservingConditionalFlowMatcher(0.1))
    with pytest.raises(ValueError):
        TrajectoryFlowMatcher(object())
    with pytest.raises(ValueError):
        TrajectoryFlowMatcher(cfm_amd.SchrodingerBridgeConditionalFlowMatcher(0.5), "spline")
    with pytest.raises(ValueError):
        TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.1), "cubic")
    fm = cfm_amd.ConditionalFlowMatcher(0.1)
    for interp in ("linear", "spline"):
        for L in (0, 4, 5, -2):           # 0, T - 1, T and a negative that is not -1
            with pytest.raises(ValueError):
                TrajectoryFlowMatcher(fm, interp, leaveout_timepoint=L).sample_location_and_conditional_flow(X)
        for L in (1, 3):                  # 1 and T - 2 are the admissible ends
            TrajectoryFlowMatcher(fm, interp, leaveout_timepoint=L).sample_location_and_conditional_flow(X)
        tfm = TrajectoryFlowMatcher(fm, interp)
        with pytest.raises(ValueError):
            tfm.sample_location_and_conditional_flow(torch.randn(8, 1, 2))       # T = 1
        with pytest.raises(ValueError):
            tfm.sample_location_and_conditional_flow(torch.randn(8, 2))          # no time axis
        for kw in ({"t_select": torch.zeros(7, dtype=torch.int64)}, {"t": torch.rand(9)}, {"eps": torch.randn(7, 2)},
                   {"eps": torch.randn(8, 3)}, {"t_select": torch.full((8,), 4)}, {"t_select": torch.full((8,), -1)},
                   {"t_select": torch.rand(8)}):
            with pytest.raises(ValueError):
                tfm.sample_location_and_conditional_flow(X, **kw)
    with pytest.raises(ValueError):       # the left-out interval cannot be asked for while training
        TrajectoryFlowMatcher(fm, "linear", 2).sample_location_and_conditional_flow(X, t_select=torch.full((8,), 2))
    TrajectoryFlowMatcher(fm, "linear", 2).sample_location_and_conditional_flow(X, training=False, t_select=torch.full((8,), 2))


def test_exported_from_the_package():
    assert cfm_amd.TrajectoryFlowMatcher is TrajectoryFlowMatcher
    assert TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.0)).last_path is None
