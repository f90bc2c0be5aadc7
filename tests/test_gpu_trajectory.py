"""GPU: cfm_amd.TrajectoryFlowMatcher on its fused path (cfm_traj_xt_ut_f32, csrc/traj.hip): interval select, gather
through the device-resident indices, interpolant, noise and leave-out rule in one launch.

linear : bit-equal to the NumPy float32 restatement (tests/trajectory_restate.py), and — with an exact coupling — to a
         loop of the existing public per-interval matcher calls under the same seeds.
spline : against scipy.interpolate.CubicSpline(bc_type="natural") in float64, per tensor
         max|got - scipy| / max|scipy| <= 1e-5."""
import numpy as np
import pytest
import torch

import trajectory_restate as rs

pytestmark = pytest.mark.gpu

SPLINE_BOUND = 1e-5


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _sb(sigma, couple=False):
    import cfm_amd
    fm = cfm_amd.SchrodingerBridgeConditionalFlowMatcher(sigma=sigma)
    if not couple:
        fm.ot_sampler = None
    return fm


def _t_select(B, T, leave, seed):
    """every admissible interval (the halved one first) while the batch has room, then random ones"""
    ks = [k for k in range(T - 1) if not (leave > 0 and k == leave)]
    if leave > 0:
        ks = [leave - 1] + ks
    g = np.random.RandomState(seed)
    return torch.from_numpy(np.concatenate([np.asarray(ks), g.choice(ks, size=B)])[:B].astype(np.int64))


# ------------------------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize("shape", [(1, 2, 1), (33, 3, 3), (257, 5, 5), (64, 4, 784), (256, 5, 100)])
@pytest.mark.parametrize("variant", ["icfm", "sb"])
@pytest.mark.parametrize("leaveout", [False, True])
def test_linear_fused_is_bit_equal_to_the_restatement(dev, shape, variant, leaveout):
    import cfm_amd
    B, T, d = shape
    if leaveout and T < 3:
        L = -1                                   # two slices have no interior one: the case runs without
    else:
        L = T - 2 if leaveout else -1
    torch.manual_seed(B + d)
    X = torch.randn(B, T, d, device=dev)
    sigma = 0.25
    fm = cfm_amd.ConditionalFlowMatcher(sigma) if variant == "icfm" else _sb(sigma)
    tfm = cfm_amd.TrajectoryFlowMatcher(fm, "linear", leaveout_timepoint=L)
    leave = L if L > 0 else 0
    ts = _t_select(B, T, leave, 1)
    t = torch.rand(B).to(dev)
    eps = torch.randn(B, d, device=dev)
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=t, eps=eps)
    assert tfm.last_path == "hip"
    assert xt.device == X.device and xt.dtype == torch.float32 and xt.shape == ut.shape == (B, d) and t_net.shape == (B,)
    sig_t = (sigma * torch.sqrt(t * (1 - t))).cpu().numpy() if variant == "sb" else None      # as the binding passes it
    wx, wu, wt = rs.linear(X.cpu().numpy(), ts.numpy(), t.cpu().numpy(), eps.cpu().numpy(), sigma, variant, leave, sigma_t=sig_t)
    assert np.array_equal(xt.cpu().numpy(), wx)
    assert np.array_equal(ut.cpu().numpy(), wu)
    assert np.array_equal(t_net.cpu().numpy(), wt)
    # not training: the left-out slice is an ordinary one again
    ts2 = _t_select(B, T, 0, 2)
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X, training=False, t_select=ts2, t=t, eps=eps)
    wx, wu, wt = rs.linear(X.cpu().numpy(), ts2.numpy(), t.cpu().numpy(), eps.cpu().numpy(), sigma, variant, 0, sigma_t=sig_t)
    assert tfm.last_path == "hip"
    assert np.array_equal(xt.cpu().numpy(), wx) and np.array_equal(ut.cpu().numpy(), wu) and np.array_equal(t_net.cpu().numpy(), wt)


@pytest.mark.parametrize("B", [64, 300])
@pytest.mark.parametrize("variant,L", [("icfm", -1), ("icfm", 2), ("sb", -1)])
def test_exact_coupling_equals_a_loop_of_the_public_matcher_calls(dev, B, variant, L):
    """B = 64: the one-workgroup solver; B = 300: the batched solver.  The loop is the single-cell notebook's form: one
    public sample_location_and_conditional_flow per interval, here fed the same t; its eps is what it drew."""
    import cfm_amd
    T, d = 5, 4
    g = torch.Generator().manual_seed(B)
    X = (torch.randn(B, T, d, generator=g) + 0.5 * torch.arange(T)[None, :, None]).to(dev)
    sigma = 0.5
    mk = (lambda: cfm_amd.ExactOptimalTransportConditionalFlowMatcher(sigma)) if variant == "icfm" else \
         (lambda: _sb(sigma, couple=True))
    leave = L if L > 0 else 0
    torch.manual_seed(9)
    t = torch.rand(B).to(dev)
    ts = _t_select(B, T, leave, 3)
    # the parent's interface, interval by interval
    fm = mk()
    np.random.seed(21)
    per = {}
    for k in range(T - 1):
        if leave and k == leave:
            continue
        k1 = k + 2 if (leave and k + 1 == leave) else k + 1
        per[k] = fm.sample_location_and_conditional_flow(X[:, k], X[:, k1], t=t, return_noise=True)
    tsd = ts.to(dev)
    eps = torch.stack([per[k][3] for k in sorted(per)])[torch.tensor([sorted(per).index(int(k)) for k in ts]), torch.arange(B)]
    want_x = torch.stack([per[int(k)][1][b] for b, k in enumerate(ts)])
    want_u = torch.stack([per[int(k)][2][b] for b, k in enumerate(ts)])
    if leave:
        want_u[tsd + 1 == leave] /= 2
    # the new call under the same NumPy seed
    tfm = cfm_amd.TrajectoryFlowMatcher(mk(), "linear", leaveout_timepoint=L)
    np.random.seed(21)
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=t, eps=eps)
    assert tfm.last_path == "hip"
    assert torch.equal(xt, want_x) and torch.equal(ut, want_u)
    want_t = torch.where(tsd + 1 == leave, t * 2, t) + tsd if leave else t + tsd
    assert torch.equal(t_net, want_t)
    # ... and the NumPy stream stands where the loop left it
    a = np.random.random_sample(3)
    np.random.seed(21)
    for k in per:
        np.random.random_sample(B)
    assert np.array_equal(a, np.random.random_sample(3))


# ------------------------------------------------------------------------------------------------------------ spline
@pytest.mark.parametrize("B,T,L,d", [(1, 2, -1, 1), (257, 2, -1, 3), (1, 3, -1, 784), (257, 3, -1, 1), (257, 8, -1, 784),
                                     (257, 32, -1, 3), (33, 32, -1, 784), (257, 6, 2, 5), (257, 33, 5, 3), (64, 4, 1, 100)])
def test_spline_fused_against_scipy(dev, B, T, L, d):
    import cfm_amd
    torch.manual_seed(T * d)
    X = torch.randn(B, T, d, device=dev) + 3.0
    sigma = 0.1
    tfm = cfm_amd.TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(sigma), "spline", leaveout_timepoint=L)
    leave = L if L > 0 else 0
    Tp = T - (1 if leave else 0)
    g = np.random.RandomState(T)
    head = [0, Tp - 2] + ([leave - 1] if leave else [])
    ts = torch.from_numpy(np.concatenate([head, g.randint(0, Tp - 1, size=B)])[:B].astype(np.int64))
    u = torch.rand(B)
    u[0] = 0.0
    if B > 1:
        u[1] = float(np.nextafter(np.float32(1), np.float32(0)))
    eps = torch.randn(B, d, device=dev)
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=u, eps=eps)
    assert tfm.last_path == "hip" and xt.shape == ut.shape == (B, d) and xt.dtype == torch.float32
    wx, wu, wt, _ = rs.spline(X.cpu().numpy(), ts.numpy(), u.numpy(), eps.cpu().numpy(), sigma, leave)
    figs = {n: rs.rel(a.cpu().numpy(), w) for n, a, w in (("xt", xt, wx), ("ut", ut, wu), ("t_net", t_net, wt))}
    print(f"spline hip B={B} T={T} L={L} d={d}: {figs}")
    assert all(v <= SPLINE_BOUND for v in figs.values()), figs
    # determinism: the same inputs give the same bits
    t2, x2, u2 = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=u, eps=eps)
    assert torch.equal(t2, t_net) and torch.equal(x2, xt) and torch.equal(u2, ut)


def test_spline_with_more_than_32_knots_reports_eager(dev):
    import cfm_amd
    B, T, d = 33, 33, 3
    torch.manual_seed(0)
    X = torch.randn(B, T, d, device=dev)
    tfm = cfm_amd.TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.1), "spline")
    ts = torch.arange(B) % (T - 1)
    u, eps = torch.rand(B), torch.randn(B, d, device=dev)
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=u, eps=eps)
    assert tfm.last_path == "eager" and xt.device == X.device
    wx, wu, wt, _ = rs.spline(X.cpu().numpy(), ts.numpy(), u.numpy(), eps.cpu().numpy(), 0.1)
    assert rs.rel(xt.cpu().numpy(), wx) <= SPLINE_BOUND and rs.rel(ut.cpu().numpy(), wu) <= SPLINE_BOUND
    assert rs.rel(t_net.cpu().numpy(), wt) <= SPLINE_BOUND
    # one slice left out while training: 32 knots, back on the fused path
    cfm_amd.TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.1), "spline", 7).sample_location_and_conditional_flow(X)


@pytest.mark.parametrize("L", [-1, 2])
def test_spline_on_the_chain_of_an_exact_coupling(dev, L):
    """B = 64: the knot values are sample_trajectory's output under the same seed; the spline through them is SciPy's"""
    import cfm_amd
    B, T, d = 64, 5, 3
    g = torch.Generator().manual_seed(12)
    X = (torch.randn(B, T, d, generator=g) + 0.4 * torch.arange(T)[None, :, None]).to(dev)
    fm = cfm_amd.ExactOptimalTransportConditionalFlowMatcher(0.05)
    tfm = cfm_amd.TrajectoryFlowMatcher(fm, "spline", leaveout_timepoint=L)
    leave = L if L > 0 else 0
    kn = rs.knots(T, leave)
    np.random.seed(4)
    traj = fm.ot_sampler.sample_trajectory(X[:, kn])
    after = np.random.random_sample(2)
    np.random.seed(4)
    chain = fm.ot_sampler._trajectory_indices(X[:, kn]).cpu().numpy()
    assert np.array_equal(traj, np.stack([X[:, s].cpu().numpy()[chain[q]] for q, s in enumerate(kn)], axis=1))
    assert any(not np.array_equal(chain[q], np.arange(B)) for q in range(1, len(kn)))
    ts = torch.arange(B) % (len(kn) - 1)
    u, eps = torch.rand(B), torch.randn(B, d, device=dev)
    np.random.seed(4)
    t_net, xt, ut = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=u, eps=eps)
    assert np.array_equal(after, np.random.random_sample(2))              # the NumPy stream of sample_trajectory
    assert tfm.last_path == "hip"
    wx, wu, wt, wtraj = rs.spline(X.cpu().numpy(), ts.numpy(), u.numpy(), eps.cpu().numpy(), 0.05, leave, chain=chain)
    assert np.array_equal(wtraj.astype(np.float32), traj)
    for got, want in ((xt, wx), (ut, wu), (t_net, wt)):
        assert rs.rel(got.cpu().numpy(), want) <= SPLINE_BOUND
    # sigma = 0 at u = 0: xt is the knot value itself, up to the rounding of a cubic with zero weights
    tfm0 = cfm_amd.TrajectoryFlowMatcher(cfm_amd.ExactOptimalTransportConditionalFlowMatcher(0.0), "spline", leaveout_timepoint=L)
    np.random.seed(4)
    _, x0, _ = tfm0.sample_location_and_conditional_flow(X, t_select=ts, t=torch.zeros(B), eps=eps)
    assert np.array_equal(x0.cpu().numpy(), traj[np.arange(B), ts.numpy()])


# ---------------------------------------------------------------------------------------------- draws, paths, training
def test_draws_follow_the_documented_order_on_the_gpu(dev):
    import cfm_amd
    B, T, d = 128, 5, 6
    X = torch.randn(B, T, d, device=dev)
    tfm = cfm_amd.TrajectoryFlowMatcher(cfm_amd.ConditionalFlowMatcher(0.1), "linear", leaveout_timepoint=2)
    torch.manual_seed(5)
    t_net, xt, ut, eps, (t_loc, ts) = tfm.sample_location_and_conditional_flow(X, return_noise=True, return_interval=True)
    torch.manual_seed(5)
    want = torch.randint(T - 2, size=(B,))
    want[want >= 2] += 1
    want_t = torch.rand(B)
    want_eps = torch.randn(B, d, device=dev)
    assert torch.equal(ts.cpu(), want) and torch.equal(t_loc.cpu(), want_t) and torch.equal(eps, want_eps)
    assert ts.device == X.device and not bool((ts == 2).any())
    # the same seeds, the same bits
    torch.manual_seed(5)
    again = tfm.sample_location_and_conditional_flow(X)
    assert all(torch.equal(a, b) for a, b in zip(again, (t_net, xt, ut)))


def test_paths_that_stay_eager_on_the_gpu(dev):
    import cfm_amd
    X = torch.randn(16, 4, 3, device=dev)
    fm = cfm_amd.ConditionalFlowMatcher(0.1)
    for interp in ("linear", "spline"):
        tfm = cfm_amd.TrajectoryFlowMatcher(fm, interp)
        tfm.sample_location_and_conditional_flow(X)
        assert tfm.last_path == "hip"
        t_net, xt, ut = tfm.sample_location_and_conditional_flow(X.double())
        assert tfm.last_path == "eager" and xt.dtype == torch.float64 and xt.device == X.device
        Xg = X.clone().requires_grad_(True)
        t_net, xt, ut = tfm.sample_location_and_conditional_flow(Xg)
        assert tfm.last_path == "eager"
        (xt.sum() + ut.sum()).backward()
        assert torch.isfinite(Xg.grad).all()
        # the two paths agree on the same draws (linear: bit for bit)
        ts, t, eps = torch.arange(16) % 3, torch.rand(16), torch.randn(16, 3, device=dev)
        a = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=t, eps=eps)
        b = tfm.sample_location_and_conditional_flow(Xg, t_select=ts, t=t, eps=eps)
        for p, q in zip(a, b):
            if interp == "linear":
                assert torch.equal(p, q.detach())
            else:
                assert rs.rel(p.cpu().numpy(), q.detach().cpu().numpy()) <= SPLINE_BOUND


def test_output_feeds_the_fused_training_steps(dev):
    import cfm_amd
    B, T, d = 256, 5, 5
    g = torch.Generator().manual_seed(1)
    X = (torch.randn(B, T, d, generator=g) + 0.5 * torch.arange(T)[None, :, None]).to(dev)
    np.random.seed(0); torch.manual_seed(0)
    for interp in ("linear", "spline"):
        tfm = cfm_amd.TrajectoryFlowMatcher(cfm_amd.ExactOptimalTransportConditionalFlowMatcher(0.1), interp, leaveout_timepoint=2)
        model = cfm_amd.MLP(dim=d, time_varying=True, w=64).to(dev)
        step = cfm_amd.RegressionStep(model, torch.optim.Adam(model.parameters(), 1e-3))
        t, xt, ut = tfm.sample_location_and_conditional_flow(X)
        assert tfm.last_path == "hip"
        loss = step(t, xt, ut)
        assert np.isfinite(float(loss))
    fm = cfm_amd.SchrodingerBridgeConditionalFlowMatcher(sigma=0.5)
    tfm = cfm_amd.TrajectoryFlowMatcher(fm, "linear", leaveout_timepoint=2)
    flow = cfm_amd.MLP(dim=d, time_varying=True, w=64).to(dev)
    score = cfm_amd.MLP(dim=d, time_varying=True, w=64).to(dev)
    opt = torch.optim.Adam(list(flow.parameters()) + list(score.parameters()), 1e-3)
    sf2m = cfm_amd.SF2MStep(flow, score, opt)
    t, xt, ut, eps, (t_loc, ts) = tfm.sample_location_and_conditional_flow(X, return_noise=True, return_interval=True)
    assert tfm.last_path == "hip"
    losses = sf2m(t, xt, ut, eps, fm.compute_lambda(t_loc))
    assert torch.isfinite(losses).all() and np.isfinite(float(sf2m.loss()))
