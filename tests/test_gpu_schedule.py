"""GPU: noise schedules sigma(t) on the fused paths — the scheduled bridge matcher (cfm_sample_xt_ut_sched_f32), its
trajectory form (cfm_traj_xt_ut_f32, variant 4), and the SDE samplers stepping a schedule (cfm_sde_em_mlp_f32 /
cfm_sde_em_step_f32 with g(t_k) per step).

The bridge kernels are compared bit for bit with the class's own eager fp32 composition on the same device (a subclass
that restates one closed form takes that composition through the public calls); the samplers with each other, with the
eager scheme and with the scheme's exact variance."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCHEDULE_NAMES = ("constant", "linear", "cosine")


def _schedule(name):
    import cfm_amd
    return {"constant": lambda: cfm_amd.ConstantNoiseScheduler(0.7),
            "linear": lambda: cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0),
            "cosine": lambda: cfm_amd.CosineNoiseScheduler(0.3, 0.5)}[name]()


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


@pytest.fixture
def launches(monkeypatch):
    """counts the calls of the scheduled bridge kernel's binding"""
    from cfm_amd import conditional_flow_matching as cfmod
    seen = []
    real = cfmod._fused_xt_ut_sched

    def spy(*a, **k):
        seen.append(1)
        return real(*a, **k)
    monkeypatch.setattr(cfmod, "_fused_xt_ut_sched", spy)
    return seen


def _pair(name):
    """(the matcher, the same matcher on its eager composition: a subclass that restates one closed form)"""
    import cfm_amd

    class Restated(cfm_amd.ScheduledBridgeConditionalFlowMatcher):
        def compute_sigma_t(self, t):
            return self.schedule.sigma_t(t)
    return cfm_amd.ScheduledBridgeConditionalFlowMatcher(_schedule(name)), Restated(_schedule(name))


def _data(dev, B, d, seed, offset=False):
    g = torch.Generator().manual_seed(seed)
    if offset:      # every row 4 bytes off a 16-byte boundary
        mk = lambda: torch.randn(B * d + 1, generator=g).to(dev)[1:].view(B, d)
    else:
        mk = lambda: torch.randn(B, d, generator=g).to(dev)
    x0, x1 = mk(), mk() + 1.0
    t = torch.rand(B, generator=g).to(dev)
    i = torch.randperm(B, generator=g).to(dev)
    j = torch.randint(B, (B,), generator=g).to(dev)
    return x0, x1, t, (i, j)


def _check_bridge(fm, eager, launches, x0, x1, t, idx):
    n0 = len(launches)
    torch.manual_seed(11)
    _, xt, ut, eps = fm._sample(x0, x1, t, True, idx=idx)
    assert len(launches) == n0 + 1
    torch.manual_seed(11)
    _, wx, wu, weps = eager._sample(x0, x1, t, True, idx=idx)
    assert len(launches) == n0 + 1 and torch.equal(eps, weps)
    assert xt.shape == x0.shape and xt.dtype == torch.float32 and xt.device == x0.device
    assert torch.isfinite(xt).all() and torch.isfinite(ut).all()
    assert torch.equal(xt, wx), float((xt - wx).abs().max())
    assert torch.equal(ut, wu), float((ut - wu).abs().max())
    return xt, ut


# ----------------------------------------------------------------------------------------------------- bridge kernel
@pytest.mark.parametrize("shape", [(1, 4), (257, 4), (300, 5), (64, 784)])
@pytest.mark.parametrize("name", SCHEDULE_NAMES)
def test_bridge_kernel_is_bit_equal_to_the_eager_composition(dev, launches, name, shape):
    B, d = shape
    fm, eager = _pair(name)
    x0, x1, t, idx = _data(dev, B, d, seed=B + d)
    _check_bridge(fm, eager, launches, x0, x1, t, None)
    xt, _ = _check_bridge(fm, eager, launches, x0, x1, t, idx)
    # the flow at a given location, and the mean path
    given = xt + 0.25
    n0 = len(launches)
    u = fm.compute_conditional_flow(x0, x1, t, given)
    m = fm.compute_mu_t(x0, x1, t)
    assert len(launches) == n0 + 2
    assert torch.equal(u, eager._eager_compute_conditional_flow(x0, x1, t, given))
    assert torch.equal(m, eager._eager_compute_mu_t(x0, x1, t))
    assert torch.equal(fm.sample_xt(x0, x1, t, given), eager.sample_xt(x0, x1, t, given))


@pytest.mark.parametrize("name", SCHEDULE_NAMES)
def test_rows_off_the_16_byte_grid_take_the_scalar_path(dev, launches, name):
    B, d = 37, 8
    fm, eager = _pair(name)
    x0, x1, t, idx = _data(dev, B, d, seed=3, offset=True)
    assert x0.data_ptr() % 16 == 4 and x0.is_contiguous()
    _check_bridge(fm, eager, launches, x0, x1, t, None)
    xt, _ = _check_bridge(fm, eager, launches, x0, x1, t, idx)
    given = (xt + 0.5).flatten()
    given = torch.cat([given[:1], given])[1:].view(B, d)             # the given location off the grid too
    assert torch.equal(fm.compute_conditional_flow(x0, x1, t, given), eager._eager_compute_conditional_flow(x0, x1, t, given))


@pytest.mark.parametrize("name", SCHEDULE_NAMES)
def test_end_points_of_the_bridge_are_finite_and_equal_to_eager(dev, launches, name):
    B, d = 66, 4
    fm, eager = _pair(name)
    x0, x1, t, idx = _data(dev, B, d, seed=8)
    t[0], t[1], t[-2], t[-1] = 0.0, 1.0, 1.0, 0.0
    xt, ut = _check_bridge(fm, eager, launches, x0, x1, t, idx)
    assert torch.equal(xt[0], x0[idx[0][0]])
    assert torch.isfinite(fm.compute_lambda(t)).all()


@pytest.mark.parametrize("name", ["linear", "cosine"])
def test_public_call_with_the_exact_coupling(dev, launches, name):
    B, d = 300, 5
    fm, eager = _pair(name)
    x0, x1, _, _ = _data(dev, B, d, seed=5)
    np.random.seed(2); torch.manual_seed(2)
    a = fm.sample_location_and_conditional_flow(x0, x1, return_noise=True)
    assert len(launches) == 1
    np.random.seed(2); torch.manual_seed(2)
    b = eager.sample_location_and_conditional_flow(x0, x1, return_noise=True)
    assert len(launches) == 1 and len(a) == len(b) == 4
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # guided: the labels follow the pairing
    y0, y1 = torch.arange(B, device=dev), torch.arange(B, device=dev) + B
    np.random.seed(2); torch.manual_seed(2)
    t, xt, ut, g0, g1 = fm.guided_sample_location_and_conditional_flow(x0, x1, y0, y1)
    assert torch.equal(xt, a[1]) and torch.equal(ut, a[2]) and g0.shape == g1.shape == (B,)
    assert bool((g0 < B).all()) and bool((g1 >= B).all())
    # inputs that want a graph, and float64, keep the eager composition
    n0 = len(launches)
    np.random.seed(2); torch.manual_seed(2)
    c = fm.sample_location_and_conditional_flow(x0.double(), x1.double())
    assert c[1].dtype == torch.float64 and len(launches) == n0
    xg = x0.clone().requires_grad_(True)
    fm.sample_location_and_conditional_flow(xg, x1)[2].sum().backward()
    assert len(launches) == n0 and torch.isfinite(xg.grad).all()


def test_group_call_equals_single_calls(dev, launches):
    fm, _ = _pair("linear")
    batches = []
    for B, d, seed in ((64, 4, 1), (64, 4, 2), (33, 5, 3)):
        x0, x1, _, _ = _data(dev, B, d, seed)
        batches.append((x0, x1))
    np.random.seed(4); torch.manual_seed(4)
    group = fm.sample_location_and_conditional_flow_group(batches, return_noise=True)
    np.random.seed(4); torch.manual_seed(4)
    singles = [fm.sample_location_and_conditional_flow(x0, x1, return_noise=True) for x0, x1 in batches]
    assert len(launches) == 6
    for a, b in zip(group, singles):
        assert len(a) == len(b) == 4 and all(torch.equal(p, q) for p, q in zip(a, b))


def test_coupling_prefetcher_takes_the_matcher(dev, launches):
    """one worker executes in submission order: the same draws, the same bits as the synchronous calls"""
    from cfm_amd.prefetch import CouplingPrefetcher
    fm, _ = _pair("cosine")
    data = [_data(dev, 256, 8, seed)[:2] for seed in (1, 2, 3)]
    torch.manual_seed(7); np.random.seed(7)
    ref = [fm.sample_location_and_conditional_flow(a, b) for a, b in data]
    torch.manual_seed(7); np.random.seed(7)
    pre = CouplingPrefetcher(fm, dev, workers=1)
    got = [h.result() for h in [pre.submit(a, b) for a, b in data]]
    pre.close()
    torch.cuda.synchronize()
    assert len(launches) == 6
    for r, g in zip(ref, got):
        assert len(r) == len(g) == 3 and all(torch.equal(x, y) for x, y in zip(r, g))


# ------------------------------------------------------------------------------------------------ trajectory matcher
def _t_select(B, T, leave, seed):
    """every admissible interval (the halved one first) while the batch has room, then random ones"""
    ks = [k for k in range(T - 1) if not (leave > 0 and k == leave)]
    if leave > 0:
        ks = [leave - 1] + ks
    g = np.random.RandomState(seed)
    return torch.from_numpy(np.concatenate([np.asarray(ks), g.choice(ks, size=B)])[:B].astype(np.int64))


@pytest.mark.parametrize("shape", [(33, 3, 5), (64, 4, 8)])
@pytest.mark.parametrize("L", [-1, 1])
@pytest.mark.parametrize("name", ["linear", "cosine"])
def test_trajectory_matcher_equals_a_loop_of_the_public_matcher_calls(dev, name, L, shape):
    import cfm_amd
    B, T, d = shape
    g = torch.Generator().manual_seed(B)
    X = (torch.randn(B, T, d, generator=g) + 0.5 * torch.arange(T)[None, :, None]).to(dev)
    leave = L if L > 0 else 0
    torch.manual_seed(9)
    t = torch.rand(B).to(dev)
    ts = _t_select(B, T, leave, 3)
    fm = cfm_amd.ScheduledBridgeConditionalFlowMatcher(_schedule(name))
    np.random.seed(21)
    per = {}
    for k in range(T - 1):
        if leave and k == leave:
            continue
        k1 = k + 2 if (leave and k + 1 == leave) else k + 1
        per[k] = fm.sample_location_and_conditional_flow(X[:, k], X[:, k1], t=t, return_noise=True)
    tsd = ts.to(dev)
    order = sorted(per)
    eps = torch.stack([per[k][3] for k in order])[torch.tensor([order.index(int(k)) for k in ts]), torch.arange(B)]
    want_x = torch.stack([per[int(k)][1][b] for b, k in enumerate(ts)])
    want_u = torch.stack([per[int(k)][2][b] for b, k in enumerate(ts)])
    if leave:
        want_u[tsd + 1 == leave] /= 2
    tfm = cfm_amd.TrajectoryFlowMatcher(cfm_amd.ScheduledBridgeConditionalFlowMatcher(_schedule(name)), "linear",
                                        leaveout_timepoint=L)
    np.random.seed(21)
    t_net, xt, ut, e, (t_loc, sel) = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=t, eps=eps, return_noise=True,
                                                                              return_interval=True)
    assert tfm.last_path == "hip"
    assert torch.equal(xt, want_x) and torch.equal(ut, want_u)
    want_t = torch.where(tsd + 1 == leave, t * 2, t) + tsd if leave else t + tsd
    assert torch.equal(t_net, want_t) and torch.equal(t_loc, t) and torch.equal(sel, tsd) and torch.equal(e, eps)
    # without a coupling: the fused launch and the eager composition of the same call (an input that wants a graph)
    free = cfm_amd.ScheduledBridgeConditionalFlowMatcher(_schedule(name))
    free.ot_sampler = None
    tfree = cfm_amd.TrajectoryFlowMatcher(free, "linear", leaveout_timepoint=L)
    hip = tfree.sample_location_and_conditional_flow(X, t_select=ts, t=t, eps=eps)
    assert tfree.last_path == "hip"
    eager = tfree.sample_location_and_conditional_flow(X.clone().requires_grad_(True), t_select=ts, t=t, eps=eps)
    assert tfree.last_path == "eager"
    assert all(torch.equal(p, q.detach()) for p, q in zip(hip, eager))


def test_trajectory_output_feeds_the_sf2m_step(dev):
    import cfm_amd
    B, T, d = 256, 4, 5
    g = torch.Generator().manual_seed(1)
    X = (torch.randn(B, T, d, generator=g) + 0.5 * torch.arange(T)[None, :, None]).to(dev)
    np.random.seed(0); torch.manual_seed(0)
    fm = cfm_amd.ScheduledBridgeConditionalFlowMatcher(_schedule("cosine"))
    tfm = cfm_amd.TrajectoryFlowMatcher(fm, "linear", leaveout_timepoint=2)
    flow = cfm_amd.MLP(dim=d, time_varying=True, w=64).to(dev)
    score = cfm_amd.MLP(dim=d, time_varying=True, w=64).to(dev)
    sf2m = cfm_amd.SF2MStep(flow, score, torch.optim.Adam(list(flow.parameters()) + list(score.parameters()), 1e-3))
    t, xt, ut, eps, (t_loc, ts) = tfm.sample_location_and_conditional_flow(X, return_noise=True, return_interval=True)
    assert tfm.last_path == "hip"
    losses = sf2m(t, xt, ut, eps, fm.compute_lambda(t_loc))
    assert torch.isfinite(losses).all() and np.isfinite(float(sf2m.loss()))


# ------------------------------------------------------------------------------------------------------ SDE sampler
TS = [0.0, 0.13, 0.5, 1.0]          # refined by dt = 0.05 to 3 + 8 + 10 steps of three different sizes


def _two_fields(dev, d=2, w=64, seed=0):
    import cfm_amd
    torch.manual_seed(seed)
    return cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev), cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)


def _zero(*nets):
    for net in nets:
        for p in net.parameters():
            p.data.zero_()


@pytest.mark.parametrize("d,w,rev", [(2, 64, False), (2, 64, True), (5, 32, False), (50, 64, False)])
@pytest.mark.parametrize("name", ["linear", "cosine"])
def test_fused_sampler_is_bit_equal_to_the_launch_per_step_scheme(dev, name, d, w, rev):
    from cfm_amd.sde import FlowScoreSDE, sdeint
    from cfm_amd import _lib
    lib = _lib.load()
    glds0 = lib.cfm_mlp_get_glds()
    v, s = _two_fields(dev, d=d, w=w, seed=11 + d)
    x0 = torch.randn(300, d, generator=torch.Generator().manual_seed(d)).to(dev)
    ts = torch.tensor(TS)
    sde = FlowScoreSDE(v, s, sigma=_schedule(name), reverse=rev)
    gen = lambda: torch.Generator(device=dev).manual_seed(3)
    a = sdeint(sde, x0, ts, dt=0.05, generator=gen(), noise="torch", fused=True)
    assert sde.last_path == "hip"
    try:
        # the fused sampler sums k in the order of the register-staged layer core (cfm_mlp_set_glds(0)); the layers'
        # default engine has another fixed order: same trajectory within 1e-5
        lib.cfm_mlp_set_glds(0)
        b = sdeint(sde, x0, ts, dt=0.05, generator=gen(), noise="torch", fused=False)
        lib.cfm_mlp_set_glds(glds0)
        c = sdeint(sde, x0, ts, dt=0.05, generator=gen(), noise="torch", fused=False)
    finally:
        lib.cfm_mlp_set_glds(glds0)
    assert sde.last_path == "hip" and a.shape == b.shape == (4, 300, d)
    assert torch.equal(a.cpu(), b.cpu()), float((a.cpu() - b.cpu()).abs().max())
    assert float((a.cpu() - c.cpu()).abs().max()) <= 1e-5 * float(a.abs().max())
    # the schedule matters: a constant at its initial value gives another trajectory
    k = sdeint(FlowScoreSDE(v, s, sigma=float(_schedule(name)(0.5)), reverse=rev), x0, ts, dt=0.05, generator=gen(),
               noise="torch", fused=True)
    assert not torch.equal(a, k)


@pytest.mark.parametrize("name", ["linear", "cosine"])
def test_hip_sampler_equals_the_eager_scheme(dev, name):
    from cfm_amd.sde import FlowScoreSDE, sdeint
    schedule = _schedule(name)
    v, s = _two_fields(dev, seed=4)
    x0 = torch.randn(256, 2, generator=torch.Generator().manual_seed(1)).to(dev)
    ts = torch.tensor(TS)
    a = sdeint(FlowScoreSDE(v, s, sigma=schedule), x0, ts, dt=0.02, generator=torch.Generator(device=dev).manual_seed(7),
               noise="torch")

    class Eager(torch.nn.Module):          # same scheme through the generic (callable) path
        noise_type, sde_type = "diagonal", "ito"

        def f(self, t, y):
            x = torch.cat([y, t.repeat(y.shape[0])[:, None]], 1)
            with torch.no_grad():
                return v.net(x) + s.net(x)

        def g(self, t, y):
            return torch.ones_like(y) * schedule(t)
    b = sdeint(Eager(), x0, ts, dt=0.02, generator=torch.Generator(device=dev).manual_seed(7))
    assert a.shape == b.shape == (4, 256, 2)
    assert float((a.cpu() - b.cpu()).abs().max()) <= 2e-5 * float(b.abs().max())


@pytest.mark.parametrize("fused", [True, False])
def test_reverse_reads_g_at_the_solver_time(dev, fused):
    """Zero fields, y0 = 0, one step of h = 0.5 from t_0 = 0 in reverse: the kernel evaluates
    f = fma(1, s, -v) = 0;  r = fma(h, f, y0) = 0;  y1 = fma(gs, xi, r) = fl32(gs * xi)   with
    gs = fl32(double(g32) * sqrt(0.5)),  g32 = fl32 g(t_0 = 0) = 1 — not g(1 - t_0) = sqrt(0.1)."""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    schedule = _schedule("linear")
    v, s = _two_fields(dev, seed=2)
    _zero(v, s)
    B, d = 300, 2
    xi = torch.randn(1, B, d, generator=torch.Generator().manual_seed(5)).to(dev)
    y = sdeint(FlowScoreSDE(v, s, sigma=schedule, reverse=True), torch.zeros(B, d, device=dev), torch.tensor([0.0, 0.5]),
               dt=0.5, noise=xi, fused=fused)
    g32 = float(schedule(torch.as_tensor(0.0, dtype=torch.float32)))
    assert g32 == 1.0
    gs = torch.tensor(np.float32(g32 * math.sqrt(0.5)), device=dev)
    assert y.shape == (2, B, d)
    assert torch.equal(y[1] - y[0], gs * xi[0])
    other = torch.tensor(np.float32(float(schedule(torch.as_tensor(1.0, dtype=torch.float32))) * math.sqrt(0.5)), device=dev)
    assert not torch.equal(y[1] - y[0], other * xi[0])


def test_brownian_variance_is_the_scheme_sum(dev):
    """zero fields: Var(y_1 - y_0) = sum_k g(t_k)^2 h_k, the left Riemann sum of the scheme (F(1) is 0.8 % away)"""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    schedule = _schedule("linear")
    v, s = _two_fields(dev, seed=5)
    _zero(v, s)
    torch.manual_seed(123)
    y = sdeint(FlowScoreSDE(v, s, sigma=schedule), torch.zeros(40000, 2), torch.tensor([0.0, 1.0]), dt=0.01)
    inc = (y[-1] - y[0]).double()
    want = sum(float(schedule(torch.as_tensor(k / 100, dtype=torch.float32))) ** 2 * 0.01 for k in range(100))
    assert abs(want - schedule.F(1.0)) / schedule.F(1.0) > 0.005
    var = float(inc.var())
    print(f"Var = {var:.5f}, scheme {want:.5f}, F(1) {schedule.F(1.0):.5f}")
    assert abs(var - want) <= 0.025 * want and abs(float(inc.mean())) < 0.03


@pytest.mark.parametrize("reverse", [False, True])
def test_flow_solver_runs_the_hip_sampler(dev, reverse):
    from cfm_amd.sde import FlowScoreSDE, FlowSolver, sdeint
    from cfm_amd.utils import torch_wrapper
    schedule = _schedule("cosine")
    v, s = _two_fields(dev, d=3, w=32, seed=9)
    x0 = torch.randn(130, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    ts = torch.tensor(TS)
    fs = FlowSolver(torch_wrapper(v), 3, score_field=torch_wrapper(s), sigma=schedule, dt=0.05)
    a = fs.sdeint(x0, ts, reverse=reverse, generator=torch.Generator(device=dev).manual_seed(6))
    assert fs.last_path == "hip" and fs.nfe == 21
    sde = FlowScoreSDE(v, s, sigma=schedule, reverse=reverse)
    b = sdeint(sde, x0, ts, dt=0.05, generator=torch.Generator(device=dev).manual_seed(6))
    assert sde.last_path == "hip" and a.shape == (4, 130, 3)
    assert torch.equal(a, b)
    # a field pair that does not unwrap to two MLPs keeps the generic scheme
    gen = FlowSolver(lambda t, x: -x, 3, score_field=torch_wrapper(s), sigma=schedule, dt=0.05)
    out = gen.sdeint(x0, ts, generator=torch.Generator(device=dev).manual_seed(6))
    assert gen.last_path == "eager" and out.shape == (4, 130, 3) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------ one SF2M step
@pytest.mark.parametrize("name", ["linear", "cosine"])
def test_one_sf2m_step_end_to_end_against_float64_autograd(dev, name):
    """scheduled matcher -> SF2MStep(t, xt, ut, eps, FM.compute_lambda(t)): both losses and every gradient within 1e-5
    relative of float64 autograd on the same tensors (the bound of test_gpu_sf2m.py's float64 comparison)"""
    import cfm_amd
    B, d, w = 256, 2, 64
    torch.manual_seed(17); np.random.seed(17)
    flow = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    score = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    params = list(flow.parameters()) + list(score.parameters())
    x0 = torch.randn(B, d, device=dev)
    x1 = torch.randn(B, d, device=dev) * 0.5 + 2.0
    fm = cfm_amd.ScheduledBridgeConditionalFlowMatcher(_schedule(name))
    t, xt, ut, eps = fm.sample_location_and_conditional_flow(x0, x1, return_noise=True)
    lam = fm.compute_lambda(t)
    assert lam.shape == (B,) and torch.isfinite(lam).all()
    step = cfm_amd.SF2MStep(flow, score, cfm_amd.FusedAdam(params, lr=1e-3))
    losses = step.backward_only(t, xt, ut, eps, lam)
    f, s = copy.deepcopy(flow).double().cpu(), copy.deepcopy(score).double().cpu()
    for p in list(f.parameters()) + list(s.parameters()):
        p.grad = None
    x = torch.cat([xt.double().cpu(), t.double().cpu()[:, None]], dim=-1)
    fl = torch.mean((f.net(x) - ut.double().cpu()) ** 2)
    sl = torch.mean((lam.double().cpu()[:, None] * s.net(x) + eps.double().cpu()) ** 2)
    (fl + sl).backward()
    got_fl, got_sl = (float(z) for z in losses.cpu())
    want_fl, want_sl = float(fl.detach()), float(sl.detach())
    devs = [abs(got_fl - want_fl) / want_fl, abs(got_sl - want_sl) / want_sl]
    devs += [float((p.grad.double().cpu() - q.grad).abs().max() / q.grad.abs().max())
             for p, q in zip(params, list(f.parameters()) + list(s.parameters()))]
    print(f"{name}: losses {devs[0]:.2e} {devs[1]:.2e}, gradients max {max(devs[2:]):.2e}")
    assert max(devs) <= 1e-5, devs
    # and the full step moves the parameters
    before = [p.detach().clone() for p in params]
    out = step(t, xt, ut, eps, lam)
    assert torch.isfinite(out).all() and any(not torch.equal(a, p) for a, p in zip(before, params))
