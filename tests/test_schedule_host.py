"""CPU: noise schedules sigma(t) for SF2M (cfm_amd.schedule), the scheduled bridge matcher's closed forms on its eager
path, the step records the SDE sampler is handed for a schedule, and the refusals.  No GPU needed."""
import math
import struct

import numpy as np
import pytest
import torch

import cfm_amd
from cfm_amd import sde as sde_mod
from cfm_amd.sde import FlowScoreSDE, FlowSolver, sdeint

SCHEDULES = {
    "constant": lambda: cfm_amd.ConstantNoiseScheduler(0.7),
    "linear": lambda: cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0),
    "cosine": lambda: cfm_amd.CosineNoiseScheduler(0.3, 0.5),
}


@pytest.fixture(params=sorted(SCHEDULES))
def schedule(request):
    return SCHEDULES[request.param]()


def _matcher(schedule):
    return cfm_amd.ScheduledBridgeConditionalFlowMatcher(schedule)


# ------------------------------------------------------------------------------------------------------- schedules
def test_the_four_names_are_exported():
    for name in ("NoiseScheduler", "ConstantNoiseScheduler", "LinearDecreasingNoiseScheduler", "CosineNoiseScheduler"):
        assert issubclass(getattr(cfm_amd, name), cfm_amd.NoiseScheduler)


def test_F_is_the_integral_of_g_squared(schedule):
    g = torch.Generator().manual_seed(0)
    t = torch.rand(64, dtype=torch.float64, generator=g).requires_grad_(True)
    (dF,) = torch.autograd.grad(schedule.F(t).sum(), t)
    err = float((dF - schedule(t.detach()) ** 2).abs().max())
    print(f"{type(schedule).__name__}: max |dF/dt - g^2| = {err:.2e}")
    assert err <= 1e-12
    assert schedule.F(0.0) == 0 and schedule.F(0) == 0
    assert float(schedule.F(torch.zeros((), dtype=torch.float64))) == 0.0
    assert torch.equal(schedule.F(torch.zeros(3, dtype=torch.float64)), torch.zeros(3, dtype=torch.float64))
    # the variance of the bridge vanishes at both ends
    bound = 1e-7 * math.sqrt(schedule.F(1.0))
    for end in (0.0, 1.0):
        assert abs(schedule.sigma_t(end)) <= bound
        assert abs(float(schedule.sigma_t(torch.tensor(end, dtype=torch.float64)))) <= bound
        assert float(schedule.sigma_t(torch.full((2,), end, dtype=torch.float64)).abs().max()) <= bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_schedules_take_numbers_scalars_and_vectors(schedule, dtype):
    tol = 1e-6 if dtype == torch.float32 else 1e-14
    for fn in (schedule, schedule.F, schedule.sigma_t):
        want = [fn(0.25), fn(0.5)]
        assert all(isinstance(w, float) for w in want)
        s = fn(torch.tensor(0.25, dtype=dtype))
        v = fn(torch.tensor([0.25, 0.5], dtype=dtype))
        assert s.shape == () and s.dtype == dtype and v.shape == (2,) and v.dtype == dtype
        assert abs(float(s) - want[0]) <= tol * max(1.0, abs(want[0]))
        assert np.abs(v.double().numpy() - np.asarray(want)).max() <= tol * max(1.0, max(abs(w) for w in want))
    # a Python integer end point (the reference's cosine schedule fails on F(1))
    assert schedule.F(1) == pytest.approx(schedule.F(1.0), rel=1e-15) and schedule.F(1) > 0
    assert schedule(1) == pytest.approx(schedule(1.0), rel=1e-15)


def test_closed_forms_of_the_three_schedules():
    c, l, k = SCHEDULES["constant"](), SCHEDULES["linear"](), SCHEDULES["cosine"]()
    assert c(0.3) == 0.7 and c.F(0.5) == pytest.approx(0.245, rel=1e-15)
    assert l(0.0) == 1.0 and l(1.0) == pytest.approx(math.sqrt(0.1)) and l.F(1.0) == pytest.approx(0.55, rel=1e-15)
    assert k(0.0) == pytest.approx(0.3) and k(0.5) == pytest.approx(1.3)
    # F(1) = 3 s^2 / 2 + 2 s m + m^2
    assert k.F(1.0) == pytest.approx(1.5 * 0.25 + 2 * 0.5 * 0.3 + 0.09, rel=1e-14)


# ---------------------------------------------------------------------------------------------------------- matcher
def _batch(B=64, d=5, seed=1):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, d, dtype=torch.float64, generator=g)
    x1 = torch.randn(B, d, dtype=torch.float64, generator=g) + 1.0
    t = 0.1 + 0.8 * torch.rand(B, dtype=torch.float64, generator=g)
    eps = torch.randn(B, d, dtype=torch.float64, generator=g)
    return x0, x1, t, eps


def test_conditional_flow_is_the_time_derivative_of_xt(schedule):
    """the only difference is the 1e-8 guard of a(t): relative effect 1e-8 / (2 sigma_t^2) <= 4.2e-7 on these inputs"""
    fm = _matcher(schedule)
    x0, x1, t, eps = _batch()
    assert float(schedule.sigma_t(t).min()) ** 2 >= 0.0119
    xt, dxdt = torch.func.jvp(lambda tt: fm.sample_xt(x0, x1, tt, eps), (t,), (torch.ones_like(t),))
    ut = fm.compute_conditional_flow(x0, x1, t, xt)
    err, scale = float((ut - dxdt).abs().max()), float(dxdt.abs().max())
    print(f"{type(schedule).__name__}: max |ut - dx/dt| = {err:.2e} on {scale:.2e}")
    assert err <= 1e-6 * scale


def test_constant_schedule_reduces_to_the_schrodinger_bridge_matcher():
    fm = _matcher(cfm_amd.ConstantNoiseScheduler(1.0))
    sb = cfm_amd.SchrodingerBridgeConditionalFlowMatcher(1.0)
    x0, x1, t, eps = _batch()
    xa, xb = fm.sample_xt(x0, x1, t, eps), sb.sample_xt(x0, x1, t, eps)
    ua, ub = fm.compute_conditional_flow(x0, x1, t, xa), sb.compute_conditional_flow(x0, x1, t, xa)
    assert float((xa - xb).abs().max()) <= 1e-12 * float(xb.abs().max())
    assert float((ua - ub).abs().max()) <= 1e-12 * float(ub.abs().max())
    assert fm.ot_sampler.reg == sb.ot_sampler.reg
    for s in (0.5, 0.7):
        assert _matcher(cfm_amd.ConstantNoiseScheduler(s)).ot_sampler.reg == \
            cfm_amd.SchrodingerBridgeConditionalFlowMatcher(s).ot_sampler.reg


def test_ot_regularisation_is_twice_F_of_one(schedule):
    assert _matcher(schedule).ot_sampler.reg == 2 * schedule.F(1.0)
    assert _matcher(schedule).ot_method == "exact"
    assert cfm_amd.ScheduledBridgeConditionalFlowMatcher(schedule, ot_method="sinkhorn").ot_sampler.method == "sinkhorn"


def test_lambda_is_the_runner_score_weight(schedule):
    fm = _matcher(schedule)
    _, _, t, _ = _batch()
    lam = fm.compute_lambda(t)
    assert torch.equal(lam, 2 * schedule.sigma_t(t) / schedule(t) ** 2)
    assert torch.equal(fm.compute_sigma_t(t), schedule.sigma_t(t))
    for s in (0.5, 1.0):
        a = _matcher(cfm_amd.ConstantNoiseScheduler(s)).compute_lambda(t)
        b = cfm_amd.SchrodingerBridgeConditionalFlowMatcher(s).compute_lambda(t)
        # SB divides by sigma^2 + 1e-8 (the reference's guard): a relative 1e-8 / sigma^2, plus rounding
        assert float(((a - b) / b).abs().max()) <= 1e-8 / s ** 2 + 1e-14


def test_eager_composition_on_host_tensors_with_index_pairs(schedule):
    """fp32 host tensors take the eager composition (there is no kernel for them); the OT pairing is a plain gather"""
    fm = _matcher(schedule)
    x0, x1, t, eps = (z.float() for z in _batch(B=17, d=3))
    i, j = torch.randperm(17, generator=torch.Generator().manual_seed(2)), torch.arange(17).flip(0)
    torch.manual_seed(3)
    tt, xt, ut, e = fm._sample(x0, x1, t, True, idx=(i, j))
    torch.manual_seed(3)
    assert torch.equal(e, torch.randn_like(x0)) and tt is t
    r, sig, a, c = (z[:, None] for z in fm._coefs(t))
    mu = x0[i] + (x1[j] - x0[i]) * r
    assert torch.equal(xt, mu + sig * e)
    assert torch.equal(ut, a * (xt - mu) + (x1[j] - x0[i]) * c)
    assert torch.equal(fm.compute_mu_t(x0[i], x1[j], t), mu)
    # a number for t
    assert torch.equal(fm.compute_mu_t(x0, x1, 0.5), x0 + (x1 - x0) * (schedule.F(0.5) / schedule.F(1.0)))
    # differentiable in the inputs
    xg = x0.clone().requires_grad_(True)
    fm.compute_conditional_flow(xg, x1, t, fm.sample_xt(xg, x1, t, eps)).sum().backward()
    assert torch.isfinite(xg.grad).all()


def test_end_points_are_finite(schedule):
    fm = _matcher(schedule)
    x0, x1, _, eps = (z.float() for z in _batch(B=4, d=3))
    t = torch.tensor([0.0, 1.0, 0.0, 1.0])
    xt = fm.sample_xt(x0, x1, t, eps)
    ut = fm.compute_conditional_flow(x0, x1, t, xt)
    assert torch.isfinite(xt).all() and torch.isfinite(ut).all()
    assert torch.equal(xt[0], x0[0])


def test_constructor_checks():
    with pytest.raises(TypeError, match="NoiseScheduler"):
        cfm_amd.ScheduledBridgeConditionalFlowMatcher(0.5)
    with pytest.raises(ValueError, match="strictly positive"):
        cfm_amd.ScheduledBridgeConditionalFlowMatcher(cfm_amd.ConstantNoiseScheduler(0.0))


# ------------------------------------------------------------------------------------------------ trajectory matcher
def test_trajectory_matcher_eager_path_and_spline_refusal(schedule):
    fm = _matcher(schedule)
    with pytest.raises(ValueError, match="spline"):
        cfm_amd.TrajectoryFlowMatcher(fm, "spline")
    fm.ot_sampler = None                                    # no coupling: nothing needs the GPU
    B, T, d, L = 12, 4, 3, 1
    X = torch.randn(B, T, d, generator=torch.Generator().manual_seed(5))
    tfm = cfm_amd.TrajectoryFlowMatcher(fm, "linear", leaveout_timepoint=L)
    ts = torch.tensor([0, 2] * (B // 2))
    t = torch.rand(B, generator=torch.Generator().manual_seed(6))
    eps = torch.randn(B, d, generator=torch.Generator().manual_seed(7))
    t_net, xt, ut, e, (t_loc, sel) = tfm.sample_location_and_conditional_flow(X, t_select=ts, t=t, eps=eps, return_noise=True,
                                                                              return_interval=True)
    assert tfm.last_path == "eager" and torch.equal(t_loc, t) and torch.equal(sel, ts)
    rb = torch.arange(B)
    x0, x1 = X[rb, ts], X[rb, torch.where(ts == 0, ts + 2, ts + 1)]
    wx = fm.sample_xt(x0, x1, t, eps)
    wu = fm.compute_conditional_flow(x0, x1, t, wx)
    half = ts + 1 == L
    assert torch.equal(xt, wx) and torch.equal(ut, torch.where(half[:, None], wu / 2, wu))
    assert torch.equal(t_net, torch.where(half, t * 2, t) + ts)
    assert fm.compute_lambda(t_loc).shape == (B,)


# --------------------------------------------------------------------------------------------------- sampler records
def _refined(ts, dt):
    """the refined grid, restated: every interval of ts in n equal steps, n the smallest with step <= dt"""
    out = []
    for a, b in zip(ts[:-1], ts[1:]):
        n = max(1, int(math.ceil(abs(b - a) / dt * (1.0 - 1e-6))))
        out += [(a + (b - a) * k / n, (b - a) / n, k == n - 1) for k in range(n)]
    return out


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", ["linear", "cosine"])
def test_step_records_carry_g_at_the_solver_time(name, reverse):
    schedule = SCHEDULES[name]()
    ts, dt = [0.0, 0.13, 0.5, 1.0], 0.1
    steps = sde_mod._grid(torch.tensor(ts, dtype=torch.float64), dt)
    want = _refined(ts, dt)
    assert len(steps) == len(want) == 11 and len({round(h, 9) for _, h, _ in steps}) == 3
    g = sde_mod._schedule_values(schedule, steps)
    blob = sde_mod._em_records(steps, g, reverse)
    assert len(blob) == 16 * len(steps)
    for k, (tk, hk, out) in enumerate(want):
        te, h, gs, is_out = struct.unpack_from("<fffi", blob, 16 * k)
        gk = float(schedule(torch.as_tensor(tk, dtype=torch.float32)))          # the SOLVER's time, also in reverse
        assert g[k] == gk
        assert gs == np.float32(gk * math.sqrt(abs(hk)))
        assert te == np.float32(1.0 - tk if reverse else tk) and h == np.float32(hk) and is_out == int(out)
    if reverse and name == "linear":  # g(1 - t_k) would be another number (the cosine schedule is symmetric in t)
        assert g[0] != float(schedule(torch.as_tensor(1.0 - want[0][0], dtype=torch.float32)))
    # a state-dependent "schedule" has no scalar per step
    assert sde_mod._schedule_values(lambda t: torch.ones(5, 2), steps) is None
    assert sde_mod._schedule_values(lambda t: "x", steps) is None
    assert sde_mod._schedule_values(lambda t: 0.5, steps) == [0.5] * 11


def test_values_of_a_built_in_schedule_are_kept_per_grid_and_parameters():
    schedule = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    steps = sde_mod._grid([0.0, 0.3, 1.0], 0.1)
    direct = [float(schedule(torch.as_tensor(t, dtype=torch.float32))) for t, _, _ in steps]
    a = sde_mod._schedule_values(schedule, steps)
    b = sde_mod._schedule_values(schedule, steps)
    assert a == b == direct and a is not b
    b[0] = -1.0                                              # the caller's list is its own
    assert sde_mod._schedule_values(schedule, steps) == direct
    schedule.sigma_max = 2.0                                 # other parameters, other values
    assert sde_mod._schedule_values(schedule, steps)[0] == float(schedule(torch.as_tensor(0.0, dtype=torch.float32))) != direct[0]
    assert sde_mod._schedule_values(schedule, steps[:3]) == [float(schedule(torch.as_tensor(t, dtype=torch.float32)))
                                                             for t, _, _ in steps[:3]]
    # any other callable is evaluated in every call
    calls = []
    probe = lambda t: calls.append(1) or 0.5
    sde_mod._schedule_values(probe, steps); sde_mod._schedule_values(probe, steps)
    assert len(calls) == 2 * len(steps)

    class Mine(cfm_amd.LinearDecreasingNoiseScheduler):
        def __call__(self, t):
            calls.append(1)
            return super().__call__(t)
    mine = Mine(0.1, 1.0)
    n0 = len(calls)
    sde_mod._schedule_values(mine, steps); sde_mod._schedule_values(mine, steps)
    assert len(calls) == n0 + 2 * len(steps)


def _drift(x):
    return -0.5 * x[:, :-1] * (1.0 + x[:, -1:])


def _score(x):
    return 0.25 * torch.sin(x[:, :-1]) - 0.1 * x[:, -1:]


@pytest.mark.parametrize("reverse", [False, True])
def test_eager_scheme_reads_the_schedule_at_the_solver_time(reverse):
    schedule = SCHEDULES["linear"]()
    y0 = torch.linspace(-1.0, 1.0, 8, dtype=torch.float64).reshape(4, 2)
    ts = torch.tensor([0.0, 0.13, 0.5, 1.0], dtype=torch.float64)
    xi = torch.randn(11, 4, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    sde = FlowScoreSDE(_drift, _score, sigma=schedule, reverse=reverse)
    got = sdeint(sde, y0, ts, dt=0.1, noise=xi)
    assert sde.last_path == "eager"
    y, outs = y0, [y0]
    for k, (tk, hk, out) in enumerate(_refined([float(v) for v in ts], 0.1)):
        tt = torch.as_tensor(tk, dtype=torch.float64)
        y = y + hk * sde.f(tt, y) + schedule(tt) * math.sqrt(abs(hk)) * xi[k]
        if out:
            outs.append(y)
    assert torch.equal(got, torch.stack(outs))
    # lambda t: schedule(1 - t) is the documented way to read it backwards
    back = sdeint(FlowScoreSDE(_drift, _score, sigma=lambda t: schedule(1 - t), reverse=reverse), y0, ts, dt=0.1, noise=xi)
    assert not torch.equal(back, got)


def test_flow_solver_reports_its_path_and_counts_steps():
    schedule = SCHEDULES["cosine"]()
    from cfm_amd.utils import torch_wrapper
    torch.manual_seed(0)
    v, s = cfm_amd.MLP(dim=2, time_varying=True, w=16), cfm_amd.MLP(dim=2, time_varying=True, w=16)
    y0 = torch.randn(6, 2)
    ts = torch.tensor([0.0, 0.5, 1.0])
    fs = FlowSolver(torch_wrapper(v), 2, score_field=torch_wrapper(s), sigma=schedule, dt=0.1)
    assert fs._hip_fields() == (v, s) and fs.last_path is None
    # what does not unwrap to two MLPs keeps the generic scheme
    for other in (FlowSolver(lambda t, x: -x, 2, score_field=torch_wrapper(s), sigma=schedule),
                  FlowSolver(torch_wrapper(v), 2, sigma=schedule),
                  FlowSolver(torch_wrapper(v), 2, score_field=torch_wrapper(s), sigma=schedule, sde_solver="srk"),
                  FlowSolver(torch_wrapper(cfm_amd.MLP(dim=2, w=16)), 2, score_field=torch_wrapper(s), sigma=schedule)):
        assert other._hip_fields() is None
    gen = FlowSolver(lambda t, x: -x, 2, score_field=lambda t, x: -0.1 * x, sigma=schedule, dt=0.1)
    out = gen.sdeint(y0, ts, generator=torch.Generator().manual_seed(4))
    assert gen.last_path == "eager" and gen.nfe == 10 and out.shape == (3, 6, 2)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    schedule = SCHEDULES["linear"]()
    y0 = torch.zeros((5, 2), dtype=torch.float64)
    ts = torch.tensor([0.0, 1.0])
    with pytest.raises(NotImplementedError, match="constant"):
        sdeint(FlowScoreSDE(_drift, _score, sigma=schedule), y0, ts, method="srk", dt=0.1)
    with pytest.raises(NotImplementedError, match="constant"):
        FlowSolver(lambda t, x: -x, 2, score_field=lambda t, x: -x, sigma=schedule, sde_solver="srk", dt=0.1).sdeint(y0, ts)
    with pytest.raises(ValueError, match="spline"):
        cfm_amd.TrajectoryFlowMatcher(_matcher(schedule), interpolant="spline")
    v, s = cfm_amd.MLP(dim=2, time_varying=True, w=16), cfm_amd.MLP(dim=2, time_varying=True, w=16)
    state_dependent = FlowScoreSDE(v, s, sigma=lambda t: torch.ones(5, 2))
    with pytest.raises(ValueError, match=r"fused=True.*scalar"):
        sdeint(state_dependent, y0.float(), ts, dt=0.1, fused=True)
    # without fused=True the same object is stepped in eager torch
    state_dependent = FlowScoreSDE(_drift, _score, sigma=lambda t: torch.ones(5, 2))
    out = sdeint(state_dependent, y0.float(), ts, dt=0.5)
    assert out.shape == (2, 5, 2) and state_dependent.last_path == "eager"
