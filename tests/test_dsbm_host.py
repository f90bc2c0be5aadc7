"""CPU: DSBM (diffusion Schrodinger bridge matching) — the matcher's eager composition against the float64 fixture and a
line-by-line restatement, the step's constructor refusals, the single-drift SDE's step records, and DSBMFlowSolver's eager
schemes against hand-written loops (no GPU needed)."""
import math
import os
import struct

import numpy as np
import pytest
import torch

NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "net.6.weight", "net.6.bias")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _schedule(case):
    import cfm_amd
    return cfm_amd.ConstantNoiseScheduler(1.0) if case == "const1" else cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)


def _matcher_with_noise(schedule, eps, **kw):
    """a matcher whose noise draw is `eps` (sample_noise_like is not one of the closed forms: the path does not change)"""
    import cfm_amd
    FM = cfm_amd.DSBMConditionalFlowMatcher(schedule, **kw)
    FM.sample_noise_like = lambda x: eps
    return FM


def _restated(schedule, x0, x1, t, eps):
    """runner/src/models/cfm_module.py:834-841, :856, :1192-1199, :1215-1216, line by line in the inputs' dtype"""
    tx = t.reshape(-1, *([1] * (x0.dim() - 1)))
    r = schedule.F(tx) / float(schedule.F(1.0))
    mu_t = x0 + (x1 - x0) * r
    xt = mu_t + schedule.sigma_t(tx) * eps
    g = schedule(tx)
    ft = (x1 - x0) - (g * torch.sqrt(tx / (1 - tx + 1e-6))) * eps
    bt = (x0 - x1) - (g * torch.sqrt((1 - tx) / (tx + 1e-6))) * eps
    g1 = schedule(t)
    fs = (1 + g1 ** 2 * t / (1 - t + 1e-6)) ** -1
    bs = (1 + g1 ** 2 * (1 - t) / (t + 1e-6)) ** -1
    return xt, ft, bt, fs, bs


@pytest.mark.parametrize("case", ["const1", "lin"])
def test_eager_matcher_matches_the_float64_fixture(golden_dir, case):
    z = np.load(os.path.join(golden_dir, "dsbm_cases.npz"))
    x0, x1, t, eps = (torch.from_numpy(z[f"{case}_b0_{k}64"]) for k in ("x0", "x1", "t", "eps"))
    assert x0.dtype == torch.float64 and float(t.min()) >= 0.05 and float(t.max()) <= 0.95
    FM = _matcher_with_noise(_schedule(case), eps)
    out = FM.sample_location_and_targets(x0, x1, t=t, return_noise=True)
    assert len(out) == 7 and out[0] is t and out[6] is eps
    for got, k in zip(out[1:6], ("xt", "ft", "bt", "fs", "bs")):
        want = torch.from_numpy(z[f"{case}_b0_{k}64"])
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
    # the recorded fp32 batch is that float64 batch, rounded once
    for k in ("xt", "ft", "bt", "fs", "bs"):
        assert np.array_equal(z[f"{case}_b0_{k}"], z[f"{case}_b0_{k}64"].astype(np.float32)), k


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_eager_matcher_in_fp32_is_the_restated_lines_bit_for_bit(kind):
    import cfm_amd
    sched = {"constant": cfm_amd.ConstantNoiseScheduler(0.7), "linear": cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0),
             "cosine": cfm_amd.CosineNoiseScheduler(0.05, 0.4)}[kind]
    torch.manual_seed(3)
    x0, x1, eps = torch.randn(33, 3, 4), torch.randn(33, 3, 4), torch.randn(33, 3, 4)
    t = torch.rand(33); t[0], t[1] = 0.0, 1.0
    out = _matcher_with_noise(sched, eps).sample_location_and_targets(x0, x1, t=t)
    assert len(out) == 6
    for got, want in zip(out[1:], _restated(sched, x0, x1, t, eps)):
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert bool(torch.isfinite(got).all())                      # t = 0 and t = 1 included: the 1e-6 keeps them finite
    assert out[2].shape == x0.shape and out[4].shape == (33,)


def test_a_number_is_a_constant_schedule_and_no_ot_method_keeps_the_pairing():
    import cfm_amd
    torch.manual_seed(4)
    x0, x1, eps, t = torch.randn(16, 2), torch.randn(16, 2), torch.randn(16, 2), torch.rand(16)
    a = _matcher_with_noise(0.5, eps).sample_location_and_targets(x0, x1, t=t)
    b = _matcher_with_noise(cfm_amd.ConstantNoiseScheduler(0.5), eps).sample_location_and_targets(x0, x1, t=t)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    FM = cfm_amd.DSBMConditionalFlowMatcher(0.5)
    assert FM.ot_sampler is None and isinstance(FM.schedule, cfm_amd.ConstantNoiseScheduler)
    # rows stay paired as given: zero noise coefficient at t = 0 makes the forward target x1 - x0 row by row
    out = _matcher_with_noise(0.5, eps).sample_location_and_targets(x0, x1, t=torch.zeros(16))
    assert torch.equal(out[2], x1 - x0) and torch.equal(out[1], x0)
    assert cfm_amd.DSBMConditionalFlowMatcher(0.5, ot_method="exact").ot_sampler is not None
    with pytest.raises(TypeError, match="NoiseScheduler or a number"):
        cfm_amd.DSBMConditionalFlowMatcher("1.0")
    with pytest.raises(ValueError, match="strictly positive"):
        cfm_amd.DSBMConditionalFlowMatcher(0.0)
    # random t and noise when none are given: the shapes of the reference's batch
    t2, xt, ft, bt, fs, bs, e2 = cfm_amd.DSBMConditionalFlowMatcher(1.0).sample_location_and_targets(x0, x1, return_noise=True)
    assert t2.shape == (16,) and xt.shape == ft.shape == bt.shape == e2.shape == (16, 2) and fs.shape == bs.shape == (16,)


def test_an_overridden_closed_form_is_used():
    import cfm_amd

    class Mine(cfm_amd.DSBMConditionalFlowMatcher):
        def compute_sigma_t(self, t):
            return 0 * t

    torch.manual_seed(5)
    x0, x1, t = torch.randn(8, 2), torch.randn(8, 2), torch.rand(8)
    FM = Mine(1.0)
    assert FM._customised() and not cfm_amd.DSBMConditionalFlowMatcher(1.0)._customised()
    out = FM.sample_location_and_targets(x0, x1, t=t)
    assert torch.equal(out[1], x0 + (x1 - x0) * (t[:, None] / 1.0))


def test_dsbm_step_names_what_it_refuses():
    import cfm_amd
    assert cfm_amd.DSBMStep is cfm_amd.train.DSBMStep
    a, b = cfm_amd.MLP(dim=2, w=16, time_varying=True), cfm_amd.MLP(dim=2, w=16, time_varying=True)
    opt = torch.optim.Adam(list(a.parameters()) + list(b.parameters()))
    with pytest.raises(TypeError, match="DSBMStep: the forward model is not on the GPU"):
        cfm_amd.DSBMStep(a, b, opt)
    with pytest.raises(TypeError, match=r"layer sizes differ \(forward .*, backward "):
        cfm_amd.DSBMStep(a, cfm_amd.MLP(dim=2, w=32, time_varying=True), opt)
    with pytest.raises(TypeError, match="the backward model is a Sequential, not a cfm_amd.MLP"):
        cfm_amd.DSBMStep(a, torch.nn.Sequential(torch.nn.Linear(3, 2)), opt)
    with pytest.raises(TypeError, match="not fp32"):
        cfm_amd.DSBMStep(a, cfm_amd.MLP(dim=2, w=16, time_varying=True).double(), opt)
    deep = cfm_amd.MLP(dim=2, w=16, time_varying=True)
    widths = [3] + [16] * 7 + [2]
    mods = []
    for k in range(8):
        mods += ([torch.nn.SELU()] if k else []) + [torch.nn.Linear(widths[k], widths[k + 1])]
    deep.net = torch.nn.Sequential(*mods)
    with pytest.raises(TypeError, match="8 Linear layers; the fused step takes at most 7"):
        cfm_amd.DSBMStep(deep, deep, opt)
    # the same module twice is refused before anything is allocated for it (checked where a device is not needed:
    # the device check comes first on a CPU net, so the order of the two is what this asserts)
    with pytest.raises(TypeError, match="not on the GPU|same module"):
        cfm_amd.DSBMStep(a, a, opt)
    assert "Loss Not Finite" in cfm_amd.DSBMStep.__doc__


def test_reverse_records_carry_one_minus_t_and_the_kernel_flag_stays_zero():
    from cfm_amd import sde
    steps = sde._grid([0.0, 0.5, 1.0], 0.25)
    assert len(steps) == 4
    g = [0.5, 0.6, 0.7, 0.8]
    fw, rv = sde._em_records(steps, g, False), sde._em_records(steps, g, True)
    for k, (t, h, is_out) in enumerate(steps):
        te_f, h_f, gs_f, out_f = struct.unpack_from("<fffi", fw, 16 * k)
        te_r, h_r, gs_r, out_r = struct.unpack_from("<fffi", rv, 16 * k)
        assert te_f == np.float32(t) and te_r == np.float32(1.0 - t)
        assert h_f == h_r == np.float32(h) and gs_f == gs_r == np.float32(g[k] * math.sqrt(abs(h)))     # g at the solver's time
        assert out_f == out_r == (1 if is_out else 0)
    f = lambda x: x[:, :-1]
    assert sde._kernel_reverse_flag(sde.DriftSDE(f, 1.0, reverse=True)) == 0
    assert sde._kernel_reverse_flag(sde.DriftSDE(f, 1.0, reverse=False)) == 0
    assert sde._kernel_reverse_flag(sde.FlowScoreSDE(f, f, 1.0, reverse=True)) == 1
    # the class itself: +drift at 1 - t on the way back
    d = lambda x: x[:, :-1] * 0 + x[:, -1:]
    y = torch.zeros(3, 2, dtype=torch.float64)
    assert torch.equal(sde.DriftSDE(d, 1.0, reverse=True).f(0.25, y), torch.full_like(y, 0.75))
    assert torch.equal(sde.DriftSDE(d, 1.0).f(0.25, y), torch.full_like(y, 0.25))


def _solver(fwd, bwd, sigma, **kw):
    import cfm_amd
    return cfm_amd.DSBMFlowSolver(fwd, 2, score_field=bwd, sigma=sigma, **kw)


@pytest.mark.parametrize("reverse", [False, True])
def test_eager_sdeint_is_the_hand_written_euler_maruyama_loop(reverse):
    import cfm_amd
    sched = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    fwd = lambda t, x: torch.sin(x) * t + 0.3
    bwd = lambda t, x: -0.5 * x + torch.cos(3 * t)
    torch.manual_seed(6)
    y0 = torch.randn(7, 2, dtype=torch.float64)
    ts = torch.tensor([0.0, 0.5, 1.0])
    n_sub, h = 10, 0.05
    xi = torch.randn(2 * n_sub, 7, 2, dtype=torch.float64)
    s = _solver(fwd, bwd, sched, dt=0.05)
    got = s.sdeint(y0, ts, reverse=reverse, noise=xi)
    assert s.last_path == "eager" and got.shape == (3, 7, 2) and s.nfe == 2 * n_sub
    y, want, k = y0, [y0], 0
    for a, b in ((0.0, 0.5), (0.5, 1.0)):
        for j in range(n_sub):
            tt = torch.as_tensor(a + (b - a) * j / n_sub, dtype=torch.float64)
            hh = (b - a) / n_sub
            drift = bwd(1 - tt, y) if reverse else fwd(tt, y)          # the backward net at 1 - t, with a PLUS sign
            y = y + hh * drift + sched(tt) * torch.ones_like(y) * math.sqrt(abs(hh)) * xi[k]      # g at the solver's time
            k += 1
        want.append(y)
    assert hh == h and torch.equal(got, torch.stack(want))
    with pytest.raises(NotImplementedError, match="srk"):
        _solver(fwd, bwd, sched, sde_solver="srk").sdeint(y0, ts)
    with pytest.raises(TypeError, match="backward drift net"):
        cfm_amd.DSBMFlowSolver(fwd, 2, sigma=sched)


@pytest.mark.parametrize("ts", [[0.0, 0.25, 0.5, 1.0], [1.0, 0.5, 0.0]])
def test_eager_odeint_steps_the_halved_difference(ts):
    fwd = lambda t, x: torch.sin(x) * t + 0.3
    bwd = lambda t, x: -0.5 * x + torch.cos(3 * t)
    torch.manual_seed(7)
    x0 = torch.randn(5, 2, dtype=torch.float64)
    s = _solver(fwd, bwd, 1.0, ode_solver="euler")
    got = s.odeint(x0, torch.tensor(ts))
    tsf = torch.tensor(ts, dtype=torch.float32)
    x, want = x0, [x0]
    for k in range(len(ts) - 1):
        tt = torch.as_tensor(float(tsf[k]), dtype=torch.float32)
        x = x + float(tsf[k + 1] - tsf[k]) * ((fwd(tt, x) - bwd(tt, x)) / 2)
        want.append(x)
    assert s.last_path == "eager" and s.nfe == len(ts) - 1 and torch.equal(got, torch.stack(want))
    s4 = _solver(fwd, bwd, 1.0, ode_solver="rk4")
    s4.odeint(x0, torch.tensor(ts))
    assert s4.nfe == 4 * (len(ts) - 1)                                 # one evaluation of the PAIR per stage


def test_resample_pairs_puts_the_time_zero_end_in_column_zero():
    """stub drifts with known trajectories (no noise, steps of 1/4: exact): forward y1 = y0 + 1 from x0's first half,
    backward y0 = y1 - 2 from x1's second half"""
    fwd = lambda t, x: torch.ones_like(x)
    bwd = lambda t, x: torch.full_like(x, -2.0)
    torch.manual_seed(8)
    x0, x1 = torch.randn(6, 2, dtype=torch.float64).round(decimals=2), torch.randn(6, 2, dtype=torch.float64).round(decimals=2)
    s = _solver(fwd, bwd, lambda t: 0.0 * t, dt=0.25)
    pairs = s.resample_pairs(x0, x1)
    assert pairs.shape == (6, 2, 2)
    assert torch.equal(pairs[:3, 0], x0[:3]) and torch.allclose(pairs[:3, 1], x0[:3] + 1, rtol=0, atol=1e-15)
    assert torch.equal(pairs[3:, 1], x1[3:]) and torch.allclose(pairs[3:, 0], x1[3:] - 2, rtol=0, atol=1e-15)
    # with noise: the given tensor is split by rows between the two solves
    xi = torch.randn(4, 6, 2, dtype=torch.float64)
    s1 = _solver(fwd, bwd, 1.0, dt=0.25)
    got = s1.resample_pairs(x0, x1, noise=xi)
    f = s1.sdeint(x0[:3], torch.linspace(0, 1, 2), noise=xi[:, :3])
    b = torch.flip(s1.sdeint(x1[3:], torch.linspace(0, 1, 2), reverse=True, noise=xi[:, 3:]), (0,))
    assert torch.equal(got, torch.cat([f, b], dim=1).transpose(0, 1))


def test_header_cites_the_reference_lines():
    src = open(os.path.join(ROOT, "include", "cfm_gfx950.h")).read()
    for name, cite in (("cfm_sample_dsbm_f32", "cfm_module.py:834-841"), ("cfm_mlp_dsbm_step_f32", "cfm_module.py:1203-1227"),
                       ("cfm_ode_fixed_pair_mlp_f32", "solver.py:259-263")):
        doc = src[:src.index(f"int {name}")]
        assert cite in doc[doc.rindex("/*"):], name


@pytest.mark.parametrize("case", ["const1", "lin"])
def test_fixture_is_self_consistent(golden_dir, case):
    """step 0 of the recorded float64 run, recomputed with torch autograd from the stored arrays alone"""
    import cfm_amd
    z = np.load(os.path.join(golden_dir, "dsbm_cases.npz"))
    B, d, w = (int(v) for v in z[f"{case}_meta"][:3])
    nets = {}
    for tag in ("fwd", "bwd"):
        nets[tag] = cfm_amd.MLP(dim=d, w=w, time_varying=True).double()
        nets[tag].load_state_dict({k: torch.from_numpy(z[f"{case}_{tag}_{k}"]).double() for k in NAMES})
    t, xt, ft, bt, fs, bs = (torch.from_numpy(z[f"{case}_b0_{k}"]).double() for k in ("t", "xt", "ft", "bt", "fs", "bs"))
    assert t.shape == (B,) and xt.shape == (B, d) and z[f"{case}_losses"].shape == (5, 2)
    x = torch.cat([xt, t[:, None]], dim=-1)
    fl = torch.mean(fs[:, None] * (nets["fwd"].net(x) - ft) ** 2)
    bl = torch.mean(bs[:, None] * (nets["bwd"].net(x) - bt) ** 2)
    (fl + bl).backward()
    fl, bl = fl.detach(), bl.detach()
    assert abs(float(fl) - z[f"{case}_losses"][0, 0]) <= 1e-12 * abs(float(fl))
    assert abs(float(bl) - z[f"{case}_losses"][0, 1]) <= 1e-12 * abs(float(bl))
    for tag in ("fwd", "bwd"):
        for k, p in nets[tag].named_parameters():
            g = torch.from_numpy(z[f"{case}_grad0_{tag}_{k}"])
            assert g.dtype == torch.float64 and (g - p.grad).abs().max() <= 1e-12 * g.abs().max(), (tag, k)
