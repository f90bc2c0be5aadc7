"""GPU: DSBM (diffusion Schrodinger bridge matching) — the bridge kernel (cfm_sample_dsbm_f32) bit for bit against the
matcher's eager composition; the two-net step (cfm_mlp_dsbm_step_f32 / cfm_amd.DSBMStep) against float64 autograd, the recorded
float64 loop (tests/golden/dsbm_cases.npz) and, with unit weights, bit for bit against the one-net step; the single-field
one-launch Euler-Maruyama sampler and the pair ODE kernel (cfm_ode_fixed_pair_mlp_f32) bit for bit against their
launch-per-step forms and against float64 restatements."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "net.6.weight", "net.6.bias")


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "dsbm_cases.npz"))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _params(*nets):
    return [p for n in nets for p in n.parameters()]


def _schedules():
    import cfm_amd
    return {"constant": cfm_amd.ConstantNoiseScheduler(0.7), "linear": cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0),
            "cosine": cfm_amd.CosineNoiseScheduler(0.05, 0.4)}


# ---------------------------------------------------------------------------------------------- the matcher kernel ----
def _eager(FM, x0, x1, t, eps):
    """the class's eager composition (its closed-form methods, which are plain torch ops), on the inputs' device"""
    from cfm_amd import pad_t_like_x
    xt = FM.compute_mu_t(x0, x1, t) + pad_t_like_x(FM.compute_sigma_t(t), x0) * eps
    ft, bt = FM.compute_targets(x0, x1, t, eps)
    return xt, ft, bt


# (256, 2): two-column rows, scalar path; (130, 7): rows off the 16-byte grid; (64, 100): the 16-byte path, more than one
# block; (33, 3, 4, 5): image-shaped samples, 60 columns on the 16-byte path; (1, 4): one row
@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
@pytest.mark.parametrize("shape", [(256, 2), (130, 7), (64, 100), (33, 3, 4, 5), (1, 4)])
def test_matcher_kernel_is_bit_equal_to_the_eager_composition(dev, kind, shape):
    import cfm_amd
    FM = cfm_amd.DSBMConditionalFlowMatcher(_schedules()[kind])
    torch.manual_seed(sum(shape))
    x0, x1 = torch.randn(shape, device=dev), torch.randn(shape, device=dev) * 0.5 + 2.0
    t = torch.rand(shape[0], device=dev)
    t[0] = 0.0
    if shape[0] > 1:
        t[1] = 1.0
    out = FM.sample_location_and_targets(x0, x1, t=t, return_noise=True)
    t2, xt, ft, bt, fs, bs, eps = out
    assert t2 is t and eps.shape == x0.shape and xt.is_cuda and xt.dtype == torch.float32
    for got, want, what in zip((xt, ft, bt), _eager(FM, x0, x1, t, eps), ("xt", "forward_target", "backward_target")):
        assert got.shape == x0.shape and torch.equal(got, want), what
        assert bool(torch.isfinite(got).all()), what
    wf, wb = FM.compute_scalings(t)
    assert torch.equal(fs, wf) and torch.equal(bs, wb) and fs.shape == (shape[0],)
    # an explicit coupling: the gather is fused; against gather-then-eager
    i, j = torch.randperm(shape[0], device=dev), torch.randperm(shape[0], device=dev)

    class _Pairs:
        def _sample_indices(self, a, b):
            return i, j
    FM.ot_sampler = _Pairs()
    _, xt, ft, bt, _, _, eps = FM.sample_location_and_targets(x0, x1, t=t, return_noise=True)
    for got, want in zip((xt, ft, bt), _eager(FM, x0[i], x1[j], t, eps)):
        assert torch.equal(got, want)


def test_matcher_escapes_and_coupled_form(dev):
    import cfm_amd
    FM = cfm_amd.DSBMConditionalFlowMatcher(1.0, ot_method="exact")
    torch.manual_seed(1)
    x0, x1 = torch.randn(64, 2, device=dev), torch.randn(64, 2, device=dev) + 3.0
    t, xt, ft, bt, fs, bs = FM.sample_location_and_targets(x0, x1)
    assert xt.shape == (64, 2) and bool(torch.isfinite(ft).all()) and bool(torch.isfinite(bt).all())
    # float64 and requires-grad inputs keep the eager composition (dtype and graph survive)
    out = cfm_amd.DSBMConditionalFlowMatcher(1.0).sample_location_and_targets(x0.double(), x1.double(), t=t.double())
    assert out[1].dtype == torch.float64
    x0g = x0.clone().requires_grad_(True)
    out = cfm_amd.DSBMConditionalFlowMatcher(1.0).sample_location_and_targets(x0g, x1, t=t)
    assert out[1].requires_grad


# -------------------------------------------------------------------------------------------------------- the step ----
def _f64(fwd, bwd, t, xt, ft, bt, fs, bs):
    """runner/src/models/cfm_module.py:1221-1227 in float64 on the host: (forward_loss, backward_loss, gradients forward first)"""
    f, b = copy.deepcopy(fwd).double().cpu(), copy.deepcopy(bwd).double().cpu()
    for p in _params(f, b):
        p.grad = None
    x = torch.cat([xt.double().cpu(), t.double().cpu()[:, None]], dim=-1)
    fl = torch.mean(fs.double().cpu()[:, None] * (f.net(x) - ft.double().cpu()) ** 2)
    bl = torch.mean(bs.double().cpu()[:, None] * (b.net(x) - bt.double().cpu()) ** 2)
    (fl + bl).backward()
    return float(fl.detach()), float(bl.detach()), [p.grad for p in _params(f, b)]


def _random_case(dev, B, d, w, seed, layers=None):
    """seeded nets and a batch shaped like the matcher's at g = 1: t in [0.05, 0.95], scalings from their formula"""
    import cfm_amd
    torch.manual_seed(seed)
    nets = []
    for _ in range(2):
        net = cfm_amd.MLP(dim=d, time_varying=True, w=w)
        if layers is not None:
            widths = [d + 1] + [w] * (layers - 1) + [d]
            mods = []
            for k in range(layers):
                mods += ([torch.nn.SELU()] if k else []) + [torch.nn.Linear(widths[k], widths[k + 1])]
            net.net = torch.nn.Sequential(*mods)
        nets.append(net.to(dev))
    t = 0.05 + 0.9 * torch.rand(B, device=dev)
    xt, ft, bt = (torch.randn(B, d, device=dev) for _ in range(3))
    fs = (1 + t / (1 - t + 1e-6)) ** -1
    bs = (1 + (1 - t) / (t + 1e-6)) ** -1
    return nets[0], nets[1], (t, xt, ft, bt, fs, bs)


def _golden_nets(dev, z, case):
    import cfm_amd
    B, d, w = (int(v) for v in z[f"{case}_meta"][:3])
    nets = []
    for tag in ("fwd", "bwd"):
        net = cfm_amd.MLP(dim=d, w=w, time_varying=True)
        net.load_state_dict({n: torch.from_numpy(z[f"{case}_{tag}_{n}"]) for n in NAMES})
        nets.append(net.to(dev))
    return nets


def _golden_batch(dev, z, case, k):
    return tuple(torch.from_numpy(z[f"{case}_b{k}_{n}"]).to(dev) for n in ("t", "xt", "ft", "bt", "fs", "bs"))


def _step(fwd, bwd, lr=1e-3):
    import cfm_amd
    return cfm_amd.DSBMStep(fwd, bwd, cfm_amd.FusedAdam(_params(fwd, bwd), lr=lr))


def _check_vs_f64(fwd, bwd, losses, want_fl, want_bl, want_grads, what):
    """tests/test_gpu_sf2m.py's convention: both losses and every gradient (largest-entry relative) within 1e-5"""
    fl, bl = (float(v) for v in losses.cpu())
    devs = [abs(fl - want_fl) / abs(want_fl), abs(bl - want_bl) / abs(want_bl)]
    devs += [_rel(p.grad.double().cpu(), g) for p, g in zip(_params(fwd, bwd), want_grads)]
    print(f"{what}: losses {devs[0]:.2e} {devs[1]:.2e}, gradients max {max(devs[2:]):.2e}")
    assert max(devs) <= 1e-5, devs


@pytest.mark.parametrize("case", ["const1", "lin"])
def test_step_matches_the_recorded_float64_step(dev, golden, case):
    fwd, bwd = _golden_nets(dev, golden, case)
    losses = _step(fwd, bwd).backward_only(*_golden_batch(dev, golden, case, 0))
    want = [torch.from_numpy(golden[f"{case}_grad0_{tag}_{n}"]) for tag in ("fwd", "bwd") for n in NAMES]
    _check_vs_f64(fwd, bwd, losses, golden[f"{case}_losses"][0, 0], golden[f"{case}_losses"][0, 1], want, case)


# shapes of tests/test_gpu_sf2m.py: (130, 7, 33) ragged tiles, odd widths, scalar loads, unpaired backward launches;
# (512, 20, 64) a direct-to-LDS hidden layer, a paired backward; (64, 3, 16) x 7 layers: the reduction table at its bound
@pytest.mark.parametrize("B,d,w,layers", [(130, 7, 33, None), (512, 20, 64, None), (64, 3, 16, 7)])
def test_step_matches_float64_autograd(dev, B, d, w, layers):
    fwd, bwd, batch = _random_case(dev, B, d, w, seed=B + d, layers=layers)
    losses = _step(fwd, bwd).backward_only(*batch)
    fl, bl, grads = _f64(fwd, bwd, *batch)
    _check_vs_f64(fwd, bwd, losses, fl, bl, grads, f"({B}, {d}, {w}, {layers})")


@pytest.mark.parametrize("B,d,w", [(256, 2, 64), (512, 20, 64)])
def test_unit_scalings_give_the_bits_of_the_one_net_step(dev, B, d, w):
    """w = 1: w * dlt = dlt and (dlt * scale) * 1 are exact, and every product's kernel is chosen per net as if it ran
    alone — each net's loss and gradients are RegressionStep's on its own target, bit for bit"""
    import cfm_amd
    fwd, bwd, (t, xt, ft, bt, fs, bs) = _random_case(dev, B, d, w, seed=41 + B)
    fc, bc = copy.deepcopy(fwd), copy.deepcopy(bwd)
    one = torch.ones_like(fs)
    losses = _step(fwd, bwd).backward_only(t, xt, ft, bt, one, one).clone()
    for net, ref, target, k in ((fwd, fc, ft, 0), (bwd, bc, bt, 1)):
        step1 = cfm_amd.RegressionStep(ref, cfm_amd.FusedAdam(ref.parameters()))
        l1 = step1.backward_only(t, xt, target)
        assert float(l1) == float(losses[k])
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(net.parameters(), ref.parameters()))


def test_halving_the_forward_weights_halves_the_forward_half_only(dev):
    fwd, bwd, (t, xt, ft, bt, fs, bs) = _random_case(dev, 512, 20, 64, seed=77)
    step = _step(fwd, bwd)
    l1 = step.backward_only(t, xt, ft, bt, fs, bs).clone()
    g1 = [p.grad.clone() for p in _params(fwd, bwd)]
    l2 = step.backward_only(t, xt, ft, bt, 0.5 * fs, bs).clone()
    nf = len(list(fwd.parameters()))
    assert float(l2[0]) == 0.5 * float(l1[0]) and float(l2[1]) == float(l1[1])
    for k, (a, p) in enumerate(zip(g1, _params(fwd, bwd))):
        assert torch.equal(p.grad, 0.5 * a if k < nf else a), k
    assert abs(float(step.loss()) - float(l2[0] + l2[1])) <= 1e-6 * float(step.loss())


def test_the_same_call_twice_gives_the_same_bits(dev):
    fwd, bwd, batch = _random_case(dev, 512, 20, 64, seed=5)
    step = _step(fwd, bwd)
    a = step.backward_only(*batch).clone(); ga = [p.grad.clone() for p in _params(fwd, bwd)]
    b = step.backward_only(*batch)
    assert torch.equal(a, b) and all(torch.equal(x, p.grad) for x, p in zip(ga, _params(fwd, bwd)))


@pytest.mark.parametrize("case", ["const1", "lin"])
def test_five_steps_track_the_recorded_float64_loop(dev, golden, case):
    """DSBMStep + one FusedAdam(lr=1e-3) over both nets on the recorded batches: both loss sequences within 1e-5 relative
    of the float64 loop (the float32 CPU loop of the fixture's script: <= 1.5e-7)"""
    fwd, bwd = _golden_nets(dev, golden, case)
    step = _step(fwd, bwd, lr=1e-3)
    got = np.asarray([step(*_golden_batch(dev, golden, case, k)).cpu().numpy().astype(np.float64) for k in range(5)])
    want = golden[f"{case}_losses"]
    rel = np.abs(got - want) / np.abs(want)
    print(f"{case}: five-step losses vs float64, max relative {rel.max():.2e}")
    assert rel.max() <= 1e-5, rel
    assert all(int(st["step"]) == 5 for st in step.opt.state.values()) and len(step.opt.state) == 16


def test_step_refusals_on_the_device(dev):
    import cfm_amd
    fwd, bwd, (t, xt, ft, bt, fs, bs) = _random_case(dev, 64, 3, 16, seed=1)
    with pytest.raises(TypeError, match="the forward and the backward model are the same module"):
        cfm_amd.DSBMStep(fwd, fwd, cfm_amd.FusedAdam(fwd.parameters()))
    step = _step(fwd, bwd)
    with pytest.raises(RuntimeError, match="scalings have 63 and 64 values for 64 rows"):
        step.backward_only(t, xt, ft, bt, fs[:63], bs)
    with pytest.raises(RuntimeError, match="the targets"):
        step.backward_only(t, xt, ft[:, :2], bt, fs, bs)


def test_matcher_step_and_optimizer_end_to_end(dev):
    """matcher -> DSBMStep -> one FusedAdam step at B = 256, d = 2 against float64 autograd of the restated lines and
    torch.optim.Adam in float64: losses, gradients and updated parameters within 1e-5"""
    import cfm_amd
    torch.manual_seed(9)
    fwd, bwd = (cfm_amd.MLP(dim=2, w=64, time_varying=True).to(dev) for _ in range(2))
    f64, b64 = copy.deepcopy(fwd).double().cpu(), copy.deepcopy(bwd).double().cpu()
    x0, x1 = torch.randn(256, 2, device=dev), torch.randn(256, 2, device=dev) * 0.5 + 2.0
    t = 0.05 + 0.9 * torch.rand(256, device=dev)
    sched = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    FM = cfm_amd.DSBMConditionalFlowMatcher(sched)
    t, xt, ft, bt, fs, bs, eps = FM.sample_location_and_targets(x0, x1, t=t, return_noise=True)
    step = _step(fwd, bwd, lr=1e-3)
    losses = step(t, xt, ft, bt, fs, bs).clone()
    # the restated lines in float64 from (x0, x1, t, eps)
    a0, a1, td, ed = x0.double().cpu(), x1.double().cpu(), t.double().cpu(), eps.double().cpu()
    tx = td[:, None]
    r = sched.F(tx) / sched.F(1.0)
    x = a0 + (a1 - a0) * r + torch.sqrt(sched.F(tx) - sched.F(tx) ** 2 / sched.F(1.0)) * ed
    g = sched(tx)
    tf = a1 - a0 - (g * torch.sqrt(tx / (1 - tx + 1e-6))) * ed
    tb = a0 - a1 - (g * torch.sqrt((1 - tx) / (tx + 1e-6))) * ed
    sf = (1 + sched(td) ** 2 * td / (1 - td + 1e-6)) ** -1
    sb = (1 + sched(td) ** 2 * (1 - td) / (td + 1e-6)) ** -1
    opt = torch.optim.Adam(_params(f64, b64), lr=1e-3)
    xin = torch.cat([x, td[:, None]], dim=-1)
    fl = torch.mean(sf[:, None] * (f64.net(xin) - tf) ** 2)
    bl = torch.mean(sb[:, None] * (b64.net(xin) - tb) ** 2)
    (fl + bl).backward()
    _check_vs_f64(fwd, bwd, losses, float(fl.detach()), float(bl.detach()), [p.grad for p in _params(f64, b64)], "end to end")
    opt.step()
    for p, q in zip(_params(fwd, bwd), _params(f64, b64)):
        assert _rel(p.detach().double().cpu(), q.detach()) <= 1e-5


# ----------------------------------------------------------------------------------------------------- the samplers ----
@contextlib.contextmanager
def _register_staged_layers():
    """The one-launch kernels sum k in the plain ascending order of the register-staged layer core; the layers' default
    engine (direct-to-LDS, gemm_glds64.h) has another fixed order.  As tests/test_gpu_round2.py and test_gpu_schedule.py do,
    the launch-per-step side of a BIT comparison runs on the register-staged core; on the default engine the same
    trajectory is held to 1e-5."""
    from cfm_amd import _lib
    lib = _lib.load()
    glds0 = lib.cfm_mlp_get_glds()
    try:
        lib.cfm_mlp_set_glds(0)
        yield
    finally:
        lib.cfm_mlp_set_glds(glds0)


def _nets(dev, d, w, seed, zero=False):
    import cfm_amd
    torch.manual_seed(seed)
    nets = [cfm_amd.MLP(dim=d, w=w, time_varying=True).to(dev) for _ in range(2)]
    if zero:
        for p in _params(*nets):
            p.data.zero_()
    return nets


def _solver(fwd, bwd, sigma, **kw):
    import cfm_amd
    from cfm_amd.utils import torch_wrapper
    return cfm_amd.DSBMFlowSolver(torch_wrapper(fwd), fwd.net[-1].out_features, score_field=torch_wrapper(bwd), sigma=sigma, **kw)


def _sde_schedules():
    import cfm_amd
    return {"constant": cfm_amd.ConstantNoiseScheduler(0.5), "linear": cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)}


# (100, 2, 64): seven 16-row tiles, the last one ragged; (17, 5, 33): two tiles, one row in the second, odd widths
@pytest.mark.parametrize("B,d,w", [(100, 2, 64), (17, 5, 33)])
@pytest.mark.parametrize("kind", ["constant", "linear"])
@pytest.mark.parametrize("reverse", [False, True])
def test_single_field_one_launch_em_is_bit_equal_to_the_launch_per_step_scheme(dev, B, d, w, kind, reverse):
    fwd, bwd = _nets(dev, d, w, seed=B + d)
    s = _solver(fwd, bwd, _sde_schedules()[kind], dt=0.05)
    torch.manual_seed(3)
    y0 = torch.randn(B, d, device=dev)
    ts = torch.linspace(0, 1, 5)
    xi = torch.randn(20, B, d, device=dev)
    one = s.sdeint(y0, ts, reverse=reverse, noise=xi)
    assert s.last_path == "hip" and one.shape == (5, B, d) and s.nfe == 20
    with _register_staged_layers():
        per_step = s.sdeint(y0, ts, reverse=reverse, noise=xi, fused=False)
    assert s.last_path == "hip" and torch.equal(one, per_step)
    assert _rel(s.sdeint(y0, ts, reverse=reverse, noise=xi, fused=False), one) <= 1e-5      # the layers' default engine
    assert torch.equal(one[0], y0) and bool(torch.isfinite(one).all()) and not torch.equal(one[-1], y0)
    # noise="torch": the increments are drawn step by step as the launch-per-step scheme draws them
    g1, g2 = torch.Generator(device=dev).manual_seed(11), torch.Generator(device=dev).manual_seed(11)
    a = s.sdeint(y0, ts, reverse=reverse, noise="torch", generator=g1)
    with _register_staged_layers():
        b = s.sdeint(y0, ts, reverse=reverse, noise="torch", generator=g2, fused=False)
    assert torch.equal(a, b) and not torch.equal(a, one)


@pytest.mark.parametrize("reverse", [False, True])
def test_sdeint_reads_the_right_net_at_the_right_time_with_the_right_sign(dev, reverse):
    """against the eager scheme in float64 on float64 copies of the nets, same noise: forward f(t, y); reverse +b(1 - t, y),
    g at the solver's time in both"""
    import cfm_amd
    fwd, bwd = _nets(dev, 2, 64, seed=21)
    sched = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    torch.manual_seed(4)
    y0 = torch.randn(100, 2, device=dev)
    ts = torch.linspace(0, 1, 5)
    xi = torch.randn(20, 100, 2, device=dev)
    got = _solver(fwd, bwd, sched, dt=0.05).sdeint(y0, ts, reverse=reverse, noise=xi)
    f64, b64 = copy.deepcopy(fwd).double().cpu(), copy.deepcopy(bwd).double().cpu()
    call = lambda net: (lambda t, x: net.net(torch.cat([x, t.reshape(1, 1).expand(x.shape[0], 1)], 1)))
    eager = cfm_amd.DSBMFlowSolver(call(f64), 2, score_field=call(b64), sigma=sched, dt=0.05)
    want = eager.sdeint(y0.double().cpu(), ts, reverse=reverse, noise=xi.double().cpu())
    assert eager.last_path == "eager"
    assert _rel(got.double().cpu(), want) <= 1e-5
    # and the other net, or the other time, is far away
    wrong = eager.sdeint(y0.double().cpu(), ts, reverse=not reverse, noise=xi.double().cpu())
    assert _rel(got.double().cpu(), wrong) > 1e-2


def test_philox_noise_is_seeded_and_has_the_schedule_variance(dev):
    import cfm_amd
    fwd, bwd = _nets(dev, 5, 64, seed=2, zero=True)
    sched = cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0)
    s = _solver(fwd, bwd, sched, dt=0.05)
    y0 = torch.zeros(4096, 5, device=dev)
    ts = torch.linspace(0, 1, 2)
    run = lambda seed, **kw: s.sdeint(y0, ts, generator=torch.Generator(device=dev).manual_seed(seed), **kw)
    a, b, c = run(5), run(5), run(6)
    assert s.last_path == "hip" and torch.equal(a, b) and not torch.equal(a, c)
    want = sum(float(sched(torch.tensor(k * 0.05))) ** 2 * 0.05 for k in range(20))      # sum_k g(t_k)^2 h, zero drift
    for traj in (a, run(5, reverse=True)):
        var = float((traj[-1] - traj[0]).double().pow(2).mean())
        print(f"variance of y1 - y0 over 4096 x 5: {var:.4f}, sum g^2 h = {want:.4f}")
        assert abs(var - want) <= 0.05 * want


def _pair_f64(fwd, bwd, x0, ts, solver):
    """the fixed-step recurrence of cfm_amd.ode.FIXED_TABLEAUS on k = (f - b) / 2, float64 on the host (times: the
    float32 grid's values)"""
    from cfm_amd.ode import FIXED_TABLEAUS
    f64, b64 = copy.deepcopy(fwd).double().cpu(), copy.deepcopy(bwd).double().cpu()
    tab = FIXED_TABLEAUS[solver]

    def ev(t, y):
        xin = torch.cat([y, torch.full((y.shape[0], 1), float(t), dtype=torch.float64)], 1)
        return (f64.net(xin) - b64.net(xin)) / 2
    x, sol = x0.double().cpu(), [x0.double().cpu()]
    tg = [float(v) for v in ts.to(torch.float32)]
    with torch.no_grad():
        for k in range(len(tg) - 1):
            t, dt = tg[k], tg[k + 1] - tg[k]
            ks = [ev(t, x)]
            for c, row in zip(tab["c"], tab["a"]):
                ks.append(ev(t + c * dt, x + dt * sum(a * kq for a, kq in zip(row, ks))))
            x = x + dt * sum(bq * kq for bq, kq in zip(tab["b"], ks))
            sol.append(x)
    return torch.stack(sol)


@pytest.mark.parametrize("B,d,w", [(100, 2, 64), (17, 5, 33)])
@pytest.mark.parametrize("solver", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("backward", [False, True])
def test_pair_ode_kernel_is_bit_equal_to_the_launch_per_stage_form(dev, B, d, w, solver, backward):
    fwd, bwd = _nets(dev, d, w, seed=B + 3 * d)
    s = _solver(fwd, bwd, 1.0, ode_solver=solver)
    torch.manual_seed(5)
    x0 = torch.randn(B, d, device=dev)
    ts = torch.linspace(1, 0, 21) if backward else torch.linspace(0, 1, 21)
    one = s.odeint(x0, ts)
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[solver]
    assert s.last_path == "hip" and one.shape == (21, B, d) and s.nfe == 20 * stages
    with _register_staged_layers():
        per_stage = s.odeint(x0, ts, fused=False)
    assert s.last_path == "hip" and s.nfe == 20 * stages
    assert _rel(s.odeint(x0, ts, fused=False), one) <= 1e-5                                   # the layers' default engine
    assert torch.equal(one, per_stage) and torch.equal(one[0], x0) and bool(torch.isfinite(one).all())
    want = _pair_f64(fwd, bwd, x0, ts, solver)
    dev_ = _rel(one.double().cpu(), want)
    print(f"pair ode {solver} ({B}, {d}, {w}) backward={backward}: vs float64 {dev_:.2e}")
    assert dev_ <= 1e-5


def test_pair_ode_of_a_negated_copy_is_the_one_field_solve(dev):
    """b = -f (the last layer negated): (f - b) / 2 = (f + f) / 2 = f with no rounding beyond the negation's, so the
    pair trajectory is NeuralODE's on the forward net alone (<= 1e-6 relative)"""
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    fwd, _ = _nets(dev, 2, 64, seed=13)
    bwd = copy.deepcopy(fwd)
    with torch.no_grad():
        bwd.net[-1].weight.neg_(); bwd.net[-1].bias.neg_()
    torch.manual_seed(6)
    x0 = torch.randn(100, 2, device=dev)
    ts = torch.linspace(0, 1, 21)
    for solver in ("euler", "rk4"):
        got = _solver(fwd, bwd, 1.0, ode_solver=solver).odeint(x0, ts)
        want = NeuralODE(torch_wrapper(fwd), solver=solver).trajectory(x0, ts)
        assert _rel(got, want) <= 1e-6


def test_pair_ode_outside_the_small_envelope_and_adaptive(dev):
    """w = 128: the layer driver of the same entry (still HIP) against the float64 restatement; dopri5: NeuralODE's generic
    path on the combined callable"""
    fwd, bwd = _nets(dev, 3, 128, seed=17)
    torch.manual_seed(7)
    x0 = torch.randn(50, 3, device=dev)
    ts = torch.linspace(0, 1, 6)
    s = _solver(fwd, bwd, 1.0, ode_solver="midpoint")
    got = s.odeint(x0, ts)
    assert s.last_path == "hip" and s.nfe == 10
    assert _rel(got.double().cpu(), _pair_f64(fwd, bwd, x0, ts, "midpoint")) <= 1e-5
    s5 = _solver(fwd, bwd, 1.0, ode_solver="dopri5")
    out = s5.odeint(x0, ts)
    assert s5.last_path == "eager" and out.shape == (6, 50, 3) and s5.nfe > 0


def test_all_three_routes_run_on_hip_and_resample_pairs_is_their_composition(dev):
    import cfm_amd
    fwd, bwd = _nets(dev, 2, 64, seed=19)
    s = _solver(fwd, bwd, cfm_amd.ConstantNoiseScheduler(1.0), dt=0.01)
    torch.manual_seed(8)
    x0, x1 = torch.randn(64, 2, device=dev), torch.randn(64, 2, device=dev) + 2.0
    ts = torch.linspace(0, 1, 2)
    paths = []
    s.sdeint(x0, ts); paths.append(s.last_path)
    s.sdeint(x1, ts, reverse=True); paths.append(s.last_path)
    s.odeint(x0, torch.linspace(0, 1, 11)); paths.append(s.last_path)
    assert paths == ["hip", "hip", "hip"]
    xi = torch.randn(100, 64, 2, device=dev)
    pairs = s.resample_pairs(x0, x1, noise=xi)
    f = s.sdeint(x0[:32], ts, noise=xi[:, :32])
    b = torch.flip(s.sdeint(x1[32:], ts, reverse=True, noise=xi[:, 32:]), (0,))
    assert pairs.shape == (64, 2, 2) and torch.equal(pairs, torch.cat([f, b], dim=1).transpose(0, 1))
    assert torch.equal(pairs[:32, 0], x0[:32]) and torch.equal(pairs[32:, 1], x1[32:])
    with pytest.raises(NotImplementedError, match="srk"):
        _solver(fwd, bwd, 1.0, sde_solver="srk").sdeint(x0, ts)


# ------------------------------------------------------------------------------------------- the second grid pass ----
BIG = 16 * 4096 + 5
PASS2_ROWS = (slice(0, 16), slice(16 * 2051, 16 * 2052), slice(BIG - 21, BIG))


def test_second_grid_pass_of_the_pair_ode_kernel(dev):
    """B = 16 * 4096 + 5, d = 2, hidden widths (33, 16, 24), rk4 over three output times on a non-uniform grid (a fixed-step
    solve steps exactly its t_span): ode_small_fixed_pair runs on at most 4096 workgroups, so workgroup 0 takes tile 4096
    after tile 0.  Rows of a tile do not interact: the first tile, a middle one and the last full tile with the 5-row tail
    are bit-equal to the same rows solved alone, and the tail is within 1e-5 of the float64 restatement."""
    import cnf_restate as R
    fwd, bwd = R.make_mlp(*R.mlp_params(2, (33, 16, 24), 80), dev), R.make_mlp(*R.mlp_params(2, (33, 16, 24), 81), dev)
    s = _solver(fwd, bwd, 1.0, ode_solver="rk4")
    x0 = torch.randn(BIG, 2, generator=torch.Generator().manual_seed(82)).to(dev)
    ts = torch.tensor([0.0, 0.25, 0.5, 1.0])
    big = s.odeint(x0, ts)
    assert s.last_path == "hip" and big.shape == (4, BIG, 2) and s.nfe == 12 and bool(torch.isfinite(big).all())
    for rows in PASS2_ROWS:
        alone = s.odeint(x0[rows].contiguous(), ts)
        assert s.last_path == "hip"
        assert torch.equal(big[:, rows], alone), (rows, float((big[:, rows] - alone).abs().max()))
    tail = PASS2_ROWS[-1]
    dev_ = _rel(big[:, tail].double().cpu(), _pair_f64(fwd, bwd, x0[tail], ts, "rk4"))
    print(f"pair ode rk4 B={BIG}: tail tile vs float64 {dev_:.2e}")
    assert dev_ <= 1e-5
