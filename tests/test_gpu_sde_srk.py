"""GPU (-m gpu): sdeint(method="srk") — the one-launch sampler (cfm_sde_srk_mlp_f32), the launch-per-step path
(cfm_sde_srk_step_f32) and the Philox mode.

torchsde is not installable next to this suite: the scheme is pinned to a float64 restatement that lives here and to
the CPU tests of tests/test_sde_srk_host.py (strong order, SSPRK3 limit)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cfm_oracle as oracle

pytestmark = pytest.mark.gpu

SQ3 = math.sqrt(3.0)
NONUNIFORM = [0.0, 0.13, 0.5, 1.0]


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _two_fields(dev, d=2, w=64, seed=0):
    import cfm_amd
    torch.manual_seed(seed)
    return cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev), cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)


def _np_params(net):
    return ([l.weight.detach().cpu().numpy() for l in net._linears()], [l.bias.detach().cpu().numpy() for l in net._linears()])


def _restatement(v, s, y0, ts, dt, sigma, xi, reverse=False):
    """the scheme in float64 on the same noise: trajectory [len(ts), B, d]"""
    from cfm_amd.sde import _grid
    Wv, bv = _np_params(v)
    Ws, bs = _np_params(s)

    def f(t, y):
        te = 1.0 - t if reverse else t
        fl = oracle.mlp_forward_f64(Wv, bv, y, te)
        return (-fl if reverse else fl) + oracle.mlp_forward_f64(Ws, bs, y, te)
    y = np.asarray(y0, dtype=np.float64)
    xi = np.asarray(xi, dtype=np.float64)
    out = [y]
    for k, (t, h, is_out) in enumerate(_grid(ts, dt)):
        x1, x2 = xi[k, 0], xi[k, 1]
        k1 = f(t, y)
        k2 = f(t + h, y + h * k1)
        k3 = f(t + h / 2, y + (h / 4) * (k1 + k2) + 0.75 * sigma * math.sqrt(h) * (x1 + x2 / SQ3))
        y = y + h * (k1 / 6 + k2 / 6 + (2.0 / 3.0) * k3) + sigma * math.sqrt(h) * x1
        if is_out:
            out.append(y)
    return np.stack(out)


def _n_steps(ts, dt):
    from cfm_amd.sde import _grid
    return len(_grid(ts, dt))


def test_fused_sampler_is_bit_equal_to_the_launch_per_step_scheme(dev):
    """cfm_sde_srk_mlp_f32 with the caller's noise against three forward passes per field + cfm_sde_srk_step_f32 per
    step: same bits under the register-staged layer core (cfm_mlp_set_glds(0)), forward and reverse time, and within
    1e-5 of the path on the default layer engine (another fixed summation order)."""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    from cfm_amd import _lib
    lib = _lib.load()
    glds0 = lib.cfm_mlp_get_glds()
    for d, w, rev in ((2, 64, False), (2, 64, True), (50, 64, False), (5, 32, False)):
        v, s = _two_fields(dev, d=d, w=w, seed=11 + d)
        x0 = torch.randn(300, d, generator=torch.Generator().manual_seed(d)).to(dev)
        ts = torch.linspace(0, 1, 6)
        sde = FlowScoreSDE(v, s, sigma=0.4, reverse=rev)
        gen = lambda: torch.Generator(device=dev).manual_seed(3)
        a = sdeint(sde, x0, ts, method="srk", dt=0.05, generator=gen(), noise="torch", fused=True)
        try:
            lib.cfm_mlp_set_glds(0)
            b = sdeint(sde, x0, ts, method="srk", dt=0.05, generator=gen(), noise="torch", fused=False)
            lib.cfm_mlp_set_glds(glds0)
            c = sdeint(sde, x0, ts, method="srk", dt=0.05, generator=gen(), noise="torch", fused=False)
        finally:
            lib.cfm_mlp_set_glds(glds0)
        assert a.shape == b.shape == (6, 300, d)
        assert torch.equal(a.cpu(), b.cpu()), float((a.cpu() - b.cpu()).abs().max())
        dev_c = float((a.cpu() - c.cpu()).abs().max())
        print(f"d={d} w={w} reverse={rev}: fused vs default-engine stepping {dev_c:.3e} (max|a| {float(a.abs().max()):.3f})")
        assert dev_c <= 1e-5 * float(a.abs().max())
        # a noise tensor is the same thing as the seeded torch draws
        g = gen()
        xi = torch.stack([torch.randn((2, 300, d), device=dev, generator=g) for _ in range(20)])
        assert torch.equal(a, sdeint(sde, x0, ts, method="srk", dt=0.05, noise=xi, fused=True))


@pytest.mark.parametrize("d", [2, 64])
@pytest.mark.parametrize("B", [1, 16, 17, 300])
def test_fused_sampler_against_the_float64_restatement(dev, B, d):
    """One step, 20 steps and the non-uniform grid refined to dt = 0.1, on the same noise tensor: <= 2e-5 max|ref|
    (the bound the Euler scheme's eager comparison uses at this shape)."""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    v, s = _two_fields(dev, d=d, w=64, seed=20 + d)
    g = torch.Generator().manual_seed(100 * d + B)
    x0 = torch.randn((B, d), generator=g)
    for name, ts, dt, rev in (("one step", [0.0, 1.0], 1.0, False), ("20 steps", list(np.linspace(0.0, 1.0, 5)), 0.05, False),
                              ("non-uniform", NONUNIFORM, 0.1, False), ("non-uniform reverse", NONUNIFORM, 0.1, True)):
        n = _n_steps(ts, dt)
        xi = torch.randn((n, 2, B, d), generator=g)
        tr = sdeint(FlowScoreSDE(v, s, sigma=0.7, reverse=rev), x0.to(dev), torch.tensor(ts), method="srk", dt=dt,
                    noise=xi.to(dev), fused=True).cpu().numpy()
        ref = _restatement(v, s, x0.numpy(), ts, dt, 0.7, xi.numpy(), reverse=rev)
        assert tr.shape == ref.shape == (len(ts), B, d)
        err = np.abs(tr - ref).max() / np.abs(ref).max()
        print(f"B={B} d={d} {name} ({n} steps): {err:.3e} of max|ref|")
        assert err <= 2e-5, (name, err)


# ---- non-square hidden layers: both fields are staged layer by layer from four different shapes ----
WMIX, WMIX2 = (64, 17, 40), (33, 64, 48)


def _two_mixed_fields(dev, d, w, seed):
    """Drift and score nets [d + 1, *w, d] (the same layer sizes, as the one-launch kernels need; different weights)."""
    import cnf_restate as R
    return R.make_mlp(*R.mlp_params(d, w, seed), dev), R.make_mlp(*R.mlp_params(d, w, seed + 1), dev)


def _em_restatement(v, s, y0, ts, dt, sigma, xi, reverse=False):
    """Euler-Maruyama in float64 on the same noise: y += h (drift + score) + sigma sqrt(h) xi; [len(ts), B, d]"""
    from cfm_amd.sde import _grid
    Wv, bv = _np_params(v)
    Ws, bs = _np_params(s)
    y = np.asarray(y0, dtype=np.float64)
    xi = np.asarray(xi, dtype=np.float64)
    out = [y]
    for k, (t, h, is_out) in enumerate(_grid(ts, dt)):
        te = 1.0 - t if reverse else t
        fl = oracle.mlp_forward_f64(Wv, bv, y, te)
        y = y + h * ((-fl if reverse else fl) + oracle.mlp_forward_f64(Ws, bs, y, te)) + sigma * math.sqrt(h) * xi[k]
        if is_out:
            out.append(y)
    return np.stack(out)


def _fused_and_stepped(dev, sde, x0, ts, method, dt, xi):
    """The one-launch sampler, and the launch-per-step scheme on the register-staged layer core (whose k order the
    fused kernels share), on the same noise tensor."""
    from cfm_amd.sde import sdeint
    from cfm_amd import _lib
    lib = _lib.load()
    a = sdeint(sde, x0.to(dev), torch.tensor(ts), method=method, dt=dt, noise=xi.to(dev), fused=True).cpu()
    glds0 = lib.cfm_mlp_get_glds()
    try:
        lib.cfm_mlp_set_glds(0)
        b = sdeint(sde, x0.to(dev), torch.tensor(ts), method=method, dt=dt, noise=xi.to(dev), fused=False).cpu()
    finally:
        lib.cfm_mlp_set_glds(glds0)
    return a, b


@pytest.mark.parametrize("w", [WMIX, WMIX2], ids=lambda w: "-".join(map(str, w)))
@pytest.mark.parametrize("d", [2, 64])
def test_fused_sampler_against_the_float64_restatement_at_non_square_widths(dev, d, w):
    """test_fused_sampler_against_the_float64_restatement (same grids, same bound) with both nets at non-square widths
    and a partial second tile; and the same bits as the launch-per-step scheme."""
    from cfm_amd.sde import FlowScoreSDE
    B = 17
    v, s = _two_mixed_fields(dev, d, w, seed=20 + d)
    assert [l.out_features for l in v._linears()] == [l.out_features for l in s._linears()] == list(w) + [d]
    g = torch.Generator().manual_seed(100 * d + B)
    x0 = torch.randn((B, d), generator=g)
    for name, ts, dt, rev in (("one step", [0.0, 1.0], 1.0, False), ("20 steps", list(np.linspace(0.0, 1.0, 5)), 0.05, False),
                              ("non-uniform", NONUNIFORM, 0.1, False), ("non-uniform reverse", NONUNIFORM, 0.1, True)):
        n = _n_steps(ts, dt)
        xi = torch.randn((n, 2, B, d), generator=g)
        a, b = _fused_and_stepped(dev, FlowScoreSDE(v, s, sigma=0.7, reverse=rev), x0, ts, "srk", dt, xi)
        ref = _restatement(v, s, x0.numpy(), ts, dt, 0.7, xi.numpy(), reverse=rev)
        assert a.shape == ref.shape == (len(ts), B, d)
        err = np.abs(a.numpy() - ref).max() / np.abs(ref).max()
        print(f"srk B={B} d={d} w={w} {name} ({n} steps): {err:.3e} of max|ref|")
        assert err <= 2e-5, (name, err)
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


@pytest.mark.parametrize("w", [WMIX, WMIX2], ids=lambda w: "-".join(map(str, w)))
@pytest.mark.parametrize("d", [2, 64])
def test_fused_euler_maruyama_against_the_float64_restatement_at_non_square_widths(dev, d, w):
    """cfm_sde_em_mlp_f32 (method="euler") on the grids and under the bound of the srk test above (2e-5 max|ref|, this
    file's bound for a sampler that carries an fp32 state through 20 steps of two fp32 fields), B = 17; and the same
    bits as two forward passes + cfm_sde_em_step_f32 per step."""
    from cfm_amd.sde import FlowScoreSDE
    B = 17
    v, s = _two_mixed_fields(dev, d, w, seed=40 + d)
    g = torch.Generator().manual_seed(300 * d + B)
    x0 = torch.randn((B, d), generator=g)
    for name, ts, dt, rev in (("one step", [0.0, 1.0], 1.0, False), ("20 steps", list(np.linspace(0.0, 1.0, 5)), 0.05, False),
                              ("non-uniform", NONUNIFORM, 0.1, False), ("non-uniform reverse", NONUNIFORM, 0.1, True)):
        n = _n_steps(ts, dt)
        xi = torch.randn((n, B, d), generator=g)
        a, b = _fused_and_stepped(dev, FlowScoreSDE(v, s, sigma=0.7, reverse=rev), x0, ts, "euler", dt, xi)
        ref = _em_restatement(v, s, x0.numpy(), ts, dt, 0.7, xi.numpy(), reverse=rev)
        assert a.shape == ref.shape == (len(ts), B, d)
        err = np.abs(a.numpy() - ref).max() / np.abs(ref).max()
        print(f"euler B={B} d={d} w={w} {name} ({n} steps): {err:.3e} of max|ref|")
        assert err <= 2e-5, (name, err)
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def test_wide_fields_take_the_launch_per_step_path(dev):
    from cfm_amd.sde import FlowScoreSDE, sdeint
    v, s = _two_fields(dev, d=3, w=128, seed=31)
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn((37, 3), generator=g)
    xi = torch.randn((11, 2, 37, 3), generator=g)
    sde = FlowScoreSDE(v, s, sigma=0.7)
    tr = sdeint(sde, x0.to(dev), torch.tensor(NONUNIFORM), method="srk", dt=0.1, noise=xi.to(dev)).cpu().numpy()
    ref = _restatement(v, s, x0.numpy(), NONUNIFORM, 0.1, 0.7, xi.numpy())
    err = np.abs(tr - ref).max() / np.abs(ref).max()
    print(f"w=128 launch-per-step: {err:.3e} of max|ref|")
    assert tr.shape == ref.shape and err <= 2e-5
    with pytest.raises(ValueError, match="fused=True"):
        sdeint(sde, x0.to(dev), torch.tensor(NONUNIFORM), method="srk", dt=0.1, noise=xi.to(dev), fused=True)
    with pytest.raises(ValueError, match=r"\[11, 2, 37, 3\]"):
        sdeint(sde, x0.to(dev), torch.tensor(NONUNIFORM), method="srk", dt=0.1, noise=xi[:, 0].to(dev))


def test_philox_mode_is_repeatable_and_brownian(dev):
    from cfm_amd.sde import FlowScoreSDE, sdeint
    v, s = _two_fields(dev, seed=5)
    sde = FlowScoreSDE(v, s, sigma=0.5)
    x0 = oracle.eight_gaussians(512, 2).to(dev)
    ts = torch.linspace(0, 1, 3)
    torch.manual_seed(123); p1 = sdeint(sde, x0, ts, method="srk", dt=0.02)
    torch.manual_seed(123); p2 = sdeint(sde, x0, ts, method="srk", dt=0.02)
    torch.manual_seed(124); p3 = sdeint(sde, x0, ts, method="srk", dt=0.02)
    assert p1.shape == (3, 512, 2) and torch.equal(p1, p2) and not torch.equal(p1, p3)
    for net in (v, s):
        for p in net.parameters():
            p.data.zero_()
    y = sdeint(FlowScoreSDE(v, s, sigma=2.0), torch.zeros(40000, 2), torch.tensor([0.0, 1.0]), method="srk", dt=0.01)
    inc = (y[-1] - y[0]).double()
    assert abs(float(inc.var()) - 4.0) < 0.1 and abs(float(inc.mean())) < 0.03
    z = inc / 2.0
    assert abs(float((z ** 4).mean()) - 3.0) < 0.15
    assert abs(float((z[:, 0] * z[:, 1]).mean())) < 0.02


def _moment_gap(a, b):
    """per coordinate: |mean_a - mean_b| and |var_a - var_b| in standard errors estimated from the two samples"""
    a, b = a.double().cpu(), b.double().cpu()
    n = a.shape[0]
    va, vb = a.var(0), b.var(0)
    zm = (a.mean(0) - b.mean(0)).abs() / ((va + vb) / n).sqrt()
    m4a, m4b = ((a - a.mean(0)) ** 4).mean(0), ((b - b.mean(0)) ** 4).mean(0)
    zv = (va - vb).abs() / (((m4a - va ** 2) + (m4b - vb ** 2)) / n).sqrt()
    return float(zm.max()), float(zv.max())


def test_philox_xi2_is_independent_of_xi1(dev):
    """One step of h = 1 from one point, B = 40000, d = 2, random w = 64 fields (seed 45), sigma = 1.0.  xi2 reaches the
    endpoint only through the third stage's state, so the endpoint's moments tell whether it is a fresh normal: under
    noise="philox" they agree with noise="torch" within 5 standard errors, and an injected tensor with xi2 := xi1 does
    not (the check has power).

    Values used: the first pair tried (field seed 41, sigma = 1.5) put the xi2 := xi1 variance 3.4 standard errors off
    on the float32 eager scheme — too little.  The gap is first order in the fields' Jacobian J (the covariance of
    (2/3) h k3 with sigma xi1 grows by the factor 1 + 1/sqrt(3)), about 0.58 sigma^2 J against a standard error of
    about 0.01 sigma^2, so it does not grow with sigma (seed 41: 5.8 / 4.4 / 1.8 standard errors at sigma = 0.5 / 1 /
    3); what helps is a pair of fields with a larger Jacobian at the start point.  Field seed 45 at sigma = 1.0 gives
    11.3 standard errors on the eager scheme (14.5 at sigma = 0.5, 5.9 at 3); on the MI355X with the draws below:
    philox against torch 2.1 (mean) / 0.8 (variance) standard errors, xi2 := xi1 against torch 2.4 / 8.0."""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    v, s = _two_fields(dev, seed=45)
    B, sigma = 40000, 1.0
    sde = FlowScoreSDE(v, s, sigma=sigma)
    x0 = torch.tensor([[0.3, -0.2]]).repeat(B, 1).to(dev)
    ts = torch.tensor([0.0, 1.0])
    torch.manual_seed(9)
    a = sdeint(sde, x0, ts, method="srk", dt=1.0, noise="philox")[-1]
    b = sdeint(sde, x0, ts, method="srk", dt=1.0, noise="torch", generator=torch.Generator(device=dev).manual_seed(10))[-1]
    xi = torch.randn((1, 2, B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(11))
    xi[:, 1] = xi[:, 0]
    c = sdeint(sde, x0, ts, method="srk", dt=1.0, noise=xi)[-1]
    zm, zv = _moment_gap(a, b)
    zm_bad, zv_bad = _moment_gap(c, b)
    print(f"philox vs torch: mean {zm:.2f} se, var {zv:.2f} se;  xi2 := xi1 vs torch: mean {zm_bad:.2f} se, var {zv_bad:.2f} se")
    assert zm <= 5.0 and zv <= 5.0
    assert max(zm_bad, zv_bad) > 5.0


def test_c_entry_rejects_what_the_kernel_is_not_built_for(dev):
    from cfm_amd import _lib
    from cfm_amd._lib import ptr
    lib = _lib.load()
    v, s = _two_fields(dev, d=2, w=64, seed=1)
    Wf, bf, dims, keep_f = v.hip_params(dev)
    Ws, bs, _, keep_s = s.hip_params(dev)
    y0 = torch.zeros((4, 2), device=dev)
    out = torch.zeros((1, 4, 2), device=dev)
    ws = torch.zeros(512, dtype=torch.uint8, device=dev)
    host = (ctypes.c_char * 32)()
    EINVAL = -1

    def call(Wf=Wf, bf=bf, dims=dims, n_layers=4, y0p=ptr(y0), B=4, hostp=host, n_steps=1, outp=ptr(out), wsp=ptr(ws)):
        return lib.cfm_sde_srk_mlp_f32(Wf, bf, Ws, bs, dims, n_layers, y0p, B, hostp, n_steps, 0, None, 0, outp, wsp, None)
    assert call(n_layers=3) == EINVAL and call(n_layers=5) == EINVAL
    wide = (ctypes.c_int * 5)(3, 65, 64, 64, 2)
    assert call(dims=wide) == EINVAL
    assert call(dims=(ctypes.c_int * 5)(66, 64, 64, 64, 65)) == EINVAL
    assert call(dims=(ctypes.c_int * 5)(2, 64, 64, 64, 2)) == EINVAL          # no time column
    for kw in (dict(Wf=None), dict(bf=None), dict(dims=None), dict(y0p=None), dict(hostp=None), dict(outp=None), dict(wsp=None)):
        assert call(**kw) == EINVAL, kw
    assert call(B=0) == 0 and call(n_steps=0) == 0
    torch.cuda.synchronize()


# ---- the second grid pass: more than 4096 tiles, so workgroup 0 runs tile 4096 after tile 0 ----
BIG = 16 * 4096 + 5
PASS2_TS, PASS2_DT = [0.0, 0.25, 0.5, 1.0], 0.25          # 1 + 1 + 2 steps: the last output is reached through a refined step
# the first tile, a middle one, and the last full tile with the 5-row tail behind it (workgroups 4095 and 0 again)
PASS2_ROWS = (slice(0, 16), slice(16 * 2051, 16 * 2052), slice(BIG - 21, BIG))


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("method", ["euler", "srk"])
def test_second_grid_pass_on_a_given_noise_tensor(dev, method, reverse):
    """B = 16 * 4096 + 5, d = 2, hidden widths (33, 16, 24): small_grid caps the launch at 4096 workgroups, so the row loop of
    ode_small_em / ode_small_srk takes a second pass, on the LDS tile buffers and the output index of the first.  Rows of
    a tile do not interact in these kernels, so the rows of PASS2_ROWS are bit-equal to the same rows run alone as a
    small batch on the same noise rows; and the tail tile is held to this file's bound against the float64 restatement."""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    d, srk = 2, method == "srk"
    v, s = _two_mixed_fields(dev, d, (33, 16, 24), seed=60)
    g = torch.Generator().manual_seed(61)
    x0 = torch.randn((BIG, d), generator=g)
    n = _n_steps(PASS2_TS, PASS2_DT)
    assert n == 4
    xi = torch.randn((n, 2, BIG, d) if srk else (n, BIG, d), generator=g)
    sde = FlowScoreSDE(v, s, sigma=0.7, reverse=reverse)
    run = lambda x, z: sdeint(sde, x.to(dev), torch.tensor(PASS2_TS), method=method, dt=PASS2_DT, noise=z.contiguous().to(dev),
                              fused=True).cpu()
    big = run(x0, xi)
    assert sde.last_path == "hip" and big.shape == (4, BIG, d) and bool(torch.isfinite(big).all())
    for rows in PASS2_ROWS:
        alone = run(x0[rows], xi[..., rows, :])
        assert torch.equal(big[:, rows], alone), (rows, float((big[:, rows] - alone).abs().max()))
    tail = PASS2_ROWS[-1]
    ref = (_restatement if srk else _em_restatement)(v, s, x0[tail].numpy(), PASS2_TS, PASS2_DT, 0.7, xi[..., tail, :].numpy(),
                                                     reverse=reverse)
    err = np.abs(big[:, tail].numpy() - ref).max() / np.abs(ref).max()
    print(f"{method} reverse={reverse} B={BIG}: tail tile {err:.3e} of max|ref|")
    assert err <= 2e-5, err
