"""GPU (-m gpu): sdeint(..., logqp=True) on the HIP paths — the LOGQP variants of the one-launch kernels (flag bit 1 of
cfm_sde_em_mlp_f32 / cfm_sde_srk_mlp_f32), the launch-per-step path and the solver classes.

torchsde is not installable next to this suite: the column is pinned to closed forms (zero weights: the drift is the
last bias) and to the float64 eager restatement of cfm_amd.sde._run_eager on the same noise tensor (itself pinned to
closed forms in tests/test_sde_logqp_host.py).

Shapes: B in {1, 16, 17, 33} (one tile, an exact tile, a one-row tail, a three-tile grid), d in {1, 17, 64} (one lane,
a wave boundary, all four waves), hidden widths (64, 64, 64) and ragged (5, 64, 7), ts = (0, 0.25, 1) at dt = 1/8:
2 + 6 dyadic steps, two output intervals of different length.

The bound of the random-field comparisons is not a constant of this file: E32 is the largest error of the SAME
restatement run in float32 torch ops on the CPU against float64, over every input of
test_random_fields_against_the_float64_restatement (error = max |a - ref| / max |ref| over the [2, B] increments of a
case), and the GPU bound is 8 E32: the MFMA field values reassociate, the row sum has its own order, and qw is divided
beforehand.  Both are printed by the tests."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TS = [0.0, 0.25, 1.0]
DT = 0.125
N_STEPS = 8
BS = (1, 16, 17, 33)
DS = (1, 17, 64)
WIDTHS = ((64, 64, 64), (5, 64, 7))
SHAPES = [(B, d) for B in BS for d in DS]
# (name, method, sigma, reverse)
MODES = [("euler", "euler", 0.5, False), ("euler-reverse", "euler", 0.5, True),
         ("euler-schedule", "euler", "lin", False), ("euler-schedule-reverse", "euler", "lin", True),
         ("srk", "srk", 0.5, False), ("srk-reverse", "srk", 0.5, True)]
GUARD = 4096
GUARD_BYTE = 0xA5
EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _sigma(s):
    from cfm_amd.schedule import LinearDecreasingNoiseScheduler
    return LinearDecreasingNoiseScheduler(0.1, 1.0) if s == "lin" else s


def _mlp(d, widths, seed, last_scale=3.0):
    """A time-varying cfm_amd.MLP [d + 1, *widths, d] with seeded default initialisation, the last layer scaled so that
    |f| = O(1)."""
    import cfm_amd
    m = cfm_amd.MLP(dim=d, time_varying=True, w=64)
    dims = [d + 1, *widths, d]
    torch.manual_seed(seed)
    layers = []
    for k, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        if k:
            layers.append(torch.nn.SELU())
        layers.append(torch.nn.Linear(a, b))
    with torch.no_grad():
        layers[-1].weight.mul_(last_scale)
        layers[-1].bias.mul_(last_scale)
    m.net = torch.nn.Sequential(*layers)
    return m


def _const_mlp(d, widths, bias):
    """all weights zero: selu(0) = 0, the output is the last bias"""
    m = _mlp(d, widths, 0)
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
        m._linears()[-1].bias.fill_(bias)
    return m


_NETS = {}


def _pair(d, widths):
    if (d, widths) not in _NETS:
        _NETS[(d, widths)] = (_mlp(d, widths, 100 + d), _mlp(d, widths, 200 + d))
    return _NETS[(d, widths)]


def _inputs(B, d, method):
    g = torch.Generator().manual_seed(1000 * d + B)
    x0 = torch.randn((B, d), generator=g)
    xi = torch.randn((N_STEPS, 2, B, d) if method == "srk" else (N_STEPS, B, d), generator=g)
    return x0, xi


def _eager(v, s, sigma, reverse, method, x0, xi, dtype, ts=TS):
    """The restatement: cfm_amd.sde's eager scheme on plain callables (no MLP object: nothing routes it to the HIP
    paths), CPU, in `dtype`."""
    from cfm_amd.sde import DriftSDE, FlowScoreSDE, sdeint
    vn = copy.deepcopy(v.net).to(dtype)
    sde = DriftSDE(vn, sigma=sigma, reverse=reverse) if s is None else \
        FlowScoreSDE(vn, copy.deepcopy(s.net).to(dtype), sigma=sigma, reverse=reverse)
    out = sdeint(sde, x0.to(dtype), torch.tensor(ts, dtype=dtype), method=method, dt=DT, noise=xi.to(dtype), logqp=True)
    assert sde.last_path == "eager"
    return out


def _err(a, ref):
    return float((a.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


@pytest.fixture(scope="module")
def reference():
    """{(B, d, widths, mode): (trajectory, log-ratio) in float64} and E32 over all of them; computed once, never changed."""
    ref, e32 = {}, 0.0
    for B, d in SHAPES:
        for widths in WIDTHS:
            v, s = _pair(d, widths)
            for name, method, sig, rev in MODES:
                x0, xi = _inputs(B, d, method)
                r64 = _eager(v, s, _sigma(sig), rev, method, x0, xi, torch.float64)
                r32 = _eager(v, s, _sigma(sig), rev, method, x0, xi, torch.float32)
                ref[(B, d, widths, name)] = r64
                e32 = max(e32, _err(r32[1], r64[1]))
    print(f"\n[sde logqp] E32 = {e32:.3e} over {len(ref)} cases; GPU bound 8 E32 = {8 * e32:.3e}")
    return ref, e32


# ------------------------------------------------------------------------------------------------ 1. exact case
@pytest.mark.parametrize("B, d", SHAPES)
def test_zero_weights_give_the_closed_form_bit_for_bit(dev, B, d):
    """All weights zero, last biases 0.5 (flow) and 0.25 (score), sigma = 0.5: every product and sum is dyadic.  euler:
    the increments equal (t_{i+1} - t_i) d 1.125 forward and (t_{i+1} - t_i) d 0.125 in reverse, and d 0.5 both ways
    for the single field of a DriftSDE, BIT FOR BIT, under Philox noise and under a given noise tensor; srk within
    1e-6 relative (1/6 is not dyadic)."""
    from cfm_amd.sde import DriftSDE, FlowScoreSDE, sdeint
    x0, xi = _inputs(B, d, "euler")
    _, xi2 = _inputs(B, d, "srk")
    x0, xi, xi2 = x0.to(dev), xi.to(dev), xi2.to(dev)
    ts = torch.tensor(TS)
    w = torch.tensor([0.25, 0.75])[:, None].expand(2, B)
    for widths in WIDTHS:
        v, s = _const_mlp(d, widths, 0.5).to(dev), _const_mlp(d, widths, 0.25).to(dev)
        for rev, per_d in ((False, 1.125), (True, 0.125)):
            two = FlowScoreSDE(v, s, sigma=0.5, reverse=rev)
            one = DriftSDE(v, sigma=0.5, reverse=rev)
            for sde, c in ((two, per_d), (one, 0.5)):
                for noise in ("philox", xi):
                    ys, lr = sdeint(sde, x0, ts, dt=DT, noise=noise, fused=True, logqp=True)
                    assert sde.last_path == "hip" and ys.shape == (3, B, d) and lr.shape == (2, B)
                    assert torch.equal(lr.cpu(), w * (d * c)), (widths, rev, c, lr.cpu()[:, :4])
            ys, lr = sdeint(two, x0, ts, method="srk", dt=DT, noise=xi2, fused=True, logqp=True)
            err = _err(lr, (w * (d * per_d)).double())
            assert err <= 1e-6, (widths, rev, err)


# ------------------------------------------------------------------------------------------------ 2. random fields
@pytest.mark.parametrize("B, d", SHAPES)
def test_random_fields_against_the_float64_restatement(dev, reference, B, d):
    """Seeded fields with |f| = O(1), a given noise tensor, every mode of MODES and both width sets: the GPU log-ratio
    against the float64 eager restatement within 8 E32 (module docstring).  Measured (the test
    prints its own): E32 = 6.88e-07 on the CPU of the MI355X machine (5.07e-07 on the development machine's), bound
    5.50e-06, largest GPU error 1.20e-06 (B = 1, d = 1; at most 5.8e-07 at every other shape)."""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    ref, e32 = reference
    worst = 0.0
    for widths in WIDTHS:
        v, s = _pair(d, widths)
        v, s = copy.deepcopy(v).to(dev), copy.deepcopy(s).to(dev)
        for name, method, sig, rev in MODES:
            x0, xi = _inputs(B, d, method)
            sde = FlowScoreSDE(v, s, sigma=_sigma(sig), reverse=rev)
            ys, lr = sdeint(sde, x0.to(dev), torch.tensor(TS), method=method, dt=DT, noise=xi.to(dev), fused=True, logqp=True)
            assert sde.last_path == "hip"
            ys64, lr64 = ref[(B, d, widths, name)]
            assert ys.shape == ys64.shape and lr.shape == lr64.shape == (2, B)
            err = _err(lr, lr64)
            worst = max(worst, err)
            print(f"[sde logqp] B={B} d={d} widths={widths} {name}: {err:.3e} (bound {8 * e32:.3e}; state {_err(ys, ys64):.3e})")
            assert err <= 8 * e32, (widths, name, err, 8 * e32)
    print(f"[sde logqp] B={B} d={d}: worst {worst:.3e}, E32 {e32:.3e}, bound {8 * e32:.3e}")


# ------------------------------------------------------------------------------------------------ 3. trajectory bits
@pytest.mark.parametrize("B, d", [(17, 17), (33, 64), (1, 1)])
def test_the_trajectory_keeps_its_bits(dev, B, d):
    """flag bit 1 changes nothing in the state: Philox noise from the same seed, and a given noise tensor"""
    from cfm_amd.sde import DriftSDE, FlowScoreSDE, sdeint
    v, s = _pair(d, WIDTHS[0])
    v, s = copy.deepcopy(v).to(dev), copy.deepcopy(s).to(dev)
    ts = torch.tensor(TS)
    for method in ("euler", "srk"):
        x0, xi = _inputs(B, d, method)
        sdes = [FlowScoreSDE(v, s, sigma=0.5), FlowScoreSDE(v, s, sigma=0.5, reverse=True)]
        if method == "euler":
            sdes.append(DriftSDE(v, sigma=_sigma("lin"), reverse=True))
        for sde in sdes:
            for noise in ("philox", xi.to(dev)):
                gen = lambda: torch.Generator(device=dev).manual_seed(5)
                plain = sdeint(sde, x0.to(dev), ts, method=method, dt=DT, noise=noise, generator=gen(), fused=True)
                ys, lr = sdeint(sde, x0.to(dev), ts, method=method, dt=DT, noise=noise, generator=gen(), fused=True, logqp=True)
                assert torch.equal(plain, ys), (method, type(sde).__name__)
                assert bool(torch.isfinite(lr).all()) and bool((lr > 0).all())


# ------------------------------------------------------------------------------------------------ 4. fused=False
@pytest.mark.parametrize("B, d", [(17, 17), (33, 64)])
def test_one_launch_against_the_launch_per_step_path(dev, reference, B, d):
    """Trajectories bit-equal under the register-staged layer core (as tests/test_gpu_sde_srk.py compares the two paths);
    log-ratios (a few torch ops per step there) within the bound of the restatement test."""
    from cfm_amd import _lib
    from cfm_amd.sde import FlowScoreSDE, sdeint
    lib = _lib.load()
    _, e32 = reference
    glds0 = lib.cfm_mlp_get_glds()
    ts = torch.tensor(TS)
    for widths in WIDTHS:
        v, s = _pair(d, widths)
        v, s = copy.deepcopy(v).to(dev), copy.deepcopy(s).to(dev)
        for name, method, sig, rev in MODES:
            x0, xi = _inputs(B, d, method)
            sde = FlowScoreSDE(v, s, sigma=_sigma(sig), reverse=rev)
            a = sdeint(sde, x0.to(dev), ts, method=method, dt=DT, noise=xi.to(dev), fused=True, logqp=True)
            try:
                lib.cfm_mlp_set_glds(0)
                b = sdeint(sde, x0.to(dev), ts, method=method, dt=DT, noise=xi.to(dev), fused=False, logqp=True)
                plain = sdeint(sde, x0.to(dev), ts, method=method, dt=DT, noise=xi.to(dev), fused=False)
            finally:
                lib.cfm_mlp_set_glds(glds0)
            assert torch.equal(a[0], b[0]) and torch.equal(b[0], plain), (widths, name)
            assert b[1].shape == (2, B)
            err = _err(a[1], b[1].cpu())
            assert err <= 8 * e32, (widths, name, err, 8 * e32)


# ------------------------------------------------------------------------------------------------ 5. intervals
@pytest.mark.parametrize("B, d", [(17, 17), (33, 1)])
def test_increments_sum_to_the_single_interval(dev, reference, B, d):
    """ts = (0, 0.25, 1) against ts = (0, 1) on the same 8 steps and noise: a cumulative write or a missing reset shows"""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    _, e32 = reference
    v, s = _pair(d, WIDTHS[0])
    v, s = copy.deepcopy(v).to(dev), copy.deepcopy(s).to(dev)
    for name, method, sig, rev in MODES:
        x0, xi = _inputs(B, d, method)
        sde = FlowScoreSDE(v, s, sigma=_sigma(sig), reverse=rev)
        _, two = sdeint(sde, x0.to(dev), torch.tensor(TS), method=method, dt=DT, noise=xi.to(dev), fused=True, logqp=True)
        _, one = sdeint(sde, x0.to(dev), torch.tensor([0.0, 1.0]), method=method, dt=DT, noise=xi.to(dev), fused=True, logqp=True)
        assert one.shape == (1, B)
        err = _err(two.double().sum(0), one[0].cpu())
        assert err <= 8 * e32, (name, err, 8 * e32)
        assert not torch.equal(two[1], one[0])


# ------------------------------------------------------------------------------------------------ 6. memory, stream
def _guarded(nbytes, dev, fill):
    arena = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=dev)
    arena[:GUARD] = GUARD_BYTE
    arena[GUARD + nbytes:] = GUARD_BYTE
    arena[GUARD:GUARD + nbytes] = fill
    return arena, arena[GUARD:GUARD + nbytes]


def _guards_intact(arena, nbytes):
    return bool((arena[:GUARD] == GUARD_BYTE).all()) and bool((arena[GUARD + nbytes:] == GUARD_BYTE).all())


@pytest.mark.parametrize("srk", [False, True], ids=["em", "srk"])
def test_entry_in_logqp_mode_on_guarded_buffers_off_the_default_stream(dev, srk):
    """The entry itself, flags = 2 | reverse, on a stream of its own: `out` of exactly (n_out B d + n_out B) floats and `ws`
    of exactly (record + 4) n_steps bytes between poisoned guard zones (the pattern of tests/test_gpu_memory_contract.py).
    Guards untouched, every element of both outputs written (0x00 and 0xFF fills give the same bits), and a flag word
    with bit 2 set is CFM_EINVAL and writes nothing."""
    from cfm_amd import _lib
    from cfm_amd import sde as S
    lib = _lib.load()
    B, d = 33, 17
    v, s = _pair(d, WIDTHS[1])
    Wf, bf, cd, keep_f = copy.deepcopy(v).hip_params(dev)
    Ws, bs, _, keep_s = copy.deepcopy(s).hip_params(dev)
    steps = S._grid(TS, DT)
    g = [0.5] * len(steps)
    qw = S._logqp_weights(steps, g, srk)
    blob, ws_bytes = S._packed_steps(steps, g, srk, True, qw)
    assert ws_bytes == ((32 if srk else 16) + 4) * N_STEPS
    host = (ctypes.c_char * ws_bytes).from_buffer_copy(blob)
    y0 = _inputs(B, d, "euler")[0].to(dev)
    n_out = 2
    out_bytes = 4 * (n_out * B * d + n_out * B)
    fn = lib.cfm_sde_srk_mlp_f32 if srk else lib.cfm_sde_em_mlp_f32
    stream = torch.cuda.Stream()
    results = []
    for fill, flags in ((0x00, 3), (0xFF, 3), (0xFF, 3 | 4), (0xFF, 4)):
        out_arena, out = _guarded(out_bytes, dev, fill)
        ws_arena, ws = _guarded(ws_bytes, dev, fill)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rc = fn(Wf, bf, Ws, bs, cd, 4, _lib.ptr(y0), B, host, N_STEPS, flags, None, 1234, _lib.ptr(out), _lib.ptr(ws),
                    _lib.stream_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
        assert _guards_intact(out_arena, out_bytes) and _guards_intact(ws_arena, ws_bytes), (fill, flags)
        if flags & 4:
            assert rc == EINVAL
            assert bool((out == fill).all()) and bool((ws == fill).all()), "a declining call wrote"
            continue
        assert rc == 0
        assert bytes(ws.cpu().numpy().tobytes()) == blob
        words = out.view(torch.int32)
        if fill == 0xFF:
            assert not bool((words == -1).any()), "an output element was not written"
        results.append(out.clone())
    assert torch.equal(results[0], results[1])
    f = results[0].view(torch.float32)
    traj, lr = f[:n_out * B * d].view(n_out, B, d), f[n_out * B * d:].view(n_out, B)
    assert bool(torch.isfinite(traj).all()) and bool((lr > 0).all())       # (the values: the restatement test)


# ------------------------------------------------------------------------------------------------ 7. solver classes
def _time_only(m):
    """the state columns of the first layer zeroed: the field depends on t alone, so the log-ratio does not depend on
    the noise (FlowSolver.sdeint takes a generator, not a noise tensor)"""
    m = copy.deepcopy(m)
    with torch.no_grad():
        m._linears()[0].weight[:, :-1] = 0.0
    return m


def test_solver_classes_take_the_hip_path_and_match_the_eager_one(dev, reference):
    from cfm_amd.schedule import ConstantNoiseScheduler
    from cfm_amd.sde import DSBMFlowSolver, FlowSolver
    _, e32 = reference
    B, d = 17, 17
    v, s = _pair(d, WIDTHS[0])
    x0, xi = _inputs(B, d, "euler")
    t_span = torch.linspace(0, 1, 3)
    # FlowSolver, the call of the runner's validation loop (cfm_module.py:911-983: t_span + i)
    vt, st = _time_only(v), _time_only(s)
    fs = FlowSolver(copy.deepcopy(vt).to(dev), d, score_field=copy.deepcopy(st).to(dev), sigma=ConstantNoiseScheduler(0.5), dt=DT)
    traj, kl = fs.sdeint(x0.to(dev), t_span + 1, logqp=True)
    assert fs.last_path == "hip" and fs.nfe == N_STEPS and traj.shape == (3, B, d) and kl.shape == (2, B)
    xi8 = torch.randn((N_STEPS, B, d), generator=torch.Generator().manual_seed(9))
    _, want = _eager(vt, st, ConstantNoiseScheduler(0.5), False, "euler", x0, xi8, torch.float64, ts=[1.0, 1.5, 2.0])
    err = _err(kl, want)
    print(f"[sde logqp] FlowSolver: {err:.3e} (bound {8 * e32:.3e})")
    assert err <= 8 * e32, (err, 8 * e32)
    # DSBMFlowSolver in reverse: the backward net alone, on a given noise tensor
    ds = DSBMFlowSolver(copy.deepcopy(v).to(dev), d, score_field=copy.deepcopy(s).to(dev), sigma=0.5, dt=DT)
    traj, kl = ds.sdeint(x0.to(dev), torch.tensor(TS), reverse=True, noise=xi.to(dev), logqp=True)
    assert ds.last_path == "hip" and ds.nfe == N_STEPS and traj.shape == (3, B, d) and kl.shape == (2, B)
    ys64, want = _eager(s, None, 0.5, True, "euler", x0, xi, torch.float64)
    err = _err(kl, want)
    print(f"[sde logqp] DSBMFlowSolver reverse: {err:.3e} (bound {8 * e32:.3e}; state {_err(traj, ys64):.3e})")
    assert err <= 8 * e32, (err, 8 * e32)
    with pytest.raises(NotImplementedError):
        fs.sdeint(x0.to(dev), t_span, logqp=True, adaptive=True)


def test_zero_g_is_refused_before_any_launch(dev):
    from cfm_amd.sde import FlowScoreSDE, sdeint
    v, s = _pair(1, WIDTHS[0])
    sde = FlowScoreSDE(copy.deepcopy(v).to(dev), copy.deepcopy(s).to(dev), sigma=0.0)
    x0 = torch.zeros((2, 1), device=dev)
    assert torch.is_tensor(sdeint(sde, x0, torch.tensor(TS), dt=DT))           # without logqp sigma = 0 is an ODE
    with pytest.raises(ValueError, match="g = 0"):
        sdeint(sde, x0, torch.tensor(TS), dt=DT, logqp=True)


# ------------------------------------------------------------------------------------------------ 8. second grid pass
BIG = 16 * 4096 + 5
PASS2_TS = [0.0, 0.25, 0.5, 1.0]                           # at DT = 1/8: 2 + 2 + 4 steps, three output intervals
PASS2_ROWS = (slice(0, 16), slice(16 * 2051, 16 * 2052), slice(BIG - 21, BIG))
PASS2_MODES = [m for m in MODES if m[2] == 0.5]             # euler and srk at a constant sigma, forward and reverse


@pytest.mark.parametrize("name, method, sig, rev", PASS2_MODES, ids=[m[0] for m in PASS2_MODES])
def test_second_grid_pass_keeps_the_rows_and_the_log_ratio(dev, reference, name, method, sig, rev):
    """B = 16 * 4096 + 5, d = 2, hidden widths (33, 16, 24): more than the 4096 workgroups of a launch, so workgroup 0 runs
    tile 4096 after tile 0 — on the `red` scratch of sm_rowsum, the wave-0 store of `logratio` and the output index of its
    first pass.  Rows of a tile do not interact (the row sum runs over columns), so the first tile, a middle one and the
    last full tile with the 5-row tail are bit-equal, state and log-ratio, to the same rows run alone on the same noise
    rows; the state is the bits of the run without logqp; and the tail's log-ratio is held to the bound of the restatement
    test (8 E32) against the float64 eager scheme."""
    import cnf_restate as R
    from cfm_amd.sde import FlowScoreSDE, sdeint
    d = 2
    v, s = R.make_mlp(*R.mlp_params(d, (33, 16, 24), 70)), R.make_mlp(*R.mlp_params(d, (33, 16, 24), 71))
    _, e32 = reference
    g = torch.Generator().manual_seed(72)
    x0 = torch.randn((BIG, d), generator=g)
    xi = torch.randn((N_STEPS, 2, BIG, d) if method == "srk" else (N_STEPS, BIG, d), generator=g)
    sde = FlowScoreSDE(copy.deepcopy(v).to(dev), copy.deepcopy(s).to(dev), sigma=_sigma(sig), reverse=rev)
    ts = torch.tensor(PASS2_TS)

    def run(x, z, logqp=True):
        out = sdeint(sde, x.to(dev), ts, method=method, dt=DT, noise=z.contiguous().to(dev), fused=True, logqp=logqp)
        return (out[0].cpu(), out[1].cpu()) if logqp else out.cpu()
    ys, lr = run(x0, xi)
    assert sde.last_path == "hip" and ys.shape == (4, BIG, d) and lr.shape == (3, BIG)
    assert bool(torch.isfinite(lr).all()) and bool((lr > 0).all())
    assert torch.equal(ys, run(x0, xi, logqp=False))
    for rows in PASS2_ROWS:
        ya, la = run(x0[rows], xi[..., rows, :])
        assert torch.equal(ys[:, rows], ya), rows
        assert torch.equal(lr[:, rows], la), (rows, float((lr[:, rows] - la).abs().max()))
    tail = PASS2_ROWS[-1]
    ys64, lr64 = _eager(v, s, _sigma(sig), rev, method, x0[tail], xi[..., tail, :], torch.float64, ts=PASS2_TS)
    err = _err(lr[:, tail], lr64)
    print(f"[sde logqp] B={BIG} {name}: tail tile {err:.3e} (bound {8 * e32:.3e}; state {_err(ys[:, tail], ys64):.3e})")
    assert err <= 8 * e32, (name, err, 8 * e32)
