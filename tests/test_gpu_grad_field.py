"""GPU (-m gpu): the action-matching field v = grad_x s(x, t) on the fused kernels — cfm_mlp_grad_field_f32, the
cfm_ode_*_gradmlp_f32 solves and the augmented cfm_ode_fixed_cnf_gradmlp_f32 — against the float64 restatement of
tests/grad_field_restate.py and the float64 integrators of oracle/cfm_oracle.py and tests/ode_rk_ref.py.

The kink rule.  v is discontinuous where a hidden pre-activation crosses 0 (selu' jumps from 1.758 to 1.051), so an fp32
evaluation within rounding of a kink may legitimately take the other side.  Rows whose float64 restatement comes within
1e-5 of a kink (for solves: at any stage point of the float64 solve) are dropped BEFORE anything runs; a test FAILS when
more than 2 % of the rows of a field case or 15 % of the rows of a trajectory case are dropped.  The seeds below were
checked on the CPU against these caps (the checks are the asserts in _kept)."""
import ctypes

import numpy as np
import pytest
import torch

import cfm_oracle as oracle
import cnf_restate as R
import grad_field_restate as G
import ode_rk_ref as rk

pytestmark = pytest.mark.gpu

STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
WIDTHS = [(64, 64, 64), (33, 33, 33), (64, 17, 40)]
FIELD_B = (1, 16, 17, 40, 4096)          # 4096: more than one workgroup, and enough rows for the 2 % cap to mean something
UNIFORM = np.linspace(0.0, 1.0, 21).astype(np.float32)
NONUNIFORM = np.array([0.0, 0.05, 0.2, 0.25, 0.5, 0.55, 0.9, 1.0], dtype=np.float32)


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _x(B, d, seed):
    return (2.0 * np.random.default_rng(seed).standard_normal((B, d))).astype(np.float32)


def _kept(clear, cap, what):
    dropped = int((~clear).sum())
    print(what, "rows dropped by the kink rule:", dropped, "of", len(clear))
    assert dropped <= cap * len(clear), (what, dropped, len(clear))
    return clear


def _hip(Ws, bs, dev):
    from cfm_amd import _lib
    a = G.make_action(Ws, bs, dev)
    Wp, bp, dims, keep = a.hip_params(dev)
    return _lib.load(), a, (Wp, bp, dims, keep)


def _field(lib, hp, xd, ldx, B, d, t, lap, dev):
    from cfm_amd import _lib
    v = torch.full((B, d), float("nan"), device=dev)
    lp = torch.full((B,), float("nan"), device=dev) if lap else None
    _lib.check(lib.cfm_mlp_grad_field_f32(hp[0], hp[1], hp[2], 4, _lib.ptr(xd), ldx, B, t, _lib.ptr(v), _lib.ptr(lp), None,
                                          _lib.stream_ptr()), "cfm_mlp_grad_field_f32")
    return v, lp


def _node(Ws, bs, solver, dev, tol=1e-5, cnf=False, **kw):
    import cfm_amd
    from cfm_amd.models import GradModel
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    gm = GradModel(G.make_action(Ws, bs, dev))
    return NeuralODE(cfm_amd.CNF(gm, **kw) if cnf else torch_wrapper(gm), solver=solver, atol=tol, rtol=tol)


# ------------------------------------------------------------------------------------------------------ 1, 2: field
@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("d", [1, 2, 5, 63])
def test_field_and_laplacian_vs_float64(dev, d, widths):
    from cfm_amd.models import GradModel
    Ws, bs = G.action_params(d, widths, seed=d % 3)
    lib, a, hp = _hip(Ws, bs, dev)
    gm = GradModel(a)
    with_lap = d <= 5
    cases, clear = [], []
    for B in FIELD_B:
        for t in (0.0, 0.37):
            x = _x(B, d, 100 + B)
            cases.append((B, t, x))
            clear.append(G.min_abs_preactivation(Ws, bs, t, x) > 1e-5)
    _kept(np.concatenate(clear), 0.02, f"field d={d} widths={widths}")
    for (B, t, x), keep in zip(cases, clear):
        ref = G.grad_field(Ws, bs, t, x, laplacian=with_lap)
        vref, lref = ref if with_lap else (ref, None)
        xd = torch.from_numpy(x).to(dev)
        v, _ = _field(lib, hp, xd, d, B, d, t, False, dev)
        if keep.any():
            err = np.abs(v.cpu().numpy() - vref)[keep].max() / np.abs(vref[keep]).max()
            print(f"B={B} t={t}: max|v - v64| / max|v64| = {err:.3g}")
            assert err <= 1e-5, (B, t, err)
        # GradModel.forward under no_grad: the same launch, x at a row stride of d + 1 inside [x, t]
        with torch.no_grad():
            vg = gm(torch.cat([xd, torch.full((B, 1), t, device=dev)], 1))
        assert torch.equal(vg, v), (B, t)
        # a strided x
        pad = torch.full((B, d + 3), 7.0, device=dev)
        pad[:, :d] = xd
        vs, _ = _field(lib, hp, pad, d + 3, B, d, t, False, dev)
        assert torch.equal(vs, v), (B, t)
        # lap given or not: bitwise the same v
        vl, lap = _field(lib, hp, xd, d, B, d, t, True, dev)
        assert torch.equal(vl, v), (B, t)
        if with_lap and keep.any():
            # tolerance (the rule of test_gpu_cnf.py for tr J): 2e-5 of sum_k |H_kk| plus 1e-6 of the magnitudes of
            # the terms whose sum the H_kk are (an entry that cancels is known to fp32 only to its terms' rounding)
            diag, mag = G.laplacian_terms(Ws, bs, t, x)
            e = (np.abs(lap.cpu().numpy() - lref) / (2e-5 * diag + 1e-6 * mag))[keep].max()
            print(f"B={B} t={t}: Laplacian error / tolerance = {e:.3g}")
            assert e <= 1.0, (B, t, e)


# ------------------------------------------------------------------------------------------------------ 3: fixed steps
# (B, d, widths, net seed, scale of W3, seed of x0).  W3 is scaled by 8 so that the states move by ~1 over [0, 1].  Every
# evaluation of a row comes within 1e-5 of some kink with probability ~0.3 % (192 hidden units; the field cases above
# measure it), so an rk4 solve of 20 steps loses ~20 % of its rows on average whatever the net: the x0 seeds are the first
# ones of a CPU search for which all twelve (solver, grid, direction) solves of a case stay within the 15 % cap.
FIXED_CASES = {"b40_d2_w64": (40, 2, (64, 64, 64), 0, 8.0, 25), "b17_d5_w33": (17, 5, (33, 33, 33), 0, 8.0, 0)}
_FIXED_REF = {}


def _fixed_ref(case, solver, grid, down):
    """float64 solve + the rows kept by the kink rule, computed once per (case, solver, grid, direction)"""
    key = (case, solver, grid, down)
    if key not in _FIXED_REF:
        B, d, widths, seed, scale, xseed = FIXED_CASES[case]
        Ws, bs = G.action_params(d, widths, seed, out_scale=scale)
        ts = {"uniform": UNIFORM, "nonuniform": NONUNIFORM}[grid]
        ts = ts[::-1].copy() if down else ts
        x0 = _x(B, d, xseed)
        watch = G.KinkWatch(Ws, bs, G.field_np(Ws, bs))
        ref = oracle.euler_trajectory(watch, x0, ts) if solver == "euler" else rk.fixed_trajectory(watch, x0, ts, solver)
        keep = _kept(watch.clear(), 0.15, f"{case} {solver} {grid} {'down' if down else 'up'}")
        assert np.abs(ref[-1] - ref[0]).max() >= 0.05            # the trajectories move
        _FIXED_REF[key] = (Ws, bs, ts, x0, ref, keep)
    return _FIXED_REF[key]


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("grid", ["uniform", "nonuniform"])
@pytest.mark.parametrize("solver", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("case", list(FIXED_CASES))
def test_fixed_step_solves_vs_float64(dev, case, solver, grid, down):
    Ws, bs, ts, x0, ref, keep = _fixed_ref(case, solver, grid, down)
    node = _node(Ws, bs, solver, dev)
    tr = node.trajectory(torch.from_numpy(x0).to(dev), torch.from_numpy(ts))
    assert node.last_path == "hip" and tr.shape == ref.shape
    assert (node.n_steps, node.nfe) == (len(ts) - 1, STAGES[solver] * (len(ts) - 1))
    assert torch.equal(tr[0].cpu(), torch.from_numpy(x0))
    err = np.abs(tr.cpu().numpy() - ref)[:, keep].max() / np.abs(ref[:, keep]).max()
    print(f"{case} {solver} {grid} down={down}: max|x - x64| / max|x64| = {err:.3g}")
    assert err <= 1e-5, err
    if solver == "euler":
        # the first step is x0 + h v of the one-evaluation entry (the kernel fuses it into one fma: within 2 ulp)
        lib, a, hp = _hip(Ws, bs, dev)
        B, d = x0.shape
        xd = torch.from_numpy(x0).to(dev)
        v, _ = _field(lib, hp, xd, d, B, d, float(ts[0]), False, dev)
        step = (xd + float(np.float32(ts[1] - ts[0])) * v).cpu().numpy()
        got = tr[1].cpu().numpy()
        assert np.all(np.abs(got - step) <= 2 * np.spacing(np.maximum(np.abs(got), np.abs(step))))


# ------------------------------------------------------------------------------------------------------ 4: adaptive
_ADAPT_REF = {}
ADAPT_TS = np.array([0.0, 0.1, 0.2], dtype=np.float32)


def _adaptive_solve(solver, f, x0, ts):
    if solver == "dopri5":
        return oracle.dopri5_trajectory(f, x0, ts, 1e-5, 1e-5, return_log=True)
    return rk.adaptive_trajectory(f, x0, ts, 1e-5, 1e-5, "tsit5", return_log=True)


def _counts_survive_fp32(solver, f, x0, ts, info):
    """The step sequence of a case must not hang on the rounding of the field: at atol = rtol = 1e-5 an fp32 field
    (relative error ~1e-6, measured) moves an error ratio by ~1e-3, which is MORE than the ratio of a cautious first
    step, so the step-size factor after it (0.9 / ratio^0.2, anywhere in 3 .. 10) is rounding's to choose.  The float64
    solve is therefore repeated with Gaussian noise of 2e-6 max|v| on every evaluation, and must take the same
    attempts."""
    for seed in range(3):
        g = np.random.default_rng(100 + seed)

        def noisy(t, y):
            v = f(t, y)
            return v + 2e-6 * np.abs(v).max() * g.standard_normal(v.shape)
        _, i2 = _adaptive_solve(solver, noisy, x0, ts)
        if (i2["steps"], i2["nfe"]) != (info["steps"], info["nfe"]):
            return False
    return True


def _adaptive_ref(solver, B, down):
    """A smooth action (every hidden pre-activation negative on [-4, 4]^2 x [-1, 1]) with W3 scaled by 300, on the grid
    [0, 0.1, 0.2].  The initial step comes out at ~0.06: short of the first grid point, and with any factor from 3 to 10
    the second attempt is clipped to that point and the third to the end, so the solve takes three attempts whatever the
    rounding of the first ratios; every ratio stays below 0.01, far from a rejection.  (Cases with a rejected attempt
    were tried: whether the attempt after a cautious first step is rejected depends on its length, i.e. on the factor
    above, and the fp32 solves - fused, host-stepped, and the float64 integrator over the fp32 field alike - then take
    one attempt fewer than float64.)"""
    key = (solver, B, down)
    if key not in _ADAPT_REF:
        Ws, bs = G.smooth_action_params(2, 64, seed=0, box=4.0, out_scale=300.0)
        x0 = np.random.default_rng(B).uniform(-1.0, 1.0, (B, 2)).astype(np.float32)
        ts = ADAPT_TS[::-1].copy() if down else ADAPT_TS
        zmax = [-np.inf]

        def f(t, y):                                                  # the field, watching the pre-activations it meets
            zmax[0] = max(zmax[0], max(float(z.max()) for z in G._forward(Ws, bs, t, y)[1]))
            return G.grad_field(Ws, bs, t, y)
        fs, tss = (R.reverse(f), -ts) if down else (f, ts)          # a decreasing grid: -f(-s, y) on s = -t_span
        ref, info = _adaptive_solve(solver, fs, x0, tss)
        # the conditions on the case: no decision near 1, every stage point where the net is smooth, the states move,
        # the attempts do not depend on fp32 rounding
        assert rk.ratios_clear_of_one(info["log"], 0.5, 2.0), (key, [l[2] for l in info["log"]])
        assert zmax[0] <= -0.05, zmax
        assert np.abs(ref[-1] - ref[0]).max() >= 0.05
        assert _counts_survive_fp32(solver, fs, x0, tss, info), key
        _ADAPT_REF[key] = (Ws, bs, ts, x0, ref, info)
    return _ADAPT_REF[key]


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("B", [40, 16 * 3 + 1])
@pytest.mark.parametrize("solver", ["dopri5", "tsit5"])
def test_adaptive_solves_on_a_smooth_action(dev, solver, B, down):
    Ws, bs, ts, x0, ref, info = _adaptive_ref(solver, B, down)
    node = _node(Ws, bs, solver, dev, tol=1e-5)
    tr = node.trajectory(torch.from_numpy(x0).to(dev), torch.from_numpy(ts))
    assert node.last_path == "hip"
    n_acc = sum(1 for l in info["log"] if l[3])
    print(f"{solver} B={B} down={down}: steps {node.n_steps} (oracle {info['steps']}, {n_acc} accepted), nfe {node.nfe}")
    assert (node.n_steps, node.nfe) == (info["steps"], info["nfe"])
    err = np.abs(tr.cpu().numpy() - ref).max() / np.abs(ref).max()
    print("max|x - x64| / max|x64| =", err)
    assert err <= 1e-5, err


# ------------------------------------------------------------------------------------------------------ 5: reverse time
@pytest.mark.parametrize("solver", ["euler", "midpoint", "rk4", "dopri5", "tsit5"])
def test_reverse_time_is_the_forward_solve_of_the_negated_action(dev, solver):
    Ws, bs = G.action_params(2, (64, 64, 64), seed=0, out_scale=8.0)
    Wn, bn = G.negated_action_params(Ws, bs)
    x0 = torch.from_numpy(_x(40, 2, 3)).to(dev)
    ts = torch.from_numpy(UNIFORM[::-1].copy())
    a, b = _node(Ws, bs, solver, dev, tol=1e-4), _node(Wn, bn, solver, dev, tol=1e-4)
    ta, tb = a.trajectory(x0, ts), b.trajectory(x0, -ts)
    assert a.last_path == b.last_path == "hip"
    assert (a.n_steps, a.nfe) == (b.n_steps, b.nfe) and a.nfe > 0
    assert torch.equal(ta, tb)


# ------------------------------------------------------------------------------------------------------ 6: augmented
@pytest.mark.parametrize("solver", ["euler", "rk4"])
def test_augmented_solve_exact_trace(dev, solver, monkeypatch):
    import cfm_amd
    from cfm_amd.models import GradModel
    from cfm_amd.ode import NeuralODE
    B, d = 40, 2
    Ws, bs = G.action_params(d, (64, 64, 64), seed=0, out_scale=8.0)
    ts = UNIFORM[::-1].copy()
    x0 = _x(B, d, 25)                                                  # (the x0 of FIXED_CASES: within the cap for rk4)
    aug0 = np.concatenate([np.zeros((B, 1), np.float32), x0], 1)
    watch = G.KinkWatch(Ws, bs, G.aug_field_np(Ws, bs), aug=True)
    ref = oracle.euler_trajectory(watch, aug0, ts) if solver == "euler" else rk.fixed_trajectory(watch, aug0, ts, solver)
    keep = _kept(watch.clear(), 0.15, f"augmented {solver}")
    node = _node(Ws, bs, solver, dev, cnf=True)
    tr = node.trajectory(torch.from_numpy(aug0).to(dev), torch.from_numpy(ts))
    assert node.last_path == "hip" and (node.n_steps, node.nfe) == (20, STAGES[solver] * 20)
    plain = _node(Ws, bs, solver, dev)
    tp = plain.trajectory(torch.from_numpy(x0).to(dev), torch.from_numpy(ts))
    assert torch.equal(tr[:, :, 1:], tp)                               # the x columns are the plain solve's
    ell, lref = tr[:, :, 0].cpu().numpy(), ref[:, :, 0]
    err = np.abs(ell - lref)[:, keep].max() / np.abs(lref[:, keep]).max()
    print(f"{solver}: max|l - l64| / max|l64| = {err:.3g}")
    assert err <= 1e-5, err
    # CNF.forward: the one-evaluation entry, [-lap, v]
    out = node.vf(torch.tensor(float(ts[0])), torch.from_numpy(aug0).to(dev))
    lib, a, hp = _hip(Ws, bs, dev)
    v, lap = _field(lib, hp, torch.from_numpy(x0).to(dev), d, B, d, float(ts[0]), True, dev)
    assert torch.equal(out[:, 1:], v) and torch.equal(out[:, 0], -lap)
    # log_likelihood runs through the same solve
    paths = []
    orig = NeuralODE.trajectory
    monkeypatch.setattr(NeuralODE, "trajectory", lambda self, x, t: (orig(self, x, t), paths.append(self.last_path))[0])
    gm = GradModel(G.make_action(Ws, bs, dev))
    ll = cfm_amd.cnf.log_likelihood(gm, torch.from_numpy(x0).to(dev), t_span=torch.from_numpy(ts), solver=solver)
    assert paths == ["hip"]
    want = cfm_amd.cnf.standard_normal_log_prob(tr[-1][:, 1:]) - tr[-1][:, 0]
    assert torch.equal(ll, want)


@pytest.mark.parametrize("estimator", ["hutch_gaussian", "hutch_rademacher"])
def test_hutchinson_on_a_gradient_field_keeps_its_path(dev, estimator):
    """Hutchinson estimators on a gradient field are not built: they take the generic path, as before.  That path
    evaluates the probe product with torch.func, which cannot transform the autograd.grad call inside GradModel.forward
    and raises a RuntimeError (DESIGN.md 4.10 records this)."""
    Ws, bs = G.action_params(2, (64, 64, 64), seed=0)
    node = _node(Ws, bs, "euler", dev, cnf=True, estimator=estimator)
    aug0 = torch.cat([torch.zeros(8, 1), torch.from_numpy(_x(8, 2, 1))], 1).to(dev)
    with pytest.raises(RuntimeError):
        node.trajectory(aug0, torch.tensor([1.0, 0.5, 0.0]))
    assert node.last_path == "generic"


def test_adaptive_augmented_solve_is_stepped_on_the_host(dev):
    """dopri5 on the augmented state of a gradient field has no fused driver: the generic path steps it on the host,
    every evaluation being CNF.forward's one launch of cfm_mlp_grad_field_f32.  On the smooth action (no kinks for the
    error estimate to see) it follows the float64 solve."""
    Ws, bs, ts, x0, _, _ = _adaptive_ref("dopri5", 40, True)
    aug0 = np.concatenate([np.zeros((40, 1), np.float32), x0], 1)
    F = R.reverse(G.aug_field_np(Ws, bs))
    ref, info = _adaptive_solve("dopri5", F, aug0, -ts)
    assert rk.ratios_clear_of_one(info["log"], 0.5, 2.0) and _counts_survive_fp32("dopri5", F, aug0, -ts, info)
    node = _node(Ws, bs, "dopri5", dev, tol=1e-5, cnf=True)
    tr = node.trajectory(torch.from_numpy(aug0).to(dev), torch.from_numpy(ts))
    assert node.last_path == "generic" and (node.n_steps, node.nfe) == (info["steps"], info["nfe"])
    err = np.abs(tr.cpu().numpy() - ref).max() / np.abs(ref).max()
    print("max|[l, x] - float64| / max|float64| =", err)
    assert err <= 1e-5, err


# ------------------------------------------------------------------------------------------------------ 7: many tiles
def test_more_tiles_than_workgroups(dev):
    """B = 16 * 4096 + 5: 4097 tiles on the 4096 workgroups of the grid cap, so workgroup 0 walks a second (partial) tile"""
    B, d = 16 * 4096 + 5, 2
    Ws, bs = G.action_params(d, (64, 64, 64), seed=0, out_scale=8.0)
    x0 = torch.from_numpy(_x(B, d, 11)).to(dev)
    ts = torch.tensor([0.0, 0.3, 0.7, 1.0])
    node = _node(Ws, bs, "euler", dev)
    tr = node.trajectory(x0, ts)
    assert node.last_path == "hip" and node.nfe == 3
    for lo, hi in ((0, 16), (16 * 2048, 16 * 2049), (16 * 4096, B), (B - 16, B)):   # first, a middle, the 4097th (= last) tile
        alone = node.trajectory(x0[lo:hi].contiguous(), ts)
        assert node.last_path == "hip"
        assert torch.equal(alone, tr[:, lo:hi]), (lo, hi)


# ------------------------------------------------------------------------------------------------------ 8: dispatch
def _generic_case(dev, Ws, bs, x0, dtype, node_kw=None):
    ts = np.linspace(0.0, 1.0, 6).astype(np.float32)
    watch = G.KinkWatch(Ws, bs, G.field_np(Ws, bs))
    ref = oracle.euler_trajectory(watch, x0, ts)
    keep = _kept(watch.clear(), 0.15, "generic euler")
    from cfm_amd.models import GradModel
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    node = NeuralODE(torch_wrapper(GradModel(G.make_action(Ws, bs, dev, dtype=dtype))), solver="euler")
    tr = node.trajectory(torch.from_numpy(x0).to(device=dev, dtype=dtype), torch.from_numpy(ts))
    err = np.abs(tr.cpu().numpy() - ref)[:, keep].max() / np.abs(ref[:, keep]).max()
    print("max|x - x64| / max|x64| =", err)
    assert err <= 1e-5, err
    return node


def test_dispatch_outside_the_envelope_is_generic(dev):
    from cfm_amd import _lib
    lib = _lib.load()
    x0 = _x(40, 2, 5)
    # an action net wider than 64
    Ww, bw = G.action_params(2, (128, 128, 128), seed=0, out_scale=8.0)
    assert _generic_case(dev, Ww, bw, x0, torch.float32).last_path == "generic"
    # a float64 input
    Ws, bs = G.action_params(2, (64, 64, 64), seed=0, out_scale=8.0)
    assert _generic_case(dev, Ws, bs, x0, torch.float64).last_path == "generic"
    # the fused path switched off: the entries decline, GradModel.forward goes through autograd
    assert _generic_case(dev, Ws, bs, x0, torch.float32).last_path == "hip"
    lib.cfm_ode_set_fused(0)
    try:
        assert _generic_case(dev, Ws, bs, x0, torch.float32).last_path == "generic"
        _, a, hp = _hip(Ws, bs, dev)
        xd = torch.from_numpy(x0).to(dev)
        v = torch.empty(40, 2, device=dev)
        assert lib.cfm_mlp_grad_field_f32(hp[0], hp[1], hp[2], 4, _lib.ptr(xd), 2, 40, 0.0, _lib.ptr(v), None, None,
                                          _lib.stream_ptr()) == -1
    finally:
        lib.cfm_ode_set_fused(1)
    assert _generic_case(dev, Ws, bs, x0, torch.float32).last_path == "hip"


def test_c_entries_refuse_what_is_outside_the_envelope(dev):
    from cfm_amd import _lib
    lib, a, hp = _hip(*G.action_params(2, (64, 64, 64), seed=0), dev)
    B, d = 16, 2
    xd = torch.zeros(B, 64, device=dev)
    aug = torch.zeros(B, 65, device=dev)
    v = torch.zeros(B, 64, device=dev)
    traj = torch.zeros(3, B, 65, device=dev)
    ws = _lib.workspace(_lib.OP_ODE, B, 64, 65, dev)
    ts = np.array([0.0, 0.5, 1.0], dtype=np.float32)
    tsp = ts.ctypes.data_as(ctypes.c_void_p)
    nfe, steps = ctypes.c_int(0), ctypes.c_int(0)
    ok = [3, 64, 64, 64, 1]
    bad = [[3, 64, 64, 64, 2], [65, 64, 64, 64, 1], [3, 65, 64, 64, 1], [3, 64, 64, 65, 1], [1, 64, 64, 64, 1], [3, 64, 0, 64, 1]]

    def calls(dims, n_layers=4, mode=0):
        cd = (ctypes.c_int * 5)(*dims)
        return [
            lib.cfm_mlp_grad_field_f32(hp[0], hp[1], cd, n_layers, _lib.ptr(xd), 64, B, 0.0, _lib.ptr(v), None, None, _lib.stream_ptr()),
            lib.cfm_ode_fixed_gradmlp_f32(hp[0], hp[1], cd, n_layers, _lib.ptr(xd), B, tsp, 3, 0, _lib.ptr(traj), ctypes.byref(nfe),
                                          _lib.ptr(ws), _lib.stream_ptr()),
            lib.cfm_ode_adaptive_gradmlp_f32(hp[0], hp[1], cd, n_layers, _lib.ptr(xd), B, tsp, 3, 0, 1e-4, 1e-4, _lib.ptr(traj),
                                             ctypes.byref(steps), ctypes.byref(nfe), _lib.ptr(ws), _lib.stream_ptr()),
            lib.cfm_ode_fixed_cnf_gradmlp_f32(hp[0], hp[1], cd, n_layers, _lib.ptr(aug), B, tsp, 3, mode, None, 0, _lib.ptr(traj),
                                              ctypes.byref(nfe), _lib.ptr(ws), _lib.stream_ptr()),
        ]
    for dims in bad:
        assert calls(dims) == [-1, -1, -1, -1], dims
    assert calls(ok, n_layers=3) == [-1, -1, -1, -1]
    assert calls(ok, mode=1)[3] == -1                                    # the exact trace only
    assert lib.cfm_ode_fixed_gradmlp_f32(hp[0], hp[1], hp[2], 4, _lib.ptr(xd), B, tsp, 3, 7, _lib.ptr(traj), ctypes.byref(nfe),
                                         _lib.ptr(ws), _lib.stream_ptr()) == -1       # an unknown scheme
    torch.cuda.synchronize()


def test_grad_enabled_calls_stay_differentiable(dev):
    """with grad enabled GradModel.forward is the reference's code: create_graph=True, so a second derivative exists"""
    from cfm_amd.models import GradModel
    Ws, bs = G.action_params(2, (64, 64, 64), seed=0)
    gm = GradModel(G.make_action(Ws, bs, dev))
    x = _x(64, 2, 9)
    keep = _kept(G.min_abs_preactivation(Ws, bs, 0.37, x) > 1e-5, 0.02, "second derivative")
    inp = torch.cat([torch.from_numpy(x), torch.full((64, 1), 0.37)], 1).to(dev)
    v = gm(inp)
    assert v.requires_grad and inp.requires_grad
    lap = sum(torch.autograd.grad(v[:, k].sum(), inp, retain_graph=True)[0][:, k] for k in range(2))
    vref, lref = G.grad_field(Ws, bs, 0.37, x, laplacian=True)
    assert np.abs(v.detach().cpu().numpy() - vref)[keep].max() <= 1e-5 * np.abs(vref[keep]).max()
    diag, mag = G.laplacian_terms(Ws, bs, 0.37, x)
    assert ((np.abs(lap.cpu().numpy() - lref) / (2e-5 * diag + 1e-6 * mag))[keep]).max() <= 1.0
