"""GPU (-m gpu): tsit5, midpoint and rk4 on the HIP drivers — against the float64 restatements of tests/ode_rk_ref.py
(fixtures: tests/golden/ode_solvers_cases.npz), fused kernel against layer-per-kernel path bit for bit, reverse time,
the augmented (CNF) solves, the wide-field layer driver and the selector entries of the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cfm_oracle as oracle
import cnf_restate as R
import ode_rk_ref as rk

pytestmark = pytest.mark.gpu

STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "ode_solvers_cases.npz"))
    for k in ("g", "c", "l"):           # the condition on the fixture: no accept can legitimately flip in fp32
        assert rk.ratios_clear_of_one(g[f"{k}_tsit5_log"]), k
    return g


def _seeded_mlp(d, w, seed):
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(d + 1, w), torch.nn.Linear(w, w), torch.nn.Linear(w, w), torch.nn.Linear(w, d)]
    return [l.weight.detach().numpy().copy() for l in lins], [l.bias.detach().numpy().copy() for l in lins]


def _node(Ws, bs, solver, tol, dev, cnf=False, **kw):
    import cfm_amd
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    m = R.make_mlp(Ws, bs, dev)
    vf = cfm_amd.CNF(m, **kw) if cnf else torch_wrapper(m)
    return NeuralODE(vf, solver=solver, atol=tol, rtol=tol)


def _aug0(x):
    return torch.cat([torch.zeros(x.shape[0], 1), x], 1)


def _close(tr, ref, what):
    err, scale = np.abs(tr - ref).max(), np.abs(ref).max()
    print(what, "max |diff| / max |ref| =", err / scale)
    assert err <= 1e-5 * scale, (what, err / scale)


# ---------------------------------------------------------------------------------------- against the restatement
def test_golden_mlp_vs_restatement(dev, cases, golden_dir):
    d = np.load(os.path.join(golden_dir, "ode_cases.npz"))
    Ws, bs = [d[f"W{k}"] for k in range(4)], [d[f"b{k}"] for k in range(4)]
    x, ts = torch.from_numpy(d["x"]), torch.from_numpy(d["t_span"])
    node = _node(Ws, bs, "tsit5", 1e-4, dev)
    tr = node.trajectory(x, ts).cpu().numpy()
    assert node.last_path == "hip"
    assert (node.n_steps, node.nfe) == (int(cases["g_tsit5_steps"]), int(cases["g_tsit5_nfe"])), (node.n_steps, node.nfe)
    _close(tr, cases["g_tsit5"], "tsit5")
    np.testing.assert_array_equal(tr[0], d["x"])
    for solver in ("midpoint", "rk4"):
        node = _node(Ws, bs, solver, 1e-4, dev)
        tr = node.trajectory(x, ts).cpu().numpy()
        assert node.last_path == "hip" and (node.n_steps, node.nfe) == (len(ts) - 1, STAGES[solver] * (len(ts) - 1))
        _close(tr, cases[f"g_{solver}"], solver)


@pytest.mark.parametrize("solver", ["tsit5", "midpoint", "rk4"])
def test_c5_shape_vs_restatement(dev, cases, solver):
    """B = 8192, 51-64-64-64-50, linspace(0, 1, 100), atol = rtol = 1e-4: the restatement is integrated here (the
    full trajectory is too large to record) and must reproduce the recorded log / last-frame rows."""
    Ws, bs = _seeded_mlp(50, 64, 0)
    x0, _ = oracle.config_inputs("C5")
    ts = torch.from_numpy(np.linspace(0, 1, 100).astype(np.float32))     # the generator's grid, to the bit
    f = lambda t, y: oracle.mlp_forward_f64(Ws, bs, y, t)
    node = _node(Ws, bs, solver, 1e-4, dev)
    tr = node.trajectory(x0, ts).cpu().numpy()
    assert node.last_path == "hip" and tr.shape == (100, 8192, 50)
    if solver == "tsit5":
        ref, info = rk.adaptive_trajectory(f, x0.numpy(), ts.numpy(), 1e-4, 1e-4, "tsit5", return_log=True)
        rk.assert_same_log(info["log"], cases["c_tsit5_log"])
        assert (info["steps"], info["nfe"]) == (int(cases["c_tsit5_steps"]), int(cases["c_tsit5_nfe"]))
        assert (node.n_steps, node.nfe) == (info["steps"], info["nfe"]), (node.n_steps, node.nfe, info["steps"], info["nfe"])
    else:
        ref = rk.fixed_trajectory(f, x0.numpy(), ts.numpy(), solver)
        assert (node.n_steps, node.nfe) == (99, STAGES[solver] * 99)
    assert np.abs(ref[-1, :256] - cases[f"c_{solver}_last"]).max() <= 1e-10 * np.abs(ref[-1]).max()
    _close(tr, ref, solver)


def test_wide_field_tsit5_vs_restatement(dev, cases):
    """d = 784, w = 512: the layer-per-kernel driver (weights regenerated from the seed, guarded by a checksum)."""
    Ws, bs = _seeded_mlp(784, 512, 5)
    assert abs(float(np.abs(Ws[0]).sum()) - float(cases["l_W0_checksum"])) <= 1e-6 * float(cases["l_W0_checksum"])
    g = torch.Generator().manual_seed(17)
    x = torch.randn(24, 784, generator=g)
    ts = torch.from_numpy(np.linspace(0, 1, 4).astype(np.float32))
    node = _node(Ws, bs, "tsit5", 1e-4, dev)
    tr = node.trajectory(x, ts).cpu().numpy()
    assert node.last_path == "hip"
    assert (node.n_steps, node.nfe) == (int(cases["l_tsit5_steps"]), int(cases["l_tsit5_nfe"])), (node.n_steps, node.nfe)
    _close(tr, cases["l_tsit5"].astype(np.float64), "wide tsit5")


# ---------------------------------------------------------------------------------------- fused == layer path
@pytest.mark.parametrize("B,d,w,n_t", [(300, 2, 64, 25), (257, 50, 64, 12), (64, 63, 33, 4), (8192, 50, 64, 6),
                                        (8231, 3, 48, 5), (20000, 2, 64, 4)])
def test_fused_small_field_equals_layer_path(dev, B, d, w, n_t):
    """The shapes of test_ode_fused_small_field_equals_layer_path (x / k1 resident in registers up to B = 8192, streamed
    above: the last two cases).  On the register-staged layer core (cfm_mlp_set_glds(0)) the fused kernels and the
    layer-per-kernel drivers run the same fp32 arithmetic in the same order: trajectories, nfe and n_steps are equal bit
    for bit, for tsit5, midpoint and rk4 (and still for euler through the generalised kernel)."""
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    lib = _lib.load()
    torch.manual_seed(3)
    model = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(9)).to(dev)
    ts = torch.linspace(0, 1, n_t, device=dev)
    out = {}
    glds0 = lib.cfm_mlp_get_glds()
    try:
        lib.cfm_mlp_set_glds(0)
        for fused in (1, 0):
            lib.cfm_ode_set_fused(fused)
            for solver in ("tsit5", "midpoint", "rk4", "euler"):
                node = NeuralODE(torch_wrapper(model), solver=solver, atol=1e-4, rtol=1e-4)
                out[(fused, solver)] = (node.trajectory(x, ts).cpu(), node.nfe, node.n_steps)
                assert node.last_path == "hip"
    finally:
        lib.cfm_ode_set_fused(1); lib.cfm_mlp_set_glds(glds0)
    for solver in ("tsit5", "midpoint", "rk4", "euler"):
        a, b = out[(1, solver)], out[(0, solver)]
        assert a[1] == b[1] and a[2] == b[2], (solver, a[1:], b[1:])
        assert torch.equal(a[0], b[0]), (solver, float((a[0] - b[0]).abs().max()))
        assert bool(torch.isfinite(a[0]).all())


# ---------------------------------------------------------------------------------------- non-square hidden layers
WMIX, WMIX2 = (64, 17, 40), (33, 64, 48)       # no two layers of a net share a shape: extents and strides cannot be exchanged
_WID = lambda w: "-".join(map(str, w))         # noqa: E731


@pytest.mark.parametrize("w", [WMIX, WMIX2], ids=_WID)
@pytest.mark.parametrize("B,d,n_t", [(300, 2, 25), (64, 63, 4)])
def test_fused_small_field_equals_layer_path_at_non_square_widths(dev, B, d, w, n_t):
    """test_fused_small_field_equals_layer_path with hidden layers [d + 1, *w, d] (sm_stage_weights pads each layer from
    its own in / out extents), for all five solvers: same bits as the layer-per-kernel path on the register-staged
    layer core, which takes every layer's K from that layer's own shape."""
    from cfm_amd import _lib
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    lib = _lib.load()
    model = R.make_mlp(*R.mlp_params(d, w, 3), dev)
    assert [l.out_features for l in model._linears()] == list(w) + [d]
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(9)).to(dev)
    ts = torch.linspace(0, 1, n_t, device=dev)
    solvers = ("dopri5", "tsit5", "midpoint", "rk4", "euler")
    out = {}
    glds0 = lib.cfm_mlp_get_glds()
    try:
        lib.cfm_mlp_set_glds(0)
        for fused in (1, 0):
            lib.cfm_ode_set_fused(fused)
            for solver in solvers:
                node = NeuralODE(torch_wrapper(model), solver=solver, atol=1e-4, rtol=1e-4)
                out[(fused, solver)] = (node.trajectory(x, ts).cpu(), node.nfe, node.n_steps)
                assert node.last_path == "hip"
    finally:
        lib.cfm_ode_set_fused(1); lib.cfm_mlp_set_glds(glds0)
    for solver in solvers:
        a, b = out[(1, solver)], out[(0, solver)]
        assert a[1] == b[1] and a[2] == b[2], (solver, a[1:], b[1:])
        assert torch.equal(a[0], b[0]), (solver, float((a[0] - b[0]).abs().max()))
        assert bool(torch.isfinite(a[0]).all())


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("d,w,B", [(5, WMIX, 77), (63, WMIX2, 33)], ids=lambda v: _WID(v) if isinstance(v, tuple) else str(v))
def test_non_square_widths_vs_restatement(dev, d, w, B, fused):
    """Two paths can agree on a wrong staging: rk4 on a non-uniform grid and an adaptive tsit5 solve against the float64
    restatement, on both paths, each to 1e-5 of max|x|.  tsit5: the same attempts as the restatement, whose ratios keep
    clear of 1 (asserted: every attempt of these two solves is accepted with a ratio below 0.06)."""
    from cfm_amd import _lib
    lib = _lib.load()
    Ws, bs = R.mlp_params(d, w, seed=13)
    f = R.mlp_field_np(Ws, bs)
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(5))
    ts = torch.tensor([0.0, 0.13, 0.5, 0.62, 1.0])
    lib.cfm_ode_set_fused(1 if fused else 0)
    try:
        fx = _node(Ws, bs, "rk4", 1e-4, dev)
        tf = fx.trajectory(x, ts).cpu().numpy()
        ad = _node(Ws, bs, "tsit5", 1e-4, dev)
        ta = ad.trajectory(x, ts).cpu().numpy()
    finally:
        lib.cfm_ode_set_fused(1)
    assert fx.last_path == "hip" and ad.last_path == "hip"
    assert (fx.n_steps, fx.nfe) == (4, 16) and tf.shape == (5, B, d)
    _close(tf, rk.fixed_trajectory(f, x.numpy(), ts.numpy(), "rk4"), f"rk4 {_WID(w)} fused={fused}")
    ref, info = rk.adaptive_trajectory(f, x.numpy(), ts.numpy(), 1e-4, 1e-4, "tsit5", return_log=True)
    assert rk.ratios_clear_of_one(info["log"])
    assert all(accept and ratio < 0.06 for _, _, ratio, accept in info["log"]), info["log"]
    assert (ad.n_steps, ad.nfe) == (info["steps"], info["nfe"]), (ad.n_steps, ad.nfe, info["steps"], info["nfe"])
    _close(ta, ref, f"tsit5 {_WID(w)} fused={fused}")


# ---------------------------------------------------------------------------------------- reverse time
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("d,w", [(2, 64), (5, 32)])
def test_reverse_tsit5_is_the_negated_mlp_forward_solve(dev, d, w, fused):
    from cfm_amd import _lib
    lib = _lib.load()
    Ws, bs = R.mlp_params(d, w, seed=7 + d)
    Wn, bn = R.negated_mlp_params(Ws, bs)
    torch.manual_seed(3)
    x = torch.randn(300, d)
    ts = torch.tensor([1.0, 0.7, 0.25, 0.0])
    lib.cfm_ode_set_fused(1 if fused else 0)
    try:
        a = _node(Ws, bs, "tsit5", 1e-5, dev)
        ta = a.trajectory(x, ts).cpu()
        b = _node(Wn, bn, "tsit5", 1e-5, dev)
        tb = b.trajectory(x, -ts).cpu()
        fixed = {}
        for solver in ("midpoint", "rk4"):
            fixed[solver] = (_node(Ws, bs, solver, 1e-5, dev).trajectory(x, ts).cpu(),
                             _node(Wn, bn, solver, 1e-5, dev).trajectory(x, -ts).cpu())
    finally:
        lib.cfm_ode_set_fused(1)
    assert a.last_path == "hip" and ta.shape == (4, 300, d)
    assert torch.equal(ta, tb) and (a.n_steps, a.nfe) == (b.n_steps, b.nfe)
    # The controller is free here (8 attempts for 3 intervals, one rejected at d = 2): same attempts as the restatement,
    # whose log keeps clear of 1.  The step sizes come from an error estimate that is a cancellation, so fp32 and float64
    # stage values give slightly different dt, and two solves with different dt differ by their integration errors:
    # the bound is the parity bar plus the restatement's own distance from a converged solve (the form of the bound on l
    # in tests/test_gpu_cnf.py).
    G = R.reverse(R.mlp_field_np(Ws, bs))
    ref, info = rk.adaptive_trajectory(G, x.numpy(), -ts.numpy(), 1e-5, 1e-5, "tsit5", return_log=True)
    assert rk.ratios_clear_of_one(info["log"])
    assert (a.n_steps, a.nfe) == (info["steps"], info["nfe"]), (a.n_steps, a.nfe, info["steps"], info["nfe"])
    own = np.abs(ref - rk.adaptive_trajectory(G, x.numpy(), -ts.numpy(), 1e-10, 1e-10, "tsit5")).max()
    err = np.abs(ta.numpy() - ref).max()
    print("reverse tsit5: |diff| / max|ref| =", err / np.abs(ref).max(), "restatement's own error:", own / np.abs(ref).max())
    assert err <= 1e-5 * np.abs(ref).max() + own
    for solver, (fa, fb) in fixed.items():          # dt < 0 steps backward: the same numbers
        assert torch.equal(fa, fb), solver
        _close(fa.numpy(), rk.fixed_trajectory(R.mlp_field_np(Ws, bs), x.numpy(), ts.numpy(), solver), "reverse " + solver)


# ---------------------------------------------------------------------------------------- CNF
@pytest.mark.parametrize("estimator", ["exact", "hutch_rademacher"])
@pytest.mark.parametrize("solver", ["tsit5", "rk4"])
@pytest.mark.parametrize("d,w,B", [(2, 64, 700), (3, 64, 9000)])
def test_log_likelihood_on_the_hip_path_vs_generic(dev, monkeypatch, solver, estimator, d, w, B):
    """log_likelihood(solver=...) runs in the augmented HIP drivers and agrees with the torch.func generic path under
    the same solver within the CNF tests' tolerance (test_augmented_dopri5_smooth_field_l_to_1e5: x and l to 1e-5, on a
    field whose SELUs stay on their smooth branch).  B = 9000: the streamed form of the adaptive kernel."""
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd.ode import NeuralODE
    lib = _lib.load()
    Ws, bs = R.smooth_mlp_params(d, w, seed=90 + d + w)
    m = R.make_mlp(Ws, bs, dev)
    torch.manual_seed(9)
    x = 0.5 * torch.randn(B, d)
    eps = torch.randint(0, 2, (B, d)).float() * 2 - 1 if estimator != "exact" else None
    ts = torch.linspace(1, 0, 9) if solver == "rk4" else torch.tensor([1.0, 0.0])
    paths = []
    orig = NeuralODE.trajectory

    def spy(self, *a, **k):
        out = orig(self, *a, **k)
        paths.append((self.solver, self.last_path, self.nfe, self.n_steps))
        return out
    monkeypatch.setattr(NeuralODE, "trajectory", spy)
    lp, z = cfm_amd.log_likelihood(m, x.to(dev), t_span=ts, solver=solver, atol=1e-5, rtol=1e-5, estimator=estimator,
                                   noise=eps, return_z=True)
    assert paths[-1][:2] == (solver, "hip"), paths
    if solver == "rk4":
        assert paths[-1][2:] == (4 * 8, 8)
    else:
        assert paths[-1][2] == 2 + 6 * paths[-1][3]
    node = _node(Ws, bs, solver, 1e-5, dev, cnf=True, estimator=estimator, noise=eps)
    tr = node.trajectory(_aug0(x), ts).cpu()
    assert node.last_path == "hip"
    assert torch.equal(tr[-1][:, 1:], z.cpu())
    last = tr[-1].to(dev)                                       # (the prior's sum where log_likelihood takes it)
    assert torch.equal(cfm_amd.cnf.standard_normal_log_prob(last[:, 1:]) - last[:, 0], lp)
    assert float(tr[..., 1:].abs().max()) < 3.0                 # inside the box where every pre-activation is < 0
    lib.cfm_ode_set_fused(0)
    try:
        gen = _node(Ws, bs, solver, 1e-5, dev, cnf=True, estimator=estimator, noise=eps)
        g = gen.trajectory(_aug0(x), ts).cpu()
    finally:
        lib.cfm_ode_set_fused(1)
    assert gen.last_path == "generic"
    tr, g = tr.numpy(), g.numpy()
    sl = np.abs(tr[..., 0]).max()
    ex, el = np.abs(g[..., 1:] - tr[..., 1:]).max() / np.abs(tr[..., 1:]).max(), np.abs(g[..., 0] - tr[..., 0]).max() / sl
    print(solver, estimator, B, "x:", ex, "l:", el, "steps hip / generic:", node.n_steps, gen.n_steps)
    assert sl > 1e-3 and ex <= 1e-5 and el <= 1e-5, (ex, el)


# ---------------------------------------------------------------------------------------- C ABI
def _abi_args(dev, B=64, d=2, w=64, n_t=5):
    import cfm_amd
    from cfm_amd import _lib
    torch.manual_seed(1)
    m = cfm_amd.MLP(dim=d, time_varying=True, w=w).to(dev)
    Wp, bp, dims, keep = m.hip_params(dev)
    x = torch.randn(B, d, device=dev)
    ts = np.linspace(0, 1, n_t).astype(np.float32)
    ws = _lib.workspace(_lib.OP_ODE, B, w, d + 1, dev)
    return m, Wp, bp, dims, keep, x, ts, ws


def test_abi_unknown_selector_is_einval(dev):
    from cfm_amd import _lib
    from cfm_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    m, Wp, bp, dims, keep, x, ts, ws = _abi_args(dev)
    B, d = x.shape
    tsp = ts.ctypes.data_as(ctypes.c_void_p)
    traj = torch.zeros((len(ts), B, d + 1), device=dev)
    xa = torch.cat([torch.zeros(B, 1, device=dev), x], 1).contiguous()
    nfe, steps = ctypes.c_int(0), ctypes.c_int(0)
    for bad in (-1, 2, 7):
        assert lib.cfm_ode_adaptive_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, len(ts), bad, 1e-4, 1e-4, ptr(traj),
                                            ctypes.byref(steps), ctypes.byref(nfe), ptr(ws), stream_ptr()) == -1
        assert lib.cfm_ode_adaptive_cnf_mlp_f32(Wp, bp, dims, 4, ptr(xa), B, tsp, len(ts), 0, None, bad, 1e-4, 1e-4,
                                                ptr(traj), ctypes.byref(steps), ctypes.byref(nfe), ptr(ws),
                                                stream_ptr()) == -1
    for bad in (-1, 3, 9):
        assert lib.cfm_ode_fixed_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, len(ts), bad, ptr(traj), ctypes.byref(nfe),
                                         ptr(ws), stream_ptr()) == -1
        assert lib.cfm_ode_fixed_cnf_mlp_f32(Wp, bp, dims, 4, ptr(xa), B, tsp, len(ts), 0, None, bad, ptr(traj),
                                             ctypes.byref(nfe), ptr(ws), stream_ptr()) == -1
    torch.cuda.synchronize()
    assert float(traj.abs().max()) == 0.0                       # refused before anything was written


EDGE_SENTINEL = 7.5
EDGE_WIDTH = {"plain": 2, "pair": 2, "cnf": 3, "gradmlp": 2, "cnf_gradmlp": 3, "reg": 4}     # state columns at d = 2
EDGE_GRID = np.array([0.0, 0.3, 0.55, 1.0], np.float32)
NON_MONOTONE = (np.array([0.0, 0.5, 0.25, 1.0], np.float32), np.array([0.0, 0.5, 0.5, 1.0], np.float32))


@pytest.mark.parametrize("edge,B", [("one_point", 1), ("one_point", 17), ("non_monotone", 1), ("non_monotone", 17),
                                    ("few_elements", 1), ("recording_off_path", 1), ("recording_off_path", 17)])
def test_abi_entry_edges(dev, edge, B):
    """What the solver entries answer at the edges of their arguments (include/cfm_gfx950.h), d = 2, hidden width 64.
    one_point: n_t = 1 is a solve without a step: traj[0] = x0, nfe = 0, nothing else written.
    non_monotone: the plain and the pair fixed-step entries step any grid (dt <= 0 included) on both paths, within this
    file's float64 bound; the fixed-step entries that have the one launch only and every adaptive entry refuse it.
    few_elements: B d = 2 < n_t = 4 sends the plain entries down the layer path (same bound); the adaptive CNF entry
    refuses B (d + 1) < n_t and the fixed one n_t > 3 B (d + 1), both before anything is written.
    recording_off_path: the recording entry declines off the one-launch kernel with n_accepted = 0 and traj untouched."""
    import cfm_amd
    from cfm_amd import _lib
    from cfm_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    d, w, tol = 2, 64, 1e-4
    Ws, bs = R.mlp_params(d, w, seed=31)
    Wb, bb = R.mlp_params(d, w, seed=32)
    Wp, bp, dims, keep = R.make_mlp(Ws, bs, dev).hip_params(dev)
    Wq, bq, _, keep_b = R.make_mlp(Wb, bb, dev).hip_params(dev)
    torch.manual_seed(33)
    Wa, ba, adims, keep_a = cfm_amd.MLP(dim=d, out_dim=1, time_varying=True, w=w).to(dev).hip_params(dev)
    ws = _lib.workspace(_lib.OP_ODE, B, w, d + 2, dev)
    f, fb = R.mlp_field_np(Ws, bs), R.mlp_field_np(Wb, bb)
    field = {"plain": f, "pair": lambda t, y: 0.5 * (f(t, y) - fb(t, y))}
    x0 = {k: torch.randn(B, D, generator=torch.Generator().manual_seed(34)).to(dev) for k, D in EDGE_WIDTH.items()}
    max_steps = 64
    log, ysteps = torch.zeros((max_steps, 4), device=dev), torch.zeros((max_steps, B, d), device=dev)

    def fixed(name, scheme, ts, traj, nfe, ws=ws):
        head = (ptr(x0[name]), B, ts.ctypes.data_as(ctypes.c_void_p), len(ts))
        tail = (ptr(traj), ctypes.byref(nfe), ptr(ws), stream_ptr())
        if name == "plain":
            return lib.cfm_ode_fixed_mlp_f32(Wp, bp, dims, 4, *head, scheme, *tail)
        if name == "pair":
            return lib.cfm_ode_fixed_pair_mlp_f32(Wp, bp, Wq, bq, dims, 4, *head, scheme, *tail)
        if name == "cnf":
            return lib.cfm_ode_fixed_cnf_mlp_f32(Wp, bp, dims, 4, *head, 0, None, scheme, *tail)
        if name == "gradmlp":
            return lib.cfm_ode_fixed_gradmlp_f32(Wa, ba, adims, 4, *head, scheme, *tail)
        if name == "cnf_gradmlp":
            return lib.cfm_ode_fixed_cnf_gradmlp_f32(Wa, ba, adims, 4, *head, 0, None, scheme, *tail)
        assert name == "reg" and scheme == 0                    # Euler, exact trace, the squared_L2 column
        return lib.cfm_ode_euler_cnf_reg_mlp_f32(Wp, bp, dims, 4, *head, 0, None, 1, ptr(traj), None, ctypes.byref(nfe), ptr(ws),
                                                 stream_ptr())

    def adaptive(name, tab, ts, traj, nfe, steps, nacc=None, net=(Wp, bp, dims), ws=ws):
        head = (4, ptr(x0["cnf" if name == "cnf" else "plain"]), B, ts.ctypes.data_as(ctypes.c_void_p), len(ts))
        tail = (tol, tol, ptr(traj), ctypes.byref(steps), ctypes.byref(nfe))
        if name == "plain":
            return lib.cfm_ode_adaptive_mlp_f32(*net, *head, tab, *tail, ptr(ws), stream_ptr())
        if name == "rec":
            return lib.cfm_ode_adaptive_rec_mlp_f32(*net, *head, tab, *tail, max_steps, ptr(log), ptr(ysteps), ctypes.byref(nacc),
                                                    ptr(ws), stream_ptr())
        if name == "cnf":
            return lib.cfm_ode_adaptive_cnf_mlp_f32(*net, *head, 0, None, tab, *tail, ptr(ws), stream_ptr())
        assert name == "gradmlp"
        return lib.cfm_ode_adaptive_gradmlp_f32(Wa, ba, adims, *head, tab, *tail, ptr(ws), stream_ptr())

    schemes = lambda name: (0,) if name == "reg" else (0, 1, 2)     # noqa: E731
    solver_of = {v: k for k, v in _lib.ODE_SCHEME.items()}
    nfe, steps, nacc = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-5)

    if edge == "one_point":
        for name, D in EDGE_WIDTH.items():
            for scheme in schemes(name):
                traj = torch.full((2, B, D), EDGE_SENTINEL, device=dev)
                nfe.value = -7
                assert fixed(name, scheme, np.array([0.3], np.float32), traj, nfe) == 0, (name, scheme)
                torch.cuda.synchronize()
                assert nfe.value == 0, (name, scheme, nfe.value)
                assert torch.equal(traj[0], x0[name]) and bool((traj[1] == EDGE_SENTINEL).all()), (name, scheme)

    elif edge == "non_monotone":
        zeros = torch.zeros((4, B, d + 2), device=dev)
        for ts in NON_MONOTONE:
            for name in ("cnf", "gradmlp", "cnf_gradmlp", "reg"):
                for scheme in schemes(name):
                    assert fixed(name, scheme, ts, zeros, nfe) == -1, (name, scheme, ts)
            for name in ("plain", "rec", "cnf", "gradmlp"):
                for tab in (0, 1):
                    assert adaptive(name, tab, ts, zeros, nfe, steps, nacc) == -1, (name, tab, ts)
            ref = {(name, s): rk.fixed_trajectory(field[name], x0[name].cpu().numpy(), ts, solver_of[s])
                   for name in ("plain", "pair") for s in (0, 1, 2)}
            try:
                for fused in (1, 0):
                    lib.cfm_ode_set_fused(fused)
                    for (name, scheme), want in ref.items():
                        traj = torch.zeros((4, B, d), device=dev)
                        assert fixed(name, scheme, ts, traj, nfe) == 0, (name, scheme, ts, fused)
                        torch.cuda.synchronize()
                        assert nfe.value == 3 * STAGES[solver_of[scheme]]
                        _close(traj.cpu().numpy(), want, f"{name} {solver_of[scheme]} on {ts} fused={fused}")
            finally:
                lib.cfm_ode_set_fused(1)
        torch.cuda.synchronize()
        assert float(zeros.abs().max()) == 0.0                  # refused before anything was written

    elif edge == "few_elements":
        assert B * d < len(EDGE_GRID)
        x = x0["plain"].cpu().numpy()
        for scheme in (0, 1, 2):
            traj = torch.zeros((4, B, d), device=dev)
            assert fixed("plain", scheme, EDGE_GRID, traj, nfe) == 0
            torch.cuda.synchronize()
            assert nfe.value == 3 * STAGES[solver_of[scheme]]
            _close(traj.cpu().numpy(), rk.fixed_trajectory(f, x, EDGE_GRID, solver_of[scheme]), f"B d < n_t {solver_of[scheme]}")
        for solver, tab in _lib.ODE_TABLEAU.items():
            want, info = rk.adaptive_trajectory(f, x, EDGE_GRID, tol, tol, solver, return_log=True)
            assert rk.ratios_clear_of_one(info["log"]) and all(l[3] and l[2] < 0.06 for l in info["log"]), info["log"]
            traj = torch.zeros((4, B, d), device=dev)
            assert adaptive("plain", tab, EDGE_GRID, traj, nfe, steps) == 0
            torch.cuda.synchronize()
            assert (steps.value, nfe.value) == (info["steps"], info["nfe"]), (solver, steps.value, nfe.value, info)
            _close(traj.cpu().numpy(), want, f"B d < n_t {solver}")
        kept = torch.full((10, B, d + 1), EDGE_SENTINEL, device=dev)
        for tab in (0, 1):
            assert B * (d + 1) < len(EDGE_GRID) and adaptive("cnf", tab, EDGE_GRID, kept, nfe, steps) == -1
        long_grid = np.linspace(0, 1, 3 * B * (d + 1) + 1).astype(np.float32)
        for scheme in (0, 1, 2):
            assert fixed("cnf", scheme, long_grid, kept, nfe) == -1
        torch.cuda.synchronize()
        assert bool((kept == EDGE_SENTINEL).all())

    else:
        ts = np.array([0.0, 1.0], np.float32)                   # B d >= n_t: only the path decides
        kept = torch.full((2, B, d), EDGE_SENTINEL, device=dev)
        wide = R.make_mlp(*R.mlp_params(d, 65, seed=31), dev).hip_params(dev)
        for tab in (0, 1):
            nacc.value = -5
            assert adaptive("rec", tab, ts, kept, nfe, steps, nacc, net=wide[:3], ws=_lib.workspace(_lib.OP_ODE, B, 65, d, dev)) == -1
            assert nacc.value == 0
            nacc.value = -5
            lib.cfm_ode_set_fused(0)
            try:
                assert adaptive("rec", tab, ts, kept, nfe, steps, nacc) == -1
            finally:
                lib.cfm_ode_set_fused(1)
            assert nacc.value == 0
            torch.cuda.synchronize()
            assert bool((kept == EDGE_SENTINEL).all())
            took = torch.zeros((2, B, d), device=dev)           # the same arguments on the one-launch path are a solve
            assert adaptive("rec", tab, ts, took, nfe, steps, nacc) == 0 and 1 <= nacc.value <= steps.value
            torch.cuda.synchronize()
            assert torch.equal(took[0], x0["plain"])


def test_abi_old_entries_are_the_new_ones_at_dopri5_and_euler(dev):
    from cfm_amd import _lib
    from cfm_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    assert _lib.ODE_TABLEAU == {"dopri5": 0, "tsit5": 1} and _lib.ODE_SCHEME == {"euler": 0, "midpoint": 1, "rk4": 2}
    m, Wp, bp, dims, keep, x, ts, ws = _abi_args(dev, B=500, d=5, w=48, n_t=6)
    B, d = x.shape
    tsp = ts.ctypes.data_as(ctypes.c_void_p)
    a, b = torch.zeros((len(ts), B, d), device=dev), torch.zeros((len(ts), B, d), device=dev)
    na, nb, sa, sb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.cfm_ode_dopri5_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, len(ts), 1e-5, 1e-5, ptr(a), ctypes.byref(sa),
                                      ctypes.byref(na), ptr(ws), stream_ptr()) == 0
    assert lib.cfm_ode_adaptive_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, len(ts), 0, 1e-5, 1e-5, ptr(b), ctypes.byref(sb),
                                        ctypes.byref(nb), ptr(ws), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and (sa.value, na.value) == (sb.value, nb.value) and na.value == 2 + 6 * sa.value
    assert lib.cfm_ode_euler_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, len(ts), ptr(a), ctypes.byref(na), ptr(ws),
                                     stream_ptr()) == 0
    assert lib.cfm_ode_fixed_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, len(ts), 0, ptr(b), ctypes.byref(nb), ptr(ws),
                                     stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and na.value == nb.value == len(ts) - 1
    # the augmented pair
    xa = torch.cat([torch.zeros(B, 1, device=dev), x], 1).contiguous()
    a, b = torch.zeros((len(ts), B, d + 1), device=dev), torch.zeros((len(ts), B, d + 1), device=dev)
    assert lib.cfm_ode_dopri5_cnf_mlp_f32(Wp, bp, dims, 4, ptr(xa), B, tsp, len(ts), 0, None, 1e-5, 1e-5, ptr(a),
                                          ctypes.byref(sa), ctypes.byref(na), ptr(ws), stream_ptr()) == 0
    assert lib.cfm_ode_adaptive_cnf_mlp_f32(Wp, bp, dims, 4, ptr(xa), B, tsp, len(ts), 0, None, 0, 1e-5, 1e-5, ptr(b),
                                            ctypes.byref(sb), ctypes.byref(nb), ptr(ws), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and (sa.value, na.value) == (sb.value, nb.value)
    assert lib.cfm_ode_euler_cnf_mlp_f32(Wp, bp, dims, 4, ptr(xa), B, tsp, len(ts), 0, None, ptr(a), ctypes.byref(na),
                                         ptr(ws), stream_ptr()) == 0
    assert lib.cfm_ode_fixed_cnf_mlp_f32(Wp, bp, dims, 4, ptr(xa), B, tsp, len(ts), 0, None, 0, ptr(b), ctypes.byref(nb),
                                         ptr(ws), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and na.value == nb.value == len(ts) - 1


# ---------------------------------------------------------------------------------------- the second grid pass
BIG = 16 * 4096 + 5
PASS2_ROWS = (slice(0, 16), slice(16 * 2051, 16 * 2052), slice(BIG - 21, BIG))


@pytest.mark.parametrize("solver", ["euler", "midpoint", "rk4"])
def test_second_grid_pass_of_the_fused_fixed_step_sampler(dev, solver):
    """B = 16 * 4096 + 5, d = 2, hidden widths (33, 16, 24), three output times on a non-uniform grid (a fixed-step solve
    steps exactly its t_span: there is no refined step): ode_small_fixed<*, AUG_NONE, FIELD_MLP> is launched on at most
    4096 workgroups, so workgroup 0 runs tile 4096 after tile 0 on the same LDS tile buffers.  Rows of a tile do not
    interact: the first tile, a middle one and the last full tile with the 5-row tail are bit-equal to the same rows
    solved alone, and the tail is within this file's 1e-5 of the float64 restatement."""
    from cfm_amd import _lib
    _lib.load().cfm_ode_set_fused(1)
    Ws, bs = R.mlp_params(2, (33, 16, 24), seed=21)
    x = torch.randn(BIG, 2, generator=torch.Generator().manual_seed(22))
    ts = torch.tensor([0.0, 0.25, 0.5, 1.0])
    node = _node(Ws, bs, solver, 1e-4, dev)
    big = node.trajectory(x, ts).cpu()
    assert node.last_path == "hip" and big.shape == (4, BIG, 2) and (node.n_steps, node.nfe) == (3, 3 * STAGES[solver])
    assert bool(torch.isfinite(big).all())
    for rows in PASS2_ROWS:
        alone = node.trajectory(x[rows].contiguous(), ts).cpu()
        assert node.last_path == "hip"
        assert torch.equal(big[:, rows], alone), (solver, rows, float((big[:, rows] - alone).abs().max()))
    tail = PASS2_ROWS[-1]
    ref = rk.fixed_trajectory(R.mlp_field_np(Ws, bs), x[tail].numpy(), ts.numpy(), solver)
    _close(big[:, tail].numpy(), ref, f"{solver} B={BIG} tail tile")
