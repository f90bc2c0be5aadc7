"""GPU: the augmented sampler (AugmentationModule's L1, L2 and squared_L2 path integrals in FlowSolver.odeint) and the L1 /
L2 penalties of RegularizedCNF, on the widened `mode` and `reg_mask` of cfm_ode_euler_cnf_reg_mlp_f32 and
cfm_cnf_reg_euler_grad_f32, against the float64 restatement of tests/augment_restate.py.

Conventions of test_gpu_cnf_train.py: cr.mlp_params, the two grids (`down` uniform, `up` non-uniform), BOUND = 1e-5 as
max|a - b| / max|b| per column or per gradient tensor, a random upstream G of mean 0.5 on all columns, seed 1.

Forward: the integrands are >= 0 and the grids monotone, so no column is a cancelled sum and no row is dropped.
Gradient: rows within 1e-5 of a kink along the float64 trajectory are dropped before anything runs (a SELU kink; |v_j|
< 1e-5 with L1; |v| < 1e-5 with L2; ||J||_F / d < 1e-5 with jacobian_frobenius): B + B // 16 + 2 rows are drawn, at most
B / 4 may go, the first B are kept.  On seed 1 the float64 restatement alone drops at most 3 rows in any case below
(checked on the CPU when the test was written; the cap is asserted).

The forward kernel runs one workgroup per 16-row tile up to 4096 of them, so STRIDE's 4101 rows take a second pass in
the gradient kernel only (256 workgroups); FWD_STRIDE puts the forward kernel on its own second pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cfm_amd
import augment_restate as ar
import cnf_restate as cr
from cfm_amd import _lib
from cfm_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

BOUND = 1e-5
CG_MAXGRID = 256
W64, WMIX, WMIX2 = (64, 64, 64), (64, 17, 40), (33, 64, 48)
# (d, hidden widths, B, steps)
SHAPES = [(2, W64, 48, 8), (5, WMIX2, 19, 5), (1, (16, 16, 16), 33, 3), (63, W64, 17, 3), (2, W64, 1, 4),
          (2, W64, 16 * CG_MAXGRID + 5, 4)]           # the last: STRIDE[0] of test_gpu_cnf_train.py
FWD_STRIDE = (2, WMIX, 16 * 4096 + 5, 2)              # more tiles than the forward kernel's 4096 workgroups
NAMES = ["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dx"]
COEFF = {1: ("squared_l2_reg", 0.3), 2: ("jacobian_frobenius_reg", 0.7), 4: ("l1_reg", 0.2), 8: ("l2_reg", 0.4)}
EINVAL = -1


def _sid(s):
    return "d%d_w%s_B%d_n%d" % (s[0], "-".join(map(str, s[1])), s[2], s[3])


def _grid(direction, steps):
    if direction == "down":
        return np.linspace(1.0, 0.0, steps + 1).astype(np.float32)
    w = 1.0 + 0.6 * np.sin(1.7 * np.arange(steps) + 0.3)
    return np.concatenate([[0.0], np.cumsum(w) / w.sum()]).astype(np.float32)


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def _c_solve(m, state0, ts, mode, mask, eps=None):
    """(rc, traj [n_t, B, D]) of one call of the C entry on a device state [B, D]; traj is NaN-filled before the call."""
    lib = _lib.load()
    dev = state0.device
    Wp, bp, dims, keep = m.hip_params(dev)
    B, D = state0.shape
    tsn = np.ascontiguousarray(ts, np.float32)
    traj = torch.full((len(tsn), B, D), float("nan"), dtype=torch.float32, device=dev)
    jsq = torch.empty((max(len(tsn) - 1, 1), B), dtype=torch.float32, device=dev) if mask & 2 else None
    ws = _lib.workspace(_lib.OP_ODE, B, max(dims[1:4]), D, dev)
    nfe = ctypes.c_int(0)
    rc = lib.cfm_ode_euler_cnf_reg_mlp_f32(Wp, bp, dims, 4, ptr(state0), B, tsn.ctypes.data_as(ctypes.c_void_p), len(tsn), mode,
                                           ptr(eps), mask, ptr(traj), ptr(jsq), ctypes.byref(nfe), ptr(ws), stream_ptr())
    torch.cuda.synchronize()
    return rc, traj


# ---- forward, no trace -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_case(shape, direction):
    """Inputs and the float64 trajectory with all three |v| columns [L1, L2, e, y], computed once per (shape, grid)."""
    d, w, B, steps = shape
    Ws, bs = cr.mlp_params(d, w, 1)
    x0 = np.random.default_rng(1).normal(size=(B, d)).astype(np.float32)
    ts = _grid(direction, steps)
    want = ar.trajectory64(Ws, bs, x0, ts, 2, 13)
    for a in (x0, ts, want, *Ws, *bs):
        a.setflags(write=False)
    return Ws, bs, x0, ts, want


def _check_no_trace(shape, mask, direction):
    from cfm_amd.ode import NeuralODE
    from cfm_amd.utils import torch_wrapper
    dev = torch.device("cuda")
    Ws, bs, x0, ts, want = _fwd_case(shape, direction)
    d = shape[0]
    m = cr.make_mlp(Ws, bs, device=dev)
    x = torch.tensor(x0, device=dev)
    a = ar.n_aug(2, mask)
    rc, traj = _c_solve(m, torch.cat([torch.zeros(len(x0), a, device=dev), x], 1), ts, 2, mask)
    assert rc == 0
    node = NeuralODE(torch_wrapper(m), solver="euler")
    # cfm_ode_fixed_mlp_f32 runs its one-launch form only while t_span fits one state buffer (B d >= n_t) and its
    # layer-per-kernel form otherwise, whose bits are its own (measured at B = 1, d = 2, n_t = 5: the two differ in the last
    # place).  The kernel under test has one form.  Rows are independent, so where B d < n_t the rows are repeated until the
    # plain entry takes its one-launch form, and the first B rows are the reference: still bit for bit.
    reps = -(-len(ts) // (len(x0) * d))
    plain = node.trajectory(x.repeat(reps, 1), torch.tensor(ts))[:, :len(x0)]
    assert node.last_path == "hip"
    assert torch.equal(traj[:, :, a:], plain)
    if reps > 1:
        alone = node.trajectory(x, torch.tensor(ts))
        assert _rel(traj[:, :, a:].cpu().double().numpy(), alone.cpu().double().numpy()) <= BOUND
    got = traj.cpu().double().numpy()
    assert np.all(np.isfinite(got))
    ref_col = {"L1": 0, "L2": 1, "squared_L2": 2}
    for k, n in enumerate(ar.columns(2, mask)):
        err = _rel(got[:, :, k], want[:, :, ref_col[n]])
        print(f"{_sid(shape)} mask {mask} {direction}: {n} {err:.2e}")
        assert err <= BOUND, (n, err)
        assert not got[0, :, k].any()


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("mask", [4, 8, 1, 12, 13])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_no_trace_forward(shape, mask, direction):
    _check_no_trace(shape, mask, direction)


def test_no_trace_forward_on_the_forward_kernel_s_grid_stride():
    assert -(-FWD_STRIDE[2] // 16) > 4096 and FWD_STRIDE[2] % 16 != 0
    _check_no_trace(FWD_STRIDE, 13, "down")


# ---- forward, a trace with bits 2 and 3 ------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("mode,mask", [(0, 4), (0, 12), (0, 5), (0, 15), (1, 4), (1, 13)])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=_sid)
def test_trace_forward_keeps_the_bits_of_the_other_columns(shape, mode, mask, direction):
    from cfm_amd.ode import NeuralODE
    dev = torch.device("cuda")
    d, w, B, steps = shape
    Ws, bs = cr.mlp_params(d, w, 1)
    g = np.random.default_rng(1)
    a = ar.n_aug(mode, mask)
    s0 = np.concatenate([g.normal(size=(B, a)) * 0.1, g.normal(size=(B, d))], 1).astype(np.float32)
    eps = g.normal(size=(B, d)).astype(np.float32) if mode == 1 else None
    ts = _grid(direction, steps)
    m = cr.make_mlp(Ws, bs, device=dev)
    e = None if eps is None else torch.tensor(eps, device=dev)
    rc, traj = _c_solve(m, torch.tensor(s0, device=dev), ts, mode, mask, e)
    assert rc == 0
    cols = ar.columns(mode, mask)
    old = [k for k, n in enumerate(cols) if n not in ("L1", "L2")] + list(range(a, a + d))
    if mask & 3:
        rc, want = _c_solve(m, torch.tensor(np.ascontiguousarray(s0[:, old]), device=dev), ts, mode, mask & 3, e)
        assert rc == 0
    else:
        node = NeuralODE(cfm_amd.CNF(m, estimator="exact" if mode == 0 else "hutch_gaussian", noise=e), solver="euler")
        want = node.trajectory(torch.tensor(np.ascontiguousarray(s0[:, old]), device=dev), torch.tensor(ts))
        assert node.last_path == "hip"
    assert torch.equal(traj[:, :, old], want)
    ref = torch.stack(ar.solve(ar.tr.as_params(Ws, bs, False), torch.tensor(s0.astype(np.float64)), ts, mode, mask,
                               None if eps is None else torch.tensor(eps.astype(np.float64)))).detach().numpy()
    got = traj.cpu().double().numpy()
    for k, n in enumerate(cols):
        if n in ("L1", "L2"):
            # the column starts at 0.1 N(0, 1) and only grows: max|b| is a scale for it
            err = _rel(got[:, :, k], ref[:, :, k])
            print(f"{_sid(shape)} mode {mode} mask {mask} {direction}: {n} {err:.2e}")
            assert err <= BOUND, (n, err)


# ---- gradient ----------------------------------------------------------------------------------------------------------
GRAD_SHAPES = SHAPES[:3] + [(63, W64, 17, 3)]


@functools.lru_cache(maxsize=None)
def _grad_case(shape, mask, hutch, direction):
    d, w, B, steps = shape
    a = ar.n_aug(0, mask)
    n = B + B // 16 + 2
    Ws, bs = cr.mlp_params(d, w, 1)
    g = np.random.default_rng(1)
    xa = np.concatenate([g.normal(size=(n, a)) * 0.1, g.normal(size=(n, d))], 1).astype(np.float32)
    G = (0.5 + g.normal(size=(n, a + d))).astype(np.float32)
    eps = g.normal(size=(n, d)).astype(np.float32) if hutch else None
    ts = _grid(direction, steps)
    mode = 1 if hutch else 0
    keep = ar.usable_rows(Ws, bs, xa, ts, mode, mask, eps, tol=1e-5)
    dropped = int((~keep).sum())
    assert dropped <= B / 4, f"{dropped} of {n} drawn rows within 1e-5 of a kink"
    xa, G = xa[keep][:B], G[keep][:B]
    eps = None if eps is None else eps[keep][:B]
    assert len(xa) == B, (len(xa), B)
    out64, gp64, gx64 = ar.grads_for_upstream(Ws, bs, xa, ts, G, mode, mask, eps)
    for q in (xa, G, ts, out64, gx64, *gp64, *Ws, *bs, *(() if eps is None else (eps,))):
        q.setflags(write=False)
    return Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped


def _make(Ws, bs, mask, eps, dev):
    m = cr.make_mlp(Ws, bs, device=dev)
    kw = dict(COEFF[b] for b in (1, 2, 4, 8) if mask & b)
    return m, cfm_amd.RegularizedCNF(m, estimator="exact" if eps is None else "hutch_gaussian",
                                     noise=None if eps is None else torch.tensor(eps, device=dev), **kw)


def _hip_grads(Ws, bs, xa, G, eps, ts, mask, x_grad=True):
    dev = torch.device("cuda")
    m, cnf = _make(Ws, bs, mask, eps, dev)
    assert cnf.reg_mask == mask and cnf.names == ar.columns(0, mask)
    x = torch.tensor(xa, device=dev, requires_grad=x_grad)
    out = cnf.solve(x, torch.tensor(ts))
    ps = [p for l in m._linears() for p in (l.weight, l.bias)]
    g = torch.autograd.grad((out * torch.tensor(G, device=dev)).sum(), ps + ([x] if x_grad else []))
    return cnf, out.detach(), [q.detach().cpu().double().numpy() for q in g]


def _grad_cases():
    for shape in GRAD_SHAPES:
        for direction in (("down", "up") if shape in SHAPES[:3] else ("down",)):
            for mask, hutch in [(4, False), (8, False), (12, False), (13, False), (15, False), (4, True), (13, True)]:
                yield pytest.param(shape, mask, hutch, direction,
                                   id=f"{_sid(shape)}-mask{mask}-{'hutch' if hutch else 'exact'}-{direction}")


@pytest.mark.parametrize("shape,mask,hutch,direction", list(_grad_cases()))
def test_gradient_against_float64(shape, mask, hutch, direction):
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped = _grad_case(shape, mask, hutch, direction)
    cnf, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, mask)
    assert cnf.last_path == "hip"
    assert np.all(np.isfinite(out.cpu().numpy()))
    errs = {n: _rel(a, b) for n, a, b in zip(NAMES, got, gp64 + [gx64])}
    print(f"{_sid(shape)} mask {mask} {'hutch' if hutch else 'exact'} {direction}: dropped {dropped}; "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert np.isfinite(v) and v <= BOUND, (k, v, errs)
    # the forward value: every augmented column of the final state
    o = out.cpu().double().numpy()
    for k, n in enumerate(ar.columns(0, mask)):
        if n != "log_prob":
            assert _rel(o[:, k], out64[:, k]) <= BOUND, n


@pytest.mark.parametrize("mask,hutch", [(15, False), (13, True)])
def test_two_backward_calls_give_the_same_bits(mask, hutch):
    Ws, bs, xa, G, eps, ts, *_ = _grad_case(SHAPES[0], mask, hutch, "down")
    a = _hip_grads(Ws, bs, xa, G, eps, ts, mask)[2]
    b = _hip_grads(Ws, bs, xa, G, eps, ts, mask)[2]
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("mask,hutch", [(12, False), (4, True)])
def test_state_without_requires_grad_keeps_the_parameter_gradients_bits(mask, hutch):
    Ws, bs, xa, G, eps, ts, *_ = _grad_case(SHAPES[1], mask, hutch, "up")
    with_x = _hip_grads(Ws, bs, xa, G, eps, ts, mask)
    without = _hip_grads(Ws, bs, xa, G, eps, ts, mask, x_grad=False)
    assert with_x[0].last_path == without[0].last_path == "hip"
    assert len(with_x[2]) == 9 and len(without[2]) == 8
    for p, q in zip(with_x[2], without[2]):
        assert np.array_equal(p, q)


def test_two_backward_calls_on_the_grid_stride_give_the_same_bits():
    """4101 rows: every workgroup's accumulators live through a second tile and 256 partials are added."""
    shape = SHAPES[5]
    d, w, B, steps = shape
    Ws, bs = cr.mlp_params(d, w, 1)
    g = np.random.default_rng(1)
    xa = np.concatenate([np.zeros((B, 3)), g.normal(size=(B, d))], 1).astype(np.float32)
    G = (0.5 + g.normal(size=(B, 3 + d))).astype(np.float32)
    ts = _grid("down", steps)
    a = _hip_grads(Ws, bs, xa, G, None, ts, 12)
    b = _hip_grads(Ws, bs, xa, G, None, ts, 12)
    assert a[0].last_path == "hip"
    for p, q in zip(a[2], b[2]):
        assert np.all(np.isfinite(p)) and np.array_equal(p, q)


# ---- refusals at the C entries -----------------------------------------------------------------------------------------
def _refusal_net(dev):
    Ws, bs = cr.mlp_params(1, 16, 1)
    return cr.make_mlp(Ws, bs, device=dev)


@pytest.mark.parametrize("mode,mask,n_t,why", [(2, 2, 3, "no trace with the Jacobian bit"), (2, 6, 3, "no trace with the Jacobian bit"),
                                               (2, 0, 3, "no trace and no column"), (3, 4, 3, "mode 3"), (0, 16, 3, "mask 16"),
                                               (2, 4, 7, "n_t > 3 B D")])
def test_forward_entry_refuses_and_enqueues_nothing(mode, mask, n_t, why):
    dev = torch.device("cuda")
    m = _refusal_net(dev)
    D = 1 + ar.n_aug(min(mode, 2), mask & 15)
    if why == "n_t > 3 B D":
        assert n_t > 3 * 1 * D
    lib = _lib.load()
    Wp, bp, dims, keep = m.hip_params(dev)
    state = torch.zeros(1, D, device=dev)
    ts = np.linspace(0, 1, n_t).astype(np.float32)
    traj = torch.full((n_t, 1, D), 7.0, device=dev)
    jsq = torch.full((n_t, 1), 7.0, device=dev)
    ws = _lib.workspace(_lib.OP_ODE, 1, 16, D, dev)
    nfe = ctypes.c_int(-5)
    rc = lib.cfm_ode_euler_cnf_reg_mlp_f32(Wp, bp, dims, 4, ptr(state), 1, ts.ctypes.data_as(ctypes.c_void_p), n_t, mode, None,
                                           mask, ptr(traj), ptr(jsq), ctypes.byref(nfe), ptr(ws), stream_ptr())
    torch.cuda.synchronize()
    assert rc == EINVAL, why
    assert bool((traj == 7.0).all()) and bool((jsq == 7.0).all()) and nfe.value == -5


def test_gradient_entry_refuses_no_trace_and_enqueues_nothing():
    dev = torch.device("cuda")
    m = _refusal_net(dev)
    lib = _lib.load()
    params = [p for l in m._linears() for p in (l.weight, l.bias)]
    Ws, bs, Wp, bp = _lib.param_tables(params, dev)
    dWs, dbs, dWp, dbp = _lib.grad_tables(Ws, bs)
    for q in dWs + dbs:
        q.fill_(7.0)
    cdims = (ctypes.c_int * 5)(*m.dims())
    n_t, D = 3, 2
    ts = np.linspace(0, 1, n_t).astype(np.float32)
    traj = torch.zeros(n_t, 1, D, device=dev)
    G = torch.ones(1, D, device=dev)
    g0 = torch.full((1, D), 7.0, device=dev)
    ws = _lib.workspace(_lib.OP_CNF_GRAD, 1, n_t, 0, dev)
    for mode, mask in [(2, 4), (3, 4), (0, 16), (1, 6)]:
        rc = lib.cfm_cnf_reg_euler_grad_f32(Wp, bp, cdims, 4, ptr(traj), 1, ts.ctypes.data_as(ctypes.c_void_p), n_t, mode, None,
                                            mask, None, ptr(G), dWp, dbp, ptr(g0), ptr(ws), stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (mode, mask)
        assert bool((g0 == 7.0).all()) and all(bool((q == 7.0).all()) for q in dWs + dbs)


# ---- a side stream -----------------------------------------------------------------------------------------------------
def test_side_stream_gives_the_default_stream_s_bits():
    dev = torch.device("cuda")
    Ws, bs, x0, ts, want = _fwd_case(SHAPES[0], "up")
    m = cr.make_mlp(Ws, bs, device=dev)
    s0 = torch.cat([torch.zeros(len(x0), 3, device=dev), torch.tensor(x0, device=dev)], 1)
    gWs, gbs, xa, G, eps, gts, *_ = _grad_case(SHAPES[1], 4, False, "down")
    rc, traj = _c_solve(m, s0, ts, 2, 13)
    grads = _hip_grads(gWs, gbs, xa, G, eps, gts, 4)[2]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc2, traj2 = _c_solve(m, s0, ts, 2, 13)
        grads2 = _hip_grads(gWs, gbs, xa, G, eps, gts, 4)[2]
    s.synchronize()
    assert rc == 0 and rc2 == 0 and torch.equal(traj, traj2)
    for p, q in zip(grads, grads2):
        assert np.array_equal(p, q)


# ---- end to end: the runner's validation loop ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _runner_case():
    Ws, bs = cr.mlp_params(2, 64, 3)
    x0 = np.random.default_rng(3).normal(size=(256, 2)).astype(np.float32)
    return Ws, bs, x0


def test_the_runner_s_loop_runs_in_one_launch():
    from cfm_amd.utils import torch_wrapper
    dev = torch.device("cuda")
    Ws, bs, x0 = _runner_case()
    m = cr.make_mlp(Ws, bs, device=dev)
    am = cfm_amd.AugmentationModule(l1_reg=1, l2_reg=1, squared_l2_reg=1)
    solver = cfm_amd.FlowSolver(torch_wrapper(m), 2, ode_solver="euler", augmentations=am)
    t_span = torch.linspace(0, 1, 101)
    traj, aug = solver.odeint(torch.tensor(x0, device=dev), t_span)
    assert solver.last_path == "hip" and solver.nfe == 100
    assert traj.shape == (101, 256, 2) and aug.shape == (101, 256, 3)
    assert not aug[0].any() and torch.equal(traj[0], torch.tensor(x0, device=dev))
    want = ar.trajectory64(Ws, bs, x0, t_span.numpy(), 2, 13)
    got = aug[-1].double().mean(0).cpu().numpy()
    ref = want[-1][:, :3].mean(0)
    for n, a, b in zip(am.names, got, ref):
        print(f"runner loop {n}: {a:.8f} float64 {b:.8f} ({abs(a - b) / abs(b):.2e})")
        assert abs(a - b) <= BOUND * abs(b), n
    reg, x = am(torch.cat([aug[-1], traj[-1]], 1))
    assert reg.shape == (256, 3) and torch.equal(x, traj[-1])
    # without augmentations the call is the one it was: a tensor, from NeuralODE on the drift callable (a launch per
    # step, x + dt * f in torch ops: the same solve, not the same bits)
    solver.augmentations = None
    bare = solver.odeint(torch.tensor(x0, device=dev), t_span)
    assert torch.is_tensor(bare) and bare.shape == traj.shape and solver.nfe == 100
    assert _rel(bare.cpu().double().numpy(), want[:, :, 3:]) <= BOUND
    # the fused path switched off: the declined call is stepped in torch ops, nothing is printed
    solver.augmentations = am
    lib = _lib.load()
    lib.cfm_ode_set_fused(0)
    try:
        t2, a2 = solver.odeint(torch.tensor(x0, device=dev), torch.linspace(0, 1, 6))
    finally:
        lib.cfm_ode_set_fused(1)
    assert solver.last_path == "eager" and a2.shape == (6, 256, 3)


def test_rk4_takes_the_eager_path_and_agrees_with_the_restatement():
    from cfm_amd.utils import torch_wrapper
    dev = torch.device("cuda")
    Ws, bs, x0 = _runner_case()
    m = cr.make_mlp(Ws, bs, device=dev)
    am = cfm_amd.AugmentationModule(l1_reg=1, l2_reg=1, squared_l2_reg=1)
    solver = cfm_amd.FlowSolver(torch_wrapper(m), 2, ode_solver="rk4", augmentations=am)
    t_span = torch.linspace(0, 1, 11)
    traj, aug = solver.odeint(torch.tensor(x0, device=dev), t_span)
    assert solver.last_path == "eager" and solver.nfe == 40
    want = ar.trajectory64(Ws, bs, x0, t_span.numpy(), 2, 13, scheme="rk4")
    assert _rel(traj.cpu().double().numpy(), want[:, :, 3:]) <= BOUND
    for k, n in enumerate(am.names):
        err = _rel(aug[:, :, k].cpu().double().numpy(), want[:, :, k])
        print(f"rk4 eager {n}: {err:.2e}")
        assert err <= BOUND, (n, err)
