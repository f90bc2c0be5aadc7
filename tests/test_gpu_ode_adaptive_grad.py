"""GPU: AdaptiveDifferentiableNeuralODE on the HIP path (forward cfm_ode_adaptive_rec_mlp_f32, backward
cfm_ode_adaptive_grad_f32) against the float64 replay (tests/ode_adaptive_grad_restate.py) of the step log the GPU
forward returned, for dopri5 and tsit5, plus the properties a training loop through the sampler relies on.

Bound (that of test_gpu_ode_grad.py): per gradient tensor, the eight parameter tensors and dx,
max|g_hip - g_64| / max|g_64| <= 1e-5.  The upstream gradient G is random with mean 0.5 on ALL n_t slices of the
trajectory; one case has it on the last slice only.  The nets are cnf_restate.smooth_mlp_params: every hidden
pre-activation is negative inside [-3, 3]^d, so no row sits near a SELU kink; each case asserts that its trajectory stays
in that box and that no stage point of the float64 replay is within 1e-5 of a kink.  One case per tableau runs the
default-initialised net, where both branches are taken: rows within 1e-5 of a kink at some stage point get G = 0 on every
slice and are left out of the dx comparison (at most a quarter of them).

What float32 arithmetic alone does to these gradients (tsit5 has tableau entries near 13) is measured on the CPU by
tests/test_ode_adaptive_grad_host.py::test_float32_replay_leaves_three_quarters_of_the_bound: the float32 replay against
the float64 replay of the same log, on the logs of the generic float32 path for every shape below, both directions, at
this file's tolerances.  Largest ratio over the nine tensors, dopri5 / tsit5:
    d 2,  64-64-64, B 48,   2 points    3.5e-07 / 9.7e-07
    d 2,  64-64-64, B 48,   9 points    2.5e-07 / 5.8e-07
    d 5,  48-48-48, B 19,   4 points    2.8e-07 / 6.9e-07
    d 1,  16-16-16, B 33,   4 points    2.0e-07 / 5.5e-07
    d 5,  33-64-48, B 37,   4 points    3.2e-07 / 1.1e-06
    d 63, 33-33-33, B 17,   3 points    3.9e-07 / 2.1e-06
    d 2,  64-64-64, B 4101, 3 points    2.7e-07 / 5.7e-07
    d 2,  16-16-16, B 8197, 2 points    2.1e-07 / 4.4e-07     (8192 + 5: the resident limit of 256 CUs x 2 workgroups)
    default-initialised nets (ode_adaptive_grad_restate.DEFAULT_NET, kinked rows zeroed)    2.7e-07 / 1.2e-06
A quarter of 1e-5 (2.5e-06) covers every one of them, so the bound is 1e-5 for every case."""
import numpy as np
import pytest
import torch

import cfm_amd
import cnf_restate as cr
import ode_adaptive_grad_restate as ar
from cfm_amd import _lib
from cfm_amd.ode import NeuralODE
from cfm_amd.utils import torch_wrapper

pytestmark = pytest.mark.gpu

BOUND = 1e-5
BOX = ar.BOX
CG_MAXGRID = 256          # csrc/cnf_grad.h: workgroups (= partial gradients) of the backward at most
NAMES = ["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dx"]
SOLVERS = ar.SOLVERS
TOL = ar.GPU_TOL
SHAPES, STRIDE = ar.GPU_SHAPES, ar.STRIDE_SHAPE          # (d, hidden widths, B, t_span points)
_grid, _inputs = ar.grid, ar.smooth_case


def _sid(s):
    return "d%d_w%s_B%d_nt%d" % (s[0], "-".join(map(str, s[1])), s[2], s[3])


def _hip(Ws, bs, x, G, ts, solver, x_grad=True, backward=True, **kw):
    dev = torch.device("cuda")
    m = cr.make_mlp(Ws, bs, device=dev)
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m), solver=solver, **{**TOL, **kw})
    xt = torch.tensor(x, device=dev, requires_grad=x_grad)
    traj = node.trajectory(xt, torch.tensor(ts))
    if not backward:
        return node, m, traj.detach(), None
    ps = [p for l in m._linears() for p in (l.weight, l.bias)]
    g = torch.autograd.grad((traj * torch.tensor(G, device=dev)).sum(), ps + ([xt] if x_grad else []))
    return node, m, traj.detach(), [q.detach().cpu().double().numpy() for q in g]


def _tsign(ts):
    return 1.0 if ts[1] > ts[0] else -1.0


def _report(tag, got, want, rows=None, bound=BOUND):
    """Every ratio is printed before anything is asserted.  rows: the rows of dx that are compared."""
    bad, line = [], []
    for n, a, b in zip(NAMES, got, want):
        if n == "dx" and rows is not None:
            a, b = a[rows], b[rows]
        scale, err = float(np.abs(b).max()), float(np.abs(a - b).max())
        line.append(f"{n} {err / scale:.2e}")
        if not np.all(np.isfinite(a)) or err > bound * scale:
            bad.append((n, err / scale))
    print(f"{tag}: " + " ".join(line))
    assert not bad, bad


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def _check_against_replay(tag, shape, solver, direction, last_only=False):
    Ws, bs, x, G = _inputs(shape, last_only)
    ts = _grid(direction, shape[3])
    node, m, traj, got = _hip(Ws, bs, x, G, ts, solver)
    assert node.last_path == "hip" and tuple(traj.shape) == (shape[3],) + x.shape
    log = node.step_log.numpy()
    assert log.shape == (node.n_accepted, 4) and node.n_steps >= node.n_accepted >= shape[3] - 1
    assert node.nfe == 2 + 6 * node.n_steps
    traj64, gp64, gx64 = ar.grads_for_upstream(Ws, bs, x, log, G, solver, _tsign(ts))
    dist = ar.kink_distance(Ws, bs, x, log, shape[3], solver, _tsign(ts))
    print(f"{tag}: accepted {node.n_accepted} of {node.n_steps}, max|y| {np.abs(traj64).max():.3f}, kink distance {dist.min():.3e}")
    assert np.abs(traj64).max() <= BOX and dist.min() >= 1e-5
    assert _rel(traj.cpu().double().numpy(), traj64) <= BOUND
    _report(tag, got, gp64 + [gx64])
    return node


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_gradient_against_float64_replay(shape, solver, direction):
    _check_against_replay(f"{_sid(shape)} {solver} {direction}", shape, solver, direction)


@pytest.mark.parametrize("solver", SOLVERS)
def test_endpoint_loss_against_float64_replay(solver):
    """G non-zero on the last slice only: the loss on traj[-1] that a sampler is trained through."""
    G = _inputs(SHAPES[4], True)[3]
    assert not G[:-1].any() and G[-1].any()
    _check_against_replay(f"{_sid(SHAPES[4])} {solver} endpoint", SHAPES[4], solver, "down", last_only=True)


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_grid_stride_gradient_against_float64_replay(solver, direction):
    """More tiles than the backward has workgroups: every workgroup's accumulators live through a second tile, and the
    reduction adds CG_MAXGRID partials."""
    assert -(-STRIDE[2] // 16) > CG_MAXGRID and STRIDE[2] % 16 != 0
    _check_against_replay(f"{_sid(STRIDE)} {solver} {direction}", STRIDE, solver, direction)


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_streamed_recording_forward_against_float64_replay(solver, direction):
    """B just above the rows the recording forward keeps in registers (asked of the library): its streamed instantiation
    runs, x and k_1 travel through the parity buffers and ysteps is copied from them."""
    limit = _lib.load().cfm_ode_rec_resident_rows(_lib.ODE_TABLEAU[solver])
    assert limit >= 16 and limit % 16 == 0, limit
    shape = ar.streamed_shape(limit)
    node = _check_against_replay(f"{_sid(shape)} {solver} {direction} (resident limit {limit})", shape, solver, direction)
    plain = NeuralODE(node.vf, solver=solver, **TOL)
    Ws, bs, x, G = _inputs(shape)
    dev = torch.device("cuda")
    ts = _grid(direction, 2)
    want = plain.trajectory(torch.tensor(x, device=dev), torch.tensor(ts))
    again = node.trajectory(torch.tensor(x, device=dev, requires_grad=True), torch.tensor(ts))
    assert torch.equal(again.detach(), want) and (node.nfe, node.n_steps) == (plain.nfe, plain.n_steps)


# ---- the default-initialised net: both SELU branches, rejected attempts -------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_default_initialised_net_with_rejected_attempts_and_kinked_rows_zeroed(solver):
    """Both SELU branches run and the controller rejects attempts (n_steps > n_accepted).  The step sequence depends on every
    row, so nothing is removed from the solve: rows within 1e-5 of a kink at some stage point of the float64 replay get
    G = 0 on every slice before backward and are left out of the dx comparison."""
    Ws, bs, x, G, ts, tol = ar.default_case(solver)
    B, n_t = len(x), len(ts)
    node, m, traj, _ = _hip(Ws, bs, x, G, ts, solver, backward=False, atol=tol, rtol=tol)
    assert node.last_path == "hip"
    log = node.step_log.numpy()
    keep = ar.kink_distance(Ws, bs, x, log, n_t, solver, 1.0) >= 1e-5
    dropped = int((~keep).sum())
    print(f"default net {solver}: accepted {node.n_accepted} of {node.n_steps}, {dropped} of {B} rows within 1e-5 of a kink")
    assert node.n_steps > node.n_accepted                  # rejected attempts, which the log does not carry
    assert dropped <= B / 4
    G = G.copy(); G[:, ~keep] = 0.0
    node2, m, traj2, got = _hip(Ws, bs, x, G, ts, solver, atol=tol, rtol=tol)
    assert torch.equal(traj, traj2) and torch.equal(node.step_log, node2.step_log)
    traj64, gp64, gx64 = ar.grads_for_upstream(Ws, bs, x, log, G, solver, 1.0)
    z = np.concatenate([x, np.zeros((B, 1), np.float32)], 1) @ Ws[0].T + bs[0]
    assert (z > 0).any() and (z < 0).any()                 # both branches really run
    assert _rel(traj.cpu().double().numpy()[:, keep], traj64[:, keep]) <= BOUND
    _report(f"default net {solver}", got, gp64 + [gx64], rows=keep)


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_steps_are_clamped_onto_the_interior_points_of_the_grid(solver, direction):
    """Nine points: the controller's step is cut to the float32 distance to the next point, the log lands on every point
    in order, and a step that follows a landing starts ON the point while its k_1 was evaluated at the landing step's
    t + dt."""
    shape = SHAPES[1]
    Ws, bs, x, G = _inputs(shape)
    ts = _grid(direction, shape[3])
    node = _hip(Ws, bs, x, G, ts, solver, backward=False)[0]
    t, dt, tk1, out = node.step_log.numpy().T
    s = (_tsign(ts) * ts).astype(np.float32)
    print(f"{solver} {direction}: accepted {node.n_accepted} of {node.n_steps} attempts; out {out.astype(int).tolist()}")
    assert [int(o) for o in out if o >= 0] == list(range(1, len(ts)))
    interior = [n for n in range(len(out)) if 1 <= out[n] < len(ts) - 1]
    assert len(interior) == len(ts) - 2
    for n in interior:
        assert np.float32(dt[n]) == np.float32(s[int(out[n])] - np.float32(t[n]))
        assert t[n + 1] == s[int(out[n])] and tk1[n + 1] == np.float32(np.float32(t[n]) + np.float32(dt[n]))
    assert np.all(np.diff(t) > 0) and tk1[0] == t[0] == s[0]


# ---- bit-level properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], STRIDE], ids=_sid)
def test_forward_is_the_sampler_s_bit_for_bit_and_ysteps_are_its_slices(shape, solver, direction, monkeypatch):
    lib = _lib.load()
    entry = lib.cfm_ode_adaptive_grad_f32
    seen = []

    def spy(*args):
        seen.append(args)
        return entry(*args)
    monkeypatch.setattr(lib, "cfm_ode_adaptive_grad_f32", spy)
    Ws, bs, x, G = _inputs(shape)
    ts = _grid(direction, shape[3])
    dev = torch.device("cuda")
    m = cr.make_mlp(Ws, bs, device=dev)
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m), solver=solver, **TOL)
    traj = node.trajectory(torch.tensor(x, device=dev, requires_grad=True), torch.tensor(ts))
    plain = NeuralODE(torch_wrapper(m), solver=solver, **TOL)
    want = plain.trajectory(torch.tensor(x, device=dev), torch.tensor(ts))
    assert node.last_path == "hip" and plain.last_path == "hip"
    assert traj.requires_grad and torch.equal(traj.detach(), want)
    assert (node.nfe, node.n_steps) == (plain.nfe, plain.n_steps)
    # ysteps: what the backward is handed.  ysteps[0] = x0, and ysteps[n + 1] is the slice the step n landed on
    ysteps, log = traj.grad_fn.saved_tensors[:2]
    out = node.step_log[:, 3].long().tolist()
    assert tuple(ysteps.shape) == (node.n_accepted,) + x.shape and tuple(log.shape) == (node.n_accepted, 4)
    assert torch.equal(ysteps[0], want[0])
    for n, o in enumerate(out[:-1]):
        if o >= 0:
            assert torch.equal(ysteps[n + 1], want[o]), (n, o)
    assert out[-1] == shape[3] - 1
    traj.sum().backward()
    assert len(seen) == 1 and seen[0][6] == node.n_accepted           # the gradient entry is called once


@pytest.mark.parametrize("solver", SOLVERS)
def test_two_backward_calls_give_the_same_bits_on_the_grid_stride(solver):
    """The partials are added in workgroup order: 256 of them, each the sum of 16 or 17 tiles' rows."""
    Ws, bs, x, G = _inputs(STRIDE)
    ts = _grid("down", STRIDE[3])
    a = _hip(Ws, bs, x, G, ts, solver)[3]
    b = _hip(Ws, bs, x, G, ts, solver)[3]
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("solver", SOLVERS)
def test_state_without_requires_grad_gets_no_dx_and_the_same_parameter_gradients(solver, monkeypatch):
    lib = _lib.load()
    entry = lib.cfm_ode_adaptive_grad_f32
    g_initial = []

    def spy(*args):
        g_initial.append(args[14].value)          # a c_void_p: None is NULL
        return entry(*args)
    monkeypatch.setattr(lib, "cfm_ode_adaptive_grad_f32", spy)
    Ws, bs, x, G = _inputs(SHAPES[4])
    ts = _grid("down", SHAPES[4][3])
    with_x = _hip(Ws, bs, x, G, ts, solver)
    without = _hip(Ws, bs, x, G, ts, solver, x_grad=False)
    assert with_x[0].last_path == without[0].last_path == "hip"
    assert len(g_initial) == 2 and g_initial[0] is not None and g_initial[1] is None
    assert len(with_x[3]) == 9 and len(without[3]) == 8
    for p, q in zip(with_x[3], without[3]):
        assert np.array_equal(p, q)


# ---- dispatch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_fused_path_off_runs_generic_and_agrees(solver):
    """The generic path in torch ops on the GPU takes (nearly) the same steps; each path is held to the float64 replay of
    ITS OWN log, and on equal step counts the two gradients agree within the bound."""
    shape = SHAPES[4]
    Ws, bs, x, G = _inputs(shape)
    ts = _grid("up", shape[3])
    lib = _lib.load()
    lib.cfm_ode_set_fused(0)
    try:
        gen = _hip(Ws, bs, x, G, ts, solver)
    finally:
        lib.cfm_ode_set_fused(1)
    assert gen[0].last_path == "generic"
    _, gp64, gx64 = ar.grads_for_upstream(Ws, bs, x, gen[0].step_log.numpy(), G, solver, 1.0)
    _report(f"{_sid(shape)} {solver} generic path", gen[3], gp64 + [gx64])
    hip = _hip(Ws, bs, x, G, ts, solver)
    assert hip[0].last_path == "hip"
    assert hip[0].n_accepted == gen[0].n_accepted and hip[0].n_steps == gen[0].n_steps
    _report(f"{_sid(shape)} {solver} hip against generic", hip[3], gen[3])


@pytest.mark.parametrize("solver", SOLVERS)
def test_a_width_65_net_takes_the_generic_path(solver):
    Ws, bs = cr.smooth_mlp_params(2, (65, 64, 64), 1, box=BOX)
    g = np.random.default_rng(1)
    x, ts = g.uniform(-1.5, 1.5, size=(19, 2)).astype(np.float32), _grid("up", 4)
    G = (0.5 + g.normal(size=(4, 19, 2))).astype(np.float32)
    node, m, traj, got = _hip(Ws, bs, x, G, ts, solver)
    assert node.last_path == "generic" and tuple(traj.shape) == (4, 19, 2)
    _, gp64, gx64 = ar.grads_for_upstream(Ws, bs, x, node.step_log.numpy(), G, solver, 1.0)
    _report(f"width 65 {solver} generic path", got, gp64 + [gx64])


@pytest.mark.parametrize("solver", SOLVERS)
def test_full_log_raises_and_leaves_the_library_usable(solver):
    Ws, bs, x, G = _inputs(SHAPES[1])
    ts = _grid("up", SHAPES[1][3])
    node, m, traj, got = _hip(Ws, bs, x, G, ts, solver)
    need = node.n_accepted
    assert need >= len(ts) - 1
    with pytest.raises(RuntimeError, match="max_steps"):
        _hip(Ws, bs, x, G, ts, solver, max_steps=need - 1)
    with pytest.raises(RuntimeError, match="max_steps"):
        _hip(Ws, bs, x, G, ts, solver, max_steps=1)
    exact = _hip(Ws, bs, x, G, ts, solver, max_steps=need)              # exactly enough, and the library still works
    assert exact[0].last_path == "hip" and exact[0].n_accepted == need and torch.equal(exact[2], traj)
    for p, q in zip(exact[3], got):
        assert np.array_equal(p, q)


def _one_step(solver, path_off):
    """Parameters after one Adam step on a loss on traj[-1] from fixed weights.  Adam's first step is lr g / (|g| + eps):
    with eps = 1e-3 its slope in g is at most lr / eps = 1, so a gradient error of 1e-5 max|g| moves a parameter by no
    more than that."""
    dev = torch.device("cuda")
    Ws, bs = cr.smooth_mlp_params(2, 64, 5, box=BOX)
    m = cr.make_mlp(Ws, bs, device=dev)
    torch.manual_seed(9)
    x = torch.rand(48, 2, device=dev) * 3 - 1.5
    target = torch.randn(48, 2, device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-3)
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m), solver=solver, **TOL)
    lib = _lib.load()
    if path_off:
        lib.cfm_ode_set_fused(0)
    try:
        opt.zero_grad()
        loss = ((node.trajectory(x, torch.linspace(0, 1, 5))[-1] - target) ** 2).mean()
        loss.backward()
    finally:
        lib.cfm_ode_set_fused(1)
    assert node.last_path == ("generic" if path_off else "hip")
    opt.step()
    return node.n_accepted, [p.detach().cpu().double().numpy() for p in m.parameters()]


@pytest.mark.parametrize("solver", SOLVERS)
def test_one_adam_step_matches_the_generic_path(solver):
    n_want, want = _one_step(solver, path_off=True)
    n_got, got = _one_step(solver, path_off=False)
    assert n_got == n_want
    for a, b in zip(got, want):
        r = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"{solver} one Adam step: {r:.2e}")
        assert r <= 1e-5
