"""GPU: DifferentiableNeuralODE on the HIP path (forward cfm_ode_fixed_mlp_f32, backward cfm_ode_fixed_grad_f32) against
the float64 restatement of tests/ode_grad_restate.py, for euler, midpoint and rk4, plus the properties a training loop
through the sampler relies on.  Measured ratios: DESIGN.md 4.12.

Bound (that of test_gpu_cnf_train.py): per gradient tensor, the eight parameter tensors and dx,
max|g_hip - g_64| / max|g_64| <= 1e-5.  The upstream gradient G is random with mean 0.5 on ALL n_t slices of the
trajectory, so no tensor is a cancelled sum; one case has G on the last slice only (an endpoint loss).  Rows within 1e-5
of a SELU kink at ANY stage point of the float64 solve are dropped before anything runs (an fp32 evaluation may take the
other branch there); B is the number of rows kept, and at most a quarter of the drawn rows may go."""
import functools

import numpy as np
import pytest
import torch

import cfm_amd
import cnf_restate as cr
import ode_grad_restate as og
from cfm_amd.utils import torch_wrapper

pytestmark = pytest.mark.gpu

BOUND = 1e-5
CG_MAXGRID = 256          # csrc/cnf_grad.h: workgroups (= partial gradients) at most
W64, W33, WMIX, WMIX2 = (64, 64, 64), (33, 33, 33), (64, 17, 40), (33, 64, 48)
NAMES = ["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dx"]
SCHEMES = og.SCHEMES

# (d, hidden widths, B = rows KEPT, steps)
SHAPES = [
    (2, W64, 48, 8),                # three full tiles, the tutorial's net
    (5, (48, 48, 48), 19, 5),       # partial widths, partial tile
    (1, (16, 16, 16), 33, 3),       # d = 1
    (2, W64, 1, 4),                 # one row: B d < n_t, the forward runs layer by layer
    (2, WMIX, 48, 8),               # non-square layers
    (5, WMIX2, 37, 5),              # non-square layers, partial tile
    (63, W64, 40, 3),               # the time in column 63 of W0
    (63, W33, 17, 3),               # the same at partial widths and a partial tile
    (2, W64, 40, 1),                # n_t = 2
]
# more tiles than workgroups: the grid stride takes a second pass, 256 partials are added, the last tile is partial
STRIDE = [((2, W64, 16 * CG_MAXGRID + 5, 4), "down"), ((2, WMIX, 16 * CG_MAXGRID + 5, 3), "up")]
LONG = (2, W64, 48, 100)            # n_t = 101: the t_span copy takes two 256-byte slots; most terms per accumulator


def _sid(s):
    return "d%d_w%s_B%d_n%d" % (s[0], "-".join(map(str, s[1])), s[2], s[3])


def _grid(direction, steps):
    if direction == "down":
        return np.linspace(1.0, 0.0, steps + 1).astype(np.float32)
    w = 1.0 + 0.6 * np.sin(1.7 * np.arange(steps) + 0.3)          # 0 -> 1, non-uniform
    return np.concatenate([[0.0], np.cumsum(w) / w.sum()]).astype(np.float32)


def _drawn(B):
    """Rows drawn for B kept rows.  Up to 16 tiles: B + B/3 + 2 >= 4 B / 3, so a draw within the cap of a quarter always
    keeps B.  The 4101-row cases draw B + B/8 + 2: rk4 loses 6 to 7 % of them on the reference alone."""
    return B + B // 8 + 2 if B > 16 * CG_MAXGRID else B + B // 3 + 2


@functools.lru_cache(maxsize=None)
def _ref(shape, scheme, direction, last_only=False, seed=1):
    """fp32 inputs and the float64 reference of one case, computed once, shared and never written to."""
    d, w, B, steps = shape
    ts = _grid(direction, steps)
    g = np.random.default_rng(seed)
    if shape == LONG:
        # a net that stays on SELU's smooth branch inside [-3, 3]^2: the default-initialised one loses 29 to 46 % of 96
        # drawn rows to kinks over 100 steps on the reference alone, so no honest cap exists there
        Ws, bs = cr.smooth_mlp_params(d, 64, seed)
        n = B
        x = g.uniform(-1.5, 1.5, size=(n, d)).astype(np.float32)
    else:
        Ws, bs = cr.mlp_params(d, w, seed)
        n = _drawn(B)
        x = g.normal(size=(n, d)).astype(np.float32)
    G = (0.5 + g.normal(size=(steps + 1, n, d))).astype(np.float32)
    if last_only:
        G[:-1] = 0.0
    keep = og.kink_free_rows(Ws, bs, x, ts, scheme, tol=1e-5)
    dropped = int((~keep).sum())
    if shape == LONG:
        assert dropped == 0, f"{dropped} rows of the smooth net within 1e-5 of a kink"
    assert dropped <= n / 4, f"{dropped} of {n} drawn rows within 1e-5 of a kink"
    x, G = np.ascontiguousarray(x[keep][:B]), np.ascontiguousarray(G[:, keep][:, :B])
    assert len(x) == B, (len(x), B)
    traj64, gp64, gx64 = og.grads_for_upstream(Ws, bs, x, ts, G, scheme)
    if shape == LONG:
        assert np.abs(traj64).max() <= 3.0, np.abs(traj64).max()
    for a in (x, G, ts, traj64, gx64, *gp64, *Ws, *bs):
        a.setflags(write=False)
    return Ws, bs, x, G, ts, traj64, gp64, gx64, dropped


def _hip_grads(Ws, bs, x, G, ts, scheme, x_grad=True):
    dev = torch.device("cuda")
    m = cr.make_mlp(Ws, bs, device=dev)
    node = cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver=scheme)
    xt = torch.tensor(x, device=dev, requires_grad=x_grad)
    traj = node.trajectory(xt, torch.tensor(ts))
    ps = [p for l in m._linears() for p in (l.weight, l.bias)]
    g = torch.autograd.grad((traj * torch.tensor(G, device=dev)).sum(), ps + ([xt] if x_grad else []))
    return node, m, traj.detach(), [q.detach().cpu().double().numpy() for q in g]


def _report(tag, got, gp64, gx64):
    """Every ratio is printed before anything is asserted."""
    bad, line = [], []
    for n, a, b in zip(NAMES, got, gp64 + [gx64]):
        scale, err = float(np.abs(b).max()), float(np.abs(a - b).max())
        line.append(f"{n} {err / scale:.2e}")
        if not np.all(np.isfinite(a)) or err > BOUND * scale:
            bad.append((n, err / scale))
    print(f"{tag}: " + " ".join(line))
    assert not bad, bad


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_gradient_against_float64(shape, scheme, direction):
    Ws, bs, x, G, ts, traj64, gp64, gx64, dropped = _ref(shape, scheme, direction)
    assert len(x) == shape[2] and len(ts) == shape[3] + 1
    node, m, traj, got = _hip_grads(Ws, bs, x, G, ts, scheme)
    assert node.last_path == "hip" and tuple(traj.shape) == traj64.shape
    assert _rel(traj.cpu().double().numpy(), traj64) <= BOUND
    _report(f"{_sid(shape)} {scheme} {direction}: dropped {dropped}", got, gp64, gx64)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_endpoint_loss_against_float64(scheme):
    """G non-zero on the last slice only: the loss on traj[-1] that a sampler is trained through."""
    Ws, bs, x, G, ts, traj64, gp64, gx64, dropped = _ref(SHAPES[5], scheme, "down", last_only=True)
    assert not G[:-1].any() and G[-1].any()
    node, m, traj, got = _hip_grads(Ws, bs, x, G, ts, scheme)
    assert node.last_path == "hip"
    _report(f"{_sid(SHAPES[5])} {scheme} endpoint: dropped {dropped}", got, gp64, gx64)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_one_point_grid_gives_zeros_and_the_upstream_gradient(scheme):
    """n_t = 1: no step.  Zero parameter gradients and g_initial == G[0], bit for bit."""
    Ws, bs = cr.mlp_params(2, 64, 1)
    g = np.random.default_rng(1)
    x, G = g.normal(size=(37, 2)).astype(np.float32), (0.5 + g.normal(size=(1, 37, 2))).astype(np.float32)
    node, m, traj, got = _hip_grads(Ws, bs, x, G, np.array([0.25], np.float32), scheme)
    assert node.last_path == "hip" and np.array_equal(traj.cpu().numpy(), x[None])
    assert all(np.all(q == 0.0) for q in got[:8])
    assert np.array_equal(got[8].astype(np.float32), G[0])


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape,direction", STRIDE, ids=[_sid(s) + "_" + k for s, k in STRIDE])
def test_grid_stride_gradient_against_float64(shape, direction, scheme):
    """More tiles than workgroups: every workgroup's accumulators live through further tiles, and the reduction adds
    CG_MAXGRID partials."""
    Ws, bs, x, G, ts, traj64, gp64, gx64, dropped = _ref(shape, scheme, direction)
    assert -(-len(x) // 16) > CG_MAXGRID and len(x) % 16 != 0
    node, m, traj, got = _hip_grads(Ws, bs, x, G, ts, scheme)
    assert node.last_path == "hip"
    _report(f"{_sid(shape)} {scheme} {direction}: dropped {dropped}", got, gp64, gx64)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_long_grid_gradient_against_float64(scheme):
    """n_t = 101 on a net without kinks inside its box: no row is dropped, and the float64 trajectory stays inside."""
    Ws, bs, x, G, ts, traj64, gp64, gx64, dropped = _ref(LONG, scheme, "down")
    assert dropped == 0 and len(ts) == 101
    node, m, traj, got = _hip_grads(Ws, bs, x, G, ts, scheme)
    assert node.last_path == "hip"
    _report(f"{_sid(LONG)} {scheme}: max|y| {np.abs(traj64).max():.3f}", got, gp64, gx64)


# ---- properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape,direction", [(SHAPES[5], "up"), STRIDE[0], STRIDE[1]],
                         ids=lambda v: _sid(v) if isinstance(v, tuple) else v)
def test_forward_value_is_the_sampler_s_bit_for_bit(shape, direction, scheme):
    from cfm_amd.ode import NeuralODE
    dev = torch.device("cuda")
    Ws, bs, x, G, ts, traj64, *_ = _ref(shape, scheme, direction)
    m = cr.make_mlp(Ws, bs, device=dev)
    node = cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver=scheme)
    traj = node.trajectory(torch.tensor(x, device=dev, requires_grad=True), torch.tensor(ts))
    plain = NeuralODE(torch_wrapper(m), solver=scheme)
    want = plain.trajectory(torch.tensor(x, device=dev), torch.tensor(ts))
    assert node.last_path == "hip" and plain.last_path == "hip"
    assert traj.requires_grad and torch.equal(traj.detach(), want)
    assert (node.nfe, node.n_steps) == (plain.nfe, plain.n_steps)
    assert _rel(want.cpu().double().numpy(), traj64) <= BOUND                             # and it is the solve


@pytest.mark.parametrize("shape,direction", STRIDE, ids=[_sid(s) + "_" + k for s, k in STRIDE])
def test_two_backward_calls_give_the_same_bits_on_the_grid_stride(shape, direction):
    """The partials are added in workgroup order: 256 of them, each the sum of 16 or 17 tiles' rows."""
    Ws, bs, x, G, ts, *_ = _ref(shape, "rk4", direction)
    a = _hip_grads(Ws, bs, x, G, ts, "rk4")[3]
    b = _hip_grads(Ws, bs, x, G, ts, "rk4")[3]
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("scheme", ["euler", "rk4"])
def test_state_without_requires_grad_gets_no_dx_and_the_same_parameter_gradients(scheme, monkeypatch):
    """x that asks for no gradient: the kernel is called with g_initial == NULL (observed at the C entry), and the eight
    parameter gradients are those of the call with it, bit for bit."""
    from cfm_amd import _lib
    lib = _lib.load()
    entry = lib.cfm_ode_fixed_grad_f32
    g_initial = []

    def spy(*args):
        g_initial.append(args[12].value)          # a c_void_p: None is NULL
        return entry(*args)
    monkeypatch.setattr(lib, "cfm_ode_fixed_grad_f32", spy)
    Ws, bs, x, G, ts, traj64, gp64, gx64, _ = _ref(SHAPES[4], scheme, "down")
    with_x = _hip_grads(Ws, bs, x, G, ts, scheme)
    without = _hip_grads(Ws, bs, x, G, ts, scheme, x_grad=False)
    assert with_x[0].last_path == without[0].last_path == "hip"
    assert len(g_initial) == 2 and g_initial[0] is not None and g_initial[1] is None
    assert len(with_x[3]) == 9 and len(without[3]) == 8
    for p, q in zip(with_x[3], without[3]):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_fused_path_off_runs_generic_and_agrees(scheme):
    from cfm_amd import _lib
    Ws, bs, x, G, ts, traj64, gp64, gx64, _ = _ref(SHAPES[5], scheme, "up")
    lib = _lib.load()
    lib.cfm_ode_set_fused(0)
    try:
        gen = _hip_grads(Ws, bs, x, G, ts, scheme)
    finally:
        lib.cfm_ode_set_fused(1)
    assert gen[0].last_path == "generic"
    _report(f"{_sid(SHAPES[5])} {scheme} generic path", gen[3], gp64, gx64)
    hip = _hip_grads(Ws, bs, x, G, ts, scheme)
    assert hip[0].last_path == "hip"


def test_a_width_65_net_takes_the_generic_path():
    Ws, bs = cr.mlp_params(2, (65, 64, 64), 1)
    g = np.random.default_rng(1)
    x, ts = g.normal(size=(19, 2)).astype(np.float32), _grid("up", 3)
    G = (0.5 + g.normal(size=(4, 19, 2))).astype(np.float32)
    node, m, traj, got = _hip_grads(Ws, bs, x, G, ts, "midpoint")
    assert node.last_path == "generic" and tuple(traj.shape) == (4, 19, 2)
    assert all(np.all(np.isfinite(q)) for q in got)


def _one_step(scheme, path_off):
    """Parameters after one Adam step on a loss on traj[-1] from fixed weights.  Adam's first step is lr g / (|g| + eps):
    with eps = 1e-3 its slope in g is at most lr / eps = 1, so a gradient error of 1e-5 max|g| moves a parameter by no
    more than that."""
    from cfm_amd import _lib
    dev = torch.device("cuda")
    Ws, bs = cr.mlp_params(2, 64, 5)
    m = cr.make_mlp(Ws, bs, device=dev)
    torch.manual_seed(9)
    x = torch.randn(48, 2, device=dev)
    target = torch.randn(48, 2, device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-3)
    node = cfm_amd.DifferentiableNeuralODE(torch_wrapper(m), solver=scheme)
    lib = _lib.load()
    if path_off:
        lib.cfm_ode_set_fused(0)
    try:
        opt.zero_grad()
        loss = ((node.trajectory(x, torch.linspace(0, 1, 9))[-1] - target) ** 2).mean()
        loss.backward()
    finally:
        lib.cfm_ode_set_fused(1)
    assert node.last_path == ("generic" if path_off else "hip")
    opt.step()
    return [p.detach().cpu().double().numpy() for p in m.parameters()]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_one_adam_step_matches_the_generic_path(scheme):
    want = _one_step(scheme, path_off=True)
    got = _one_step(scheme, path_off=False)
    for a, b in zip(got, want):
        r = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"{scheme} one Adam step: {r:.2e}")
        assert r <= 1e-5
