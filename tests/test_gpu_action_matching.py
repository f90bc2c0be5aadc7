"""GPU (-m gpu): cfm_amd.action_matching_loss on the HIP path (cfm_action_matching_grad_f32, csrc/action_grad.h) against the
float64 restatement of tests/action_matching_restate.py, plus the properties a training loop relies on.

Kink rule: rows of which any float64 pre-activation, at any of the three evaluation points, comes
within 1e-5 of a SELU kink are dropped from x0, x1, t and xt together before anything runs; a case FAILS when more than
5 % of its drawn rows go.  Every case's seed was picked by a CPU search for one inside that cap and is committed here.

Tolerance: per gradient tensor max|g_hip - g_64| <= max(1e-5 max|g_64|, 2^-24 S), S the largest sum over
the rows of |a row's float64 contribution| to one element; loss: |L - L_64| <= 1e-5 mean_rows(|s(x0, 0)| + |s(x1, 1)| +
1/2 |g_x|^2 + |g_t|); db3 is an exact 0.

Measured on an MI355X (err / max|g_64| per tensor, worst case over CASES): see DESIGN.md 4.11."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import action_matching_restate as R

pytestmark = pytest.mark.gpu

BOUND = 1e-5
ROUNDING = 2.0 ** -24
CG_MAXGRID = 256          # csrc/cnf_grad.h: workgroups (= partial gradients) at most
W64, W33, WMIX = R.WIDTHS

# (B, d, widths, seed, kind): kind "ends" puts rows at t = 0 and t = 1 exactly, "xt" passes an xt off the interpolant,
# "default" lets action_matching_loss interpolate
CASES = [
    (1, 2, W64, 1, "plain"),
    (16, 2, W64, 1, "plain"),
    (17, 5, W33, 1, "plain"),                      # a partial tile; no row may go at this size
    (40, 2, W64, 1, "plain"),
    (16 * CG_MAXGRID + 5, 2, W64, 1, "plain"),     # the grid stride takes a second pass, the last tile is partial
    (100, 1, WMIX, 1, "plain"),
    (40, 63, W64, 1, "plain"),                     # d + 1 = 64: the time sits in the last column of the tile
    (17, 63, W33, 1, "plain"),
    (40, 5, WMIX, 1, "plain"),
    (40, 2, W64, 1, "ends"),
    (40, 2, W64, 1, "xt"),
    (40, 2, W64, 1, "default"),
]
IDS = ["B%d_d%d_w%s_%s" % (B, d, "-".join(map(str, w)), kind) for B, d, w, _, kind in CASES]


@functools.lru_cache(maxsize=None)
def _case(B, d, widths, seed, kind):
    """fp32 inputs with the kinked rows dropped, and the float64 reference (computed once, shared, never written to)."""
    Ws, bs = R.action_params(d, widths, seed)
    n = B + B // 16 + 2                                     # drawn rows: B are kept after the drop
    x0, x1, t, xt = R.draw(n, d, seed + 100, ends=kind == "ends")
    if kind == "xt":
        xt = (xt + 0.3 * np.random.default_rng(seed + 7).normal(size=xt.shape)).astype(np.float32)
    keep = R.kink_free(Ws, bs, x0, x1, xt, t, tol=1e-5)
    dropped = int((~keep).sum())
    assert dropped <= 0.05 * n, f"{dropped} of {n} rows within 1e-5 of a kink"
    if kind == "ends":
        assert keep[0] and keep[1]
    x0, x1, t, xt = (v[keep][:B] for v in (x0, x1, t, xt))
    assert len(x0) == B
    if kind == "ends":
        assert t[0] == 0.0 and t[1] == 1.0
    ref = R.sweeps(Ws, bs, x0, x1, xt, t, scales=True)
    for a in (x0, x1, t, xt, *ref[1], *ref[3]):
        a.setflags(write=False)
    return Ws, bs, x0, x1, t, xt, ref, dropped


def _params(m):
    return [p for l in m._linears() for p in (l.weight, l.bias)]


def _run(m, x0, x1, t, xt, dev, dtype=torch.float32):
    """loss and the eight gradients of one action_matching_loss call, as float64 numpy; the path that ran"""
    import cfm_amd
    T = lambda v: None if v is None else torch.tensor(np.asarray(v), device=dev, dtype=dtype)   # noqa: E731
    loss = cfm_amd.action_matching_loss(m, T(x0), T(x1), T(t), xt=T(xt))
    path = cfm_amd.action_matching_loss.last_path
    gs = torch.autograd.grad(loss, _params(m), allow_unused=True)
    return float(loss.detach()), [None if g is None else g.detach().cpu().double().numpy() for g in gs], path


def _check(tag, loss, grads, ref, strict=False):
    """The tolerance of the module docstring (strict: 1e-5 max|g_64| alone); prints every figure before it asserts."""
    l64, g64, lscale, S = ref
    lerr = abs(loss - l64)
    line = [f"loss err/scale {lerr / lscale:.2e}"]
    bad = []
    if lerr > BOUND * lscale:
        bad.append(("loss", lerr, lscale))
    for n, a, b, s in zip(R.NAMES[:7], grads, g64, S):
        scale, err, floor = float(np.abs(b).max()), float(np.abs(a - b).max()), ROUNDING * float(s.max())
        line.append(f"{n} {err / scale:.2e} (2^-24 S = {floor / scale:.1e})")
        if err > (BOUND * scale if strict else max(BOUND * scale, floor)):
            bad.append((n, err, scale, floor))
    print(f"{tag}: " + " ".join(line))
    assert not bad, bad


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loss_and_gradient_against_float64(case):
    Ws, bs, x0, x1, t, xt, ref, dropped = _case(*case)
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    loss, grads, path = _run(m, x0, x1, t, None if case[4] == "default" else xt, dev)
    assert path == "hip"
    assert grads[7].shape == (1,) and grads[7][0] == 0.0 and not np.signbit(grads[7][0])
    assert all(np.all(np.isfinite(g)) for g in grads) and np.isfinite(loss)
    _check(f"{IDS[CASES.index(case)]} dropped {dropped}", loss, grads, ref)


def test_default_xt_is_the_interpolant_bit_for_bit():
    Ws, bs, x0, x1, t, xt, ref, _ = _case(40, 2, W64, 1, "default")
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    a = _run(m, x0, x1, t, None, dev)
    b = _run(m, x0, x1, t, xt, dev)
    assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))


@pytest.mark.parametrize("case", [CASES[3], CASES[4]], ids=[IDS[3], IDS[4]])
def test_two_calls_give_the_same_bits(case):
    Ws, bs, x0, x1, t, xt, ref, _ = _case(*case)
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    a = _run(m, x0, x1, t, xt, dev)
    b = _run(m, x0, x1, t, xt, dev)
    assert a[2] == b[2] == "hip"
    assert a[0] == b[0]
    for p, q in zip(a[1], b[1]):
        assert np.array_equal(p, q)


def test_backward_fills_accumulates_and_scales():
    import cfm_amd
    Ws, bs, x0, x1, t, xt, ref, _ = _case(40, 2, W64, 1, "plain")
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    T = lambda v: torch.tensor(v, device=dev)   # noqa: E731
    args = (T(x0), T(x1), T(t))
    ps = list(m.parameters())
    assert len(ps) == 8
    cfm_amd.action_matching_loss(m, *args, xt=T(xt)).backward()
    assert cfm_amd.action_matching_loss.last_path == "hip"
    once = [p.grad.detach().clone() for p in ps]
    assert all(g is not None and g.shape == p.shape for g, p in zip(once, ps))
    cfm_amd.action_matching_loss(m, *args, xt=T(xt)).backward()
    for p, g in zip(ps, once):
        assert torch.equal(p.grad, g + g)
    for p in ps:
        p.grad = None
    (3 * cfm_amd.action_matching_loss(m, *args, xt=T(xt))).backward()
    for p, g in zip(ps, once):
        assert torch.equal(p.grad, 3 * g)


def test_gradmodel_and_mlp_give_the_same_bits():
    from cfm_amd.models import GradModel
    Ws, bs, x0, x1, t, xt, ref, _ = _case(17, 5, W33, 1, "plain")
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    a = _run(m, x0, x1, t, xt, dev)
    gm = GradModel(m)
    import cfm_amd
    T = lambda v: torch.tensor(v, device=dev)   # noqa: E731
    loss = cfm_amd.action_matching_loss(gm, T(x0), T(x1), T(t), xt=T(xt))
    assert cfm_amd.action_matching_loss.last_path == "hip"
    gs = torch.autograd.grad(loss, _params(m))
    assert float(loss.detach()) == a[0]
    for p, q in zip(a[1], gs):
        assert np.array_equal(p, q.cpu().double().numpy())


def test_a_double_backward_of_the_hip_path_raises():
    import cfm_amd
    Ws, bs, x0, x1, t, xt, ref, _ = _case(16, 2, W64, 1, "plain")
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    T = lambda v: torch.tensor(v, device=dev)   # noqa: E731
    loss = cfm_amd.action_matching_loss(m, T(x0), T(x1), T(t), xt=T(xt))
    assert cfm_amd.action_matching_loss.last_path == "hip"
    gs = torch.autograd.grad(loss, _params(m), create_graph=True)
    with pytest.raises(RuntimeError):
        gs[0].sum().backward()


# ---- dispatch -----------------------------------------------------------------------------------------------------
def test_a_wide_net_takes_the_generic_path():
    Ws, bs, x0, x1, t, xt, ref, _ = _case(40, 2, (128, 128, 128), 1, "plain")
    dev = torch.device("cuda")
    loss, grads, path = _run(R.make_action(Ws, bs, device=dev), x0, x1, t, xt, dev)
    assert path == "generic"
    assert grads[7] is None or not np.any(grads[7])
    _check("w128 generic", loss, grads, ref, strict=True)


def test_float64_inputs_take_the_generic_path():
    Ws, bs, x0, x1, t, xt, ref, _ = _case(40, 2, W64, 1, "plain")
    dev = torch.device("cuda")
    loss, grads, path = _run(R.make_action(Ws, bs, device=dev), x0, x1, t, xt, dev, dtype=torch.float64)
    assert path == "generic"
    _check("float64 generic", loss, grads, ref, strict=True)


def test_the_fused_path_switched_off_takes_the_generic_path():
    from cfm_amd import _lib
    Ws, bs, x0, x1, t, xt, ref, _ = _case(40, 2, W64, 1, "plain")
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    lib = _lib.load()
    lib.cfm_ode_set_fused(0)
    try:
        loss, grads, path = _run(m, x0, x1, t, xt, dev)
    finally:
        lib.cfm_ode_set_fused(1)
    assert path == "generic"
    _check("fused off generic", loss, grads, ref, strict=True)
    assert _run(m, x0, x1, t, xt, dev)[2] == "hip"


def test_the_c_entry_refuses_what_is_outside_the_envelope():
    from cfm_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    B = 16
    z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731

    def call(dims, n_layers=4, B=B):
        Ws = [z(dims[l + 1], dims[l]) for l in range(4)]
        bs = [z(dims[l + 1]) for l in range(4)]
        dW = [torch.empty_like(w) for w in Ws]
        db = [torch.empty_like(b) for b in bs]
        arr = lambda ts: (ctypes.c_void_p * 4)(*[v.data_ptr() for v in ts])   # noqa: E731
        d = dims[0] - 1
        x = z(max(B, 1), max(d, 1))
        tt = z(max(B, 1))
        loss = z(1)
        ws = _lib.workspace(_lib.OP_ACTION_GRAD, max(B, 1), 0, 0, dev)
        return lib.cfm_action_matching_grad_f32(arr(Ws), arr(bs), (ctypes.c_int * 5)(*dims), n_layers, _lib.ptr(x), _lib.ptr(x),
                                                _lib.ptr(x), _lib.ptr(tt), B, _lib.ptr(loss), arr(dW), arr(db), _lib.ptr(ws),
                                                _lib.stream_ptr())
    assert call([3, 64, 64, 64, 1]) == 0
    assert call([3, 65, 64, 64, 1]) == -1          # a width above 64
    assert call([3, 64, 64, 65, 1]) == -1
    assert call([65, 64, 64, 64, 1]) == -1         # d + 1 > 64
    assert call([3, 64, 64, 64, 2]) == -1          # not a scalar action
    assert call([1, 64, 64, 64, 1]) == -1          # d = 0
    assert call([3, 64, 64, 64, 1], n_layers=3) == -1
    assert call([3, 64, 64, 64, 1], B=0) == -1
    assert lib.cfm_workspace_bytes(_lib.OP_ACTION_GRAD, 0, 0, 0) == 0
    torch.cuda.synchronize()


# ---- the training loop --------------------------------------------------------------------------------------------
def _one_step(make_opt, path_off):
    """Parameters after one optimiser step from fixed weights.  Adam's first step is lr g / (|g| + eps): with eps = 1e-3
    its slope in g is at most lr / eps = 1, so a gradient error of 1e-5 max|g| moves a parameter by no more than that
    (with the default eps = 1e-8 the step is sign(g) and any element near zero would flip it)."""
    import cfm_amd
    from cfm_amd import _lib
    Ws, bs, x0, x1, t, xt, ref, _ = _case(40, 2, W64, 1, "plain")
    dev = torch.device("cuda")
    m = R.make_action(Ws, bs, device=dev)
    T = lambda v: torch.tensor(v, device=dev)   # noqa: E731
    opt = make_opt(m.parameters())
    lib = _lib.load()
    if path_off:
        lib.cfm_ode_set_fused(0)
    try:
        opt.zero_grad()
        cfm_amd.action_matching_loss(m, T(x0), T(x1), T(t), xt=T(xt)).backward()
    finally:
        lib.cfm_ode_set_fused(1)
    assert cfm_amd.action_matching_loss.last_path == ("generic" if path_off else "hip")
    opt.step()
    return [p.detach().cpu().double().numpy() for p in m.parameters()]


@pytest.mark.parametrize("which", ["adam", "fused_adam"])
def test_one_optimiser_step_matches_the_generic_path(which):
    import cfm_amd
    kw = dict(lr=1e-3, eps=1e-3)
    mk = (lambda ps: torch.optim.Adam(ps, **kw)) if which == "adam" else (lambda ps: cfm_amd.FusedAdam(ps, **kw))
    want = _one_step(lambda ps: torch.optim.Adam(ps, **kw), path_off=True)
    got = _one_step(mk, path_off=False)
    for a, b in zip(got, want):
        assert float(np.abs(a - b).max() / np.abs(b).max()) <= 1e-5


def test_the_feature_is_exported():
    """Fails on the parent commit: neither the function nor the ABI symbol exists there."""
    from cfm_amd import action_matching_loss, _lib
    assert callable(action_matching_loss)
    lib = _lib.load()
    assert hasattr(lib, "cfm_action_matching_grad_f32") and "cfm_action_matching_grad_f32" in _lib.SIGNATURES
    n = lib.cfm_workspace_bytes(_lib.OP_ACTION_GRAD, 256, 0, 0)
    assert n > 0 and n % 256 == 0
