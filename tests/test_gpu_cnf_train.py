"""GPU: DifferentiableCNF on the HIP path (forward cfm_ode_fixed_cnf_mlp_f32 at Euler, backward cfm_cnf_euler_grad_f32)
against the float64 restatement of tests/cnf_train_restate.py, plus the properties the training loop relies on.

SHAPES are the cases the kernel arrived with (uniform widths, B <= 48, d <= 5, at most 8 steps).  EDGES and STRIDE put
it at the edges of its envelope: non-square hidden layers, d = 63, more tiles than workgroups, the default 101-point
grid of nll, a 2-point grid, and a state that asks for no gradient.  Measured ratios: DESIGN.md 4.9."""
import functools

import numpy as np
import pytest
import torch

import cfm_amd
import cnf_restate as cr
import cnf_train_restate as tr

pytestmark = pytest.mark.gpu

BOUND = 1e-5           # the project's fp32 bound: max|g_hip - g_64| / max|g_64| per gradient tensor
SHAPES = [(2, 64, 48, 8), (5, 48, 19, 5), (1, 16, 33, 3), (2, 64, 37, 8), (2, 64, 1, 4)]      # (d, w, B, steps)


def _grid(direction, steps):
    if direction == "down":
        return np.linspace(1.0, 0.0, steps + 1).astype(np.float32)
    w = 1.0 + 0.6 * np.sin(1.7 * np.arange(steps) + 0.3)          # 0 -> 1, non-uniform
    return np.concatenate([[0.0], np.cumsum(w) / w.sum()]).astype(np.float32)


def _case(d, w, B, steps, hutch, direction, seed=1, g_mean=0.5):
    """fp32 inputs (as float64 for the reference) and the reference gradients.  The rows within 1e-5 of a SELU kink
    somewhere along the float64 trajectory are dropped before anything runs: an fp32 evaluation may take the other
    branch there.  The random upstream gradient has mean g_mean.  With the default 0.5 no gradient tensor is a cancelled
    sum, and the bound (relative to max|g_64| of the tensor) is a scale for every one of them; g_mean = 0 is
    test_zero_mean_upstream_at_d1 below, which says what happens to the one-element db3 then."""
    Ws, bs = cr.mlp_params(d, w, seed)
    g = np.random.default_rng(seed)
    xa = np.concatenate([g.normal(size=(B, 1)) * 0.1, g.normal(size=(B, d))], 1).astype(np.float32)
    G = (g_mean + g.normal(size=(B, d + 1))).astype(np.float32)
    eps = g.normal(size=(B, d)).astype(np.float32) if hutch else None
    ts = _grid(direction, steps)
    keep = tr.kink_free_rows(Ws, bs, xa, ts, eps, tol=1e-5)
    dropped = int((~keep).sum())
    assert dropped <= B / 4, f"{dropped} of {B} rows within 1e-5 of a kink"
    xa, G = xa[keep], G[keep]
    eps = None if eps is None else eps[keep]
    out64, gp64, gx64 = tr.grads_for_upstream(Ws, bs, xa, ts, G, eps)
    return Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped


def _hip_grads(Ws, bs, xa, G, eps, ts, estimator, x_grad=True):
    dev = torch.device("cuda")
    m = cr.make_mlp(Ws, bs, device=dev)
    cnf = cfm_amd.DifferentiableCNF(m, estimator=estimator, noise=None if eps is None else torch.tensor(eps, device=dev))
    x = torch.tensor(xa, device=dev, requires_grad=x_grad)
    out = cnf.solve(x, torch.tensor(ts))
    lins = m._linears()
    ps = [p for l in lins for p in (l.weight, l.bias)]
    g = torch.autograd.grad((out * torch.tensor(G, device=dev)).sum(), ps + ([x] if x_grad else []))
    return cnf, m, out.detach(), [q.detach().cpu().double().numpy() for q in g]


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


NAMES = ["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dx"]


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_w%d_B%d_n%d" % s)
def test_kernel_gradient_against_float64(shape, estimator, direction):
    d, w, B, steps = shape
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped = _case(d, w, B, steps, estimator != "exact", direction)
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, estimator)
    assert cnf.last_path == "hip"
    errs = {n: _rel(a, b) for n, a, b in zip(NAMES, got, gp64 + [gx64])}
    print(f"{shape} {estimator} {direction}: dropped {dropped}; " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.all(np.isfinite(out.cpu().numpy()))
    for k, v in errs.items():
        assert v <= BOUND, (k, v, errs)


ROUNDING = 2.0 ** -24       # one fp32 rounding, relative


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
def test_zero_mean_upstream_at_d1(estimator, direction):
    """The d = 1 case with a ZERO-mean random G.  db3 has one element there, sum_n h_n sum_rows a_{n+1}, and with a
    zero-mean G that sum cancels: on the increasing grid with the exact trace it is 0.0057 while the rows' terms add up
    to 20 in magnitude.  max|g_64| is then no scale for the error: torch's own fp32 autograd through the restatement is
    4.0e-5 of it from float64 on these inputs (computed on the CPU), and the kernel measured 1.3e-5 on the GPU, i.e.
    7e-8 absolute on terms of magnitude 20.  Rule: per tensor, with S = max over its elements of sum_rows |the row's
    contribution in float64|, the error may be the larger of the bound of every other test, 1e-5 max|g_64|, and
    2^-24 S: one fp32 rounding of every row's term, which no fp32 summation order avoids.  The second figure is the
    larger one only where S > 168 max|g_64|; the test asserts that this is never the case for a tensor other than db3,
    so every other tensor is held to 1e-5 as everywhere else."""
    d, w, B, steps = 1, 16, 33, 3
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped = _case(d, w, B, steps, estimator != "exact", direction, g_mean=0.0)
    S = [np.zeros_like(q) for q in gp64]
    for r in range(len(xa)):
        Gr = np.zeros_like(G)
        Gr[r] = G[r]
        for acc, q in zip(S, tr.grads_for_upstream(Ws, bs, xa, ts, Gr, eps)[1]):
            acc += np.abs(q)
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, estimator)
    assert cnf.last_path == "hip"
    for n, a, b, acc in zip(NAMES, got, gp64 + [gx64], S + [None]):
        scale = float(np.abs(b).max())
        err = float(np.abs(a - b).max())
        floor = 0.0 if acc is None else ROUNDING * float(acc.max())
        print(f"d1 zero-mean {estimator} {direction}: {n} err/max|g| {err / scale:.2e} max|g| {scale:.3e} "
              f"2^-24 S {floor:.2e} = {floor / scale:.2e} max|g|")
        if n != "db3":
            assert floor <= BOUND * scale, (n, floor, scale)
        assert err <= max(BOUND * scale, floor), (n, err, scale, floor)


# ---- the edges of the envelope --------------------------------------------------------------------------------------
CG_MAXGRID = 256          # csrc/cnf_grad.h: workgroups (= partial gradients) at most
W64, W33, WMIX, WMIX2 = (64, 64, 64), (33, 33, 33), (64, 17, 40), (33, 64, 48)

# (d, hidden widths, B = rows KEPT after the kink drop, steps)
EDGES = [
    (2, WMIX, 48, 8),               # non-square layers, three full tiles
    (5, WMIX2, 37, 5),              # non-square layers, partial tile
    (1, WMIX, 100, 4),              # non-square layers, d = 1
    (63, W64, 40, 3),               # 63 directions, the time in column 63 of W0
    (63, W33, 17, 3),               # 63 directions, partial widths, partial tile
    (2, W64, 48, 100),              # the default steps of nll: n_t = 101, t_span takes 512 bytes of the workspace
    (2, W64, 40, 1),                # n_t = 2
]
# the grid stride takes a second pass, 256 partials are added, the last tile is partial; with the direction each runs in
STRIDE = [
    ((2, W64, 16 * CG_MAXGRID + 5, 4), "down"),
    ((2, WMIX, 16 * CG_MAXGRID + 5, 3), "up"),
]


def _sid(s):
    return "d%d_w%s_B%d_n%d" % (s[0], "-".join(map(str, s[1])), s[2], s[3])


def _drawn(B, steps):
    """Rows drawn for B kept rows, and the share of them that may go.  A quarter at most; the 100-step case is the
    exception: a trajectory of 100 points passes 100 times as many pre-activations, the reference alone drops about a
    third of the drawn rows there (26 to 40 of 96 over seeds 1 to 12), so 96 are drawn and at most 40 % may go."""
    return (2 * B, 0.40) if steps == 100 else (B + B // 16 + 2, 0.25)


# every case runs on seed 1 but the 100-step one: of seeds 1 to 12, seed 7 leaves the widest margin under its cap on the
# reference alone (27 of 96 drawn rows go on the decreasing grid, 31 on the increasing one; seed 1: 33 and 38)
SEEDS = {(2, W64, 48, 100): 7}


@functools.lru_cache(maxsize=None)
def _edge(shape, hutch, direction):
    """_case with B the number of rows KEPT: more rows are drawn, the kinked ones dropped, the first B kept.  The
    float64 reference is computed once per (shape, estimator, direction), shared and never written to.  Above
    16 CG_MAXGRID rows also S: per parameter tensor the sum over the rows of |the row's float64 contribution|
    (DESIGN.md 4.9)."""
    d, w, B, steps = shape
    seed = SEEDS.get(shape, 1)
    n, cap = _drawn(B, steps)
    Ws, bs = cr.mlp_params(d, w, seed)
    g = np.random.default_rng(seed)
    xa = np.concatenate([g.normal(size=(n, 1)) * 0.1, g.normal(size=(n, d))], 1).astype(np.float32)
    G = (0.5 + g.normal(size=(n, d + 1))).astype(np.float32)
    eps = g.normal(size=(n, d)).astype(np.float32) if hutch else None
    ts = _grid(direction, steps)
    keep = tr.kink_free_rows(Ws, bs, xa, ts, eps, tol=1e-5)
    dropped = int((~keep).sum())
    assert dropped <= cap * n, f"{dropped} of {n} drawn rows within 1e-5 of a kink"
    xa, G = xa[keep][:B], G[keep][:B]
    eps = None if eps is None else eps[keep][:B]
    assert len(xa) == B, (len(xa), B)
    out64, gp64, gx64 = tr.grads_for_upstream(Ws, bs, xa, ts, G, eps)
    S = _row_sums(Ws, bs, xa, ts, G, eps) if B > 16 * CG_MAXGRID else None
    for a in (xa, G, ts, out64, gx64, *gp64, *Ws, *bs, *(S or ()), *(() if eps is None else (eps,))):
        a.setflags(write=False)
    return Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped, S


def _row_sums(Ws, bs, xa, ts, G, eps, chunk=512):
    """Per parameter tensor: sum over the rows of |d/dtheta of the row's term of sum(G * solve)| in float64, by per-row
    gradients under torch.func.vmap in chunks of rows (the loop of test_zero_mean_upstream_at_d1, vectorised)."""
    params = tuple(tr.as_params(Ws, bs, requires_grad=False))
    X, Gt = torch.tensor(np.asarray(xa, np.float64)), torch.tensor(np.asarray(G, np.float64))
    E = None if eps is None else torch.tensor(np.asarray(eps, np.float64))

    def row_term(ps, x, g, e):
        out = tr.euler_solve(list(ps), x[None], ts, None if e is None else e[None])
        return (out[0] * g).sum()

    per_row = torch.func.vmap(torch.func.grad(row_term), in_dims=(None, 0, 0, None if E is None else 0))
    S = [np.zeros(tuple(p.shape)) for p in params]
    for a in range(0, len(X), chunk):
        gs = per_row(params, X[a:a + chunk], Gt[a:a + chunk], None if E is None else E[a:a + chunk])
        for acc, q in zip(S, gs):
            acc += q.abs().sum(0).numpy()
    return S


def _report(tag, got, gp64, gx64, S=None):
    """Every ratio is printed before anything is asserted.  Per tensor err <= BOUND max|g_64|; with S (the cases that add
    256 partials of 16 rows each) the larger of that and 2^-24 S, the rule of test_zero_mean_upstream_at_d1."""
    bad, line = [], []
    for n, a, b, acc in zip(NAMES, got, gp64 + [gx64], (S or [None] * 8) + [None]):
        scale, err = float(np.abs(b).max()), float(np.abs(a - b).max())
        floor = 0.0 if acc is None else ROUNDING * float(acc.max())
        line.append(f"{n} {err / scale:.2e}" + ("" if acc is None else f" (2^-24 S = {floor / scale:.1e})"))
        if not np.all(np.isfinite(a)) or err > max(BOUND * scale, floor):
            bad.append((n, err / scale, floor / scale))
    print(f"{tag}: " + " ".join(line))
    assert not bad, bad


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
@pytest.mark.parametrize("shape", EDGES, ids=_sid)
def test_edge_gradient_against_float64(shape, estimator, direction):
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped, _ = _edge(shape, estimator != "exact", direction)
    assert len(xa) == shape[2] and len(ts) == shape[3] + 1
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, estimator)
    assert cnf.last_path == "hip"
    assert np.all(np.isfinite(out.cpu().numpy()))
    _report(f"{_sid(shape)} {estimator} {direction}: dropped {dropped}", got, gp64, gx64)


@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
@pytest.mark.parametrize("shape,direction", STRIDE, ids=[_sid(s) + "_" + k for s, k in STRIDE])
def test_grid_stride_gradient_against_float64(shape, direction, estimator):
    """More tiles than workgroups: every workgroup's accumulators live through a second tile, and the reduction adds
    CG_MAXGRID partials.  A tensor's error may be the larger of BOUND max|g_64| and 2^-24 S."""
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped, S = _edge(shape, estimator != "exact", direction)
    assert -(-len(xa) // 16) > CG_MAXGRID and len(xa) % 16 != 0
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, estimator)
    assert cnf.last_path == "hip"
    assert np.all(np.isfinite(out.cpu().numpy()))
    _report(f"{_sid(shape)} {estimator} {direction}: dropped {dropped}", got, gp64, gx64, S)


@pytest.mark.parametrize("shape,estimator,direction", [(EDGES[1], "hutch_gaussian", "up"), (STRIDE[1][0], "exact", "up"),
                                                       (STRIDE[0][0], "hutch_gaussian", "down")],
                         ids=lambda v: _sid(v) if isinstance(v, tuple) else v)
def test_edge_forward_value_is_the_sampler_s_bit_for_bit(shape, estimator, direction):
    from cfm_amd.ode import NeuralODE
    dev = torch.device("cuda")
    Ws, bs, xa, G, eps, ts, out64, *_ = _edge(shape, estimator != "exact", direction)
    m = cr.make_mlp(Ws, bs, device=dev)
    e = None if eps is None else torch.tensor(eps, device=dev)
    cnf = cfm_amd.DifferentiableCNF(m, estimator=estimator, noise=e)
    out = cnf.solve(torch.tensor(xa, device=dev), torch.tensor(ts))
    node = NeuralODE(cfm_amd.CNF(m, estimator=estimator, noise=e), solver="euler")
    want = node.trajectory(torch.tensor(xa, device=dev), torch.tensor(ts))[-1]
    assert cnf.last_path == "hip" and node.last_path == "hip"
    assert torch.equal(out.detach(), want)
    assert _rel(out.detach().cpu().double().numpy()[:, 1:], out64[:, 1:]) <= BOUND      # and it is the solve


@pytest.mark.parametrize("shape,direction", STRIDE, ids=[_sid(s) + "_" + k for s, k in STRIDE])
def test_two_backward_calls_give_the_same_bits_on_the_grid_stride(shape, direction):
    """The partials are added in workgroup order: 256 of them, each the sum of two tiles' rows."""
    Ws, bs, xa, G, eps, ts, *_ = _edge(shape, True, direction)
    a = _hip_grads(Ws, bs, xa, G, eps, ts, "hutch_gaussian")[3]
    b = _hip_grads(Ws, bs, xa, G, eps, ts, "hutch_gaussian")[3]
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("shape,estimator", [(EDGES[0], "exact"), (EDGES[1], "hutch_gaussian")],
                         ids=lambda v: _sid(v) if isinstance(v, tuple) else v)
def test_state_without_requires_grad_gets_no_dx_and_the_same_parameter_gradients(shape, estimator, monkeypatch):
    """x_aug that asks for no gradient: the kernel is called with g_initial == NULL (observed at the C entry: no buffer
    for dx exists, so none is returned), and the eight parameter gradients are those of the call with it, bit for bit."""
    from cfm_amd import _lib
    lib = _lib.load()
    entry = lib.cfm_cnf_euler_grad_f32
    g_initial = []

    def spy(*args):
        g_initial.append(args[13].value)          # a c_void_p: None is NULL
        return entry(*args)
    monkeypatch.setattr(lib, "cfm_cnf_euler_grad_f32", spy)
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, _, _ = _edge(shape, estimator != "exact", "down")
    with_x = _hip_grads(Ws, bs, xa, G, eps, ts, estimator)
    without = _hip_grads(Ws, bs, xa, G, eps, ts, estimator, x_grad=False)
    assert with_x[0].last_path == without[0].last_path == "hip"
    assert len(g_initial) == 2 and g_initial[0] is not None and g_initial[1] is None
    assert len(with_x[3]) == 9 and len(without[3]) == 8
    for p, q in zip(with_x[3], without[3]):
        assert np.array_equal(p, q)
    _report(f"{_sid(shape)} {estimator} no dx", without[3] + [with_x[3][8]], gp64, gx64)


def test_fused_path_off_runs_generic_and_agrees_at_mixed_widths():
    from cfm_amd import _lib
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, _, _ = _edge(EDGES[1], False, "up")
    hip = _hip_grads(Ws, bs, xa, G, eps, ts, "exact")
    assert hip[0].last_path == "hip"
    lib = _lib.load()
    lib.cfm_ode_set_fused(0)
    try:
        gen = _hip_grads(Ws, bs, xa, G, eps, ts, "exact")
    finally:
        lib.cfm_ode_set_fused(1)
    assert gen[0].last_path == "generic"
    for n, a, b, ref in zip(NAMES, hip[3], gen[3], gp64 + [gx64]):
        r = float(np.abs(a - b).max() / np.abs(ref).max())
        print(f"mixed widths, hip vs generic: {n} {r:.2e}")
        assert r <= BOUND, n


@pytest.mark.parametrize("estimator", ["exact", "hutch_rademacher"])
def test_forward_value_is_the_sampler_s_bit_for_bit(estimator):
    from cfm_amd.ode import NeuralODE
    dev = torch.device("cuda")
    Ws, bs = cr.mlp_params(2, 64, 2)
    m = cr.make_mlp(Ws, bs, device=dev)
    torch.manual_seed(4)
    x = torch.randn(37, 3, device=dev)
    e = None if estimator == "exact" else (torch.randint(0, 2, (37, 2), device=dev).float() * 2 - 1)
    ts = torch.linspace(1, 0, 9)
    cnf = cfm_amd.DifferentiableCNF(m, estimator=estimator, noise=e)
    out = cnf.solve(x, ts)
    node = NeuralODE(cfm_amd.CNF(m, estimator=estimator, noise=e), solver="euler")
    want = node.trajectory(x, ts)[-1]
    assert cnf.last_path == "hip" and node.last_path == "hip"
    assert torch.equal(out.detach(), want)


def test_two_backward_calls_give_the_same_bits():
    Ws, bs, xa, G, eps, ts, *_ = _case(2, 64, 37, 8, True, "down")
    a = _hip_grads(Ws, bs, xa, G, eps, ts, "hutch_gaussian")[3]
    b = _hip_grads(Ws, bs, xa, G, eps, ts, "hutch_gaussian")[3]
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


def test_fused_path_off_runs_generic_and_agrees():
    from cfm_amd import _lib
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, _ = _case(2, 64, 37, 8, False, "down")
    hip = _hip_grads(Ws, bs, xa, G, eps, ts, "exact")
    assert hip[0].last_path == "hip"
    lib = _lib.load()
    lib.cfm_ode_set_fused(0)
    try:
        gen = _hip_grads(Ws, bs, xa, G, eps, ts, "exact")
    finally:
        lib.cfm_ode_set_fused(1)
    assert gen[0].last_path == "generic"
    for n, a, b, ref in zip(NAMES, hip[3], gen[3], gp64 + [gx64]):
        assert float(np.abs(a - b).max() / np.abs(ref).max()) <= BOUND, n


def _one_step(make_opt, path_off):
    """Parameters after one optimiser step on the NLL from fixed weights.  Adam's first step is lr g / (|g| + eps): with
    eps = 1e-3 its slope in g is at most lr / eps = 1, so a gradient error of 1e-5 max|g| moves a parameter by no more
    than that (with the default eps = 1e-8 the step is sign(g) and any element near zero would flip it)."""
    from cfm_amd import _lib
    dev = torch.device("cuda")
    Ws, bs = cr.mlp_params(2, 64, 5)
    m = cr.make_mlp(Ws, bs, device=dev)
    torch.manual_seed(9)
    x = torch.randn(48, 2, device=dev)
    opt = make_opt(m.parameters())
    cnf = cfm_amd.DifferentiableCNF(m)
    lib = _lib.load()
    if path_off:
        lib.cfm_ode_set_fused(0)
    try:
        opt.zero_grad()
        loss = cnf.nll(x, steps=8)
        loss.backward()
    finally:
        lib.cfm_ode_set_fused(1)
    assert cnf.last_path == ("generic" if path_off else "hip")
    opt.step()
    return [p.detach().cpu().double().numpy() for p in m.parameters()]


@pytest.mark.parametrize("which", ["adam", "fused_adam"])
def test_one_optimiser_step_matches_the_generic_path(which):
    kw = dict(lr=1e-3, eps=1e-3)
    mk = (lambda ps: torch.optim.Adam(ps, **kw)) if which == "adam" else (lambda ps: cfm_amd.FusedAdam(ps, **kw))
    want = _one_step(lambda ps: torch.optim.Adam(ps, **kw), path_off=True)
    got = _one_step(mk, path_off=False)
    for a, b in zip(got, want):
        assert float(np.abs(a - b).max() / np.abs(b).max()) <= 1e-5


def test_twenty_steps_of_the_tutorial_loop_lower_the_loss():
    from cfm_amd.utils import sample_moons
    dev = torch.device("cuda")
    torch.manual_seed(0)
    np.random.seed(0)
    m = cfm_amd.MLP(dim=2, time_varying=True).to(dev)
    cnf = cfm_amd.DifferentiableCNF(m)
    opt = torch.optim.Adam(m.parameters())
    held = sample_moons(64).to(dev)
    with torch.no_grad():
        before = float(cnf.nll(held, steps=8))
    for _ in range(20):
        opt.zero_grad()
        loss = cnf.nll(sample_moons(64).to(dev), steps=8)
        loss.backward()
        opt.step()
        assert cnf.last_path == "hip"
    with torch.no_grad():
        after = float(cnf.nll(held, steps=8))
    print(f"held-out NLL {before:.4f} -> {after:.4f}")
    assert np.isfinite(after) and after < before
