"""GPU: RegularizedCNF on the HIP path (forward cfm_ode_euler_cnf_reg_mlp_f32, backward cfm_cnf_reg_euler_grad_f32)
against the float64 restatement of tests/cnf_reg_restate.py, on the conventions of test_gpu_cnf_train.py: cr.mlp_params,
the two grids (`down` uniform, `up` non-uniform), a random upstream G of mean 0.5 on all columns, seed 1.

Rows within 1e-5 of a SELU kink along the float64 trajectory are dropped before anything runs, and so are rows where
||J||_F / d < 1e-5 anywhere along it (f has a kink of its own at J = 0): B + B/16 + 2 rows are drawn, at most a quarter
may go, the first B kept.  Bound: max|g_hip - g_64| <= 1e-5 max|g_64| per gradient tensor; at 4101 rows (256 partials of
16-row tiles) the larger of that and 2^-24 S, the rule of test_gpu_cnf_train.test_zero_mean_upstream_at_d1.
Measured ratios: DESIGN.md 4.13."""
import functools

import numpy as np
import pytest
import torch

import cfm_amd
import cnf_reg_restate as rr
import cnf_restate as cr
import cnf_train_restate as tr

pytestmark = pytest.mark.gpu

BOUND = 1e-5
ROUNDING = 2.0 ** -24
CG_MAXGRID = 256
W64, W33, WMIX, WMIX2 = (64, 64, 64), (33, 33, 33), (64, 17, 40), (33, 64, 48)
COEFFS = {1: (0.3, 0.0), 2: (0.0, 0.7), 3: (0.3, 0.7)}         # reg_mask -> (squared_l2_reg, jacobian_frobenius_reg)
NAMES = ["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dx"]

# (d, hidden widths, B kept, steps)
CASES = [
    (2, 64, 48, 8),                 # three full tiles
    (5, 48, 19, 5),                 # partial tile, width below 64
    (1, 16, 33, 3),                 # d = 1: S is one entry squared
    (2, 64, 1, 4),                  # one row
    (5, WMIX2, 37, 5),              # non-square layers, partial tile
    (1, WMIX, 100, 4),              # smallest ||J||_F, non-square layers
    (2, W64, 40, 1),                # n_t = 2
]
CASES_D63 = [(63, W64, 40, 3), (63, W33, 17, 3)]       # 63 directions; time in column 63; partial everything
STRIDE = (2, W64, 16 * CG_MAXGRID + 5, 4)              # second grid-stride pass, 256 partials, partial last tile


def _sid(s):
    w = s[1] if isinstance(s[1], tuple) else (s[1],)
    return "d%d_w%s_B%d_n%d" % (s[0], "-".join(map(str, w)), s[2], s[3])


def _grids(direction, steps):
    if direction == "down":
        return np.linspace(1.0, 0.0, steps + 1).astype(np.float32)
    w = 1.0 + 0.6 * np.sin(1.7 * np.arange(steps) + 0.3)
    return np.concatenate([[0.0], np.cumsum(w) / w.sum()]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(shape, mask, hutch, direction, g_zero_reg=False):
    """fp32 inputs and the float64 reference, computed once per case, shared and never written to."""
    d, w, B, steps = shape
    r = rr.n_reg(mask)
    n = B + B // 16 + 2
    Ws, bs = cr.mlp_params(d, w, 1)
    g = np.random.default_rng(1)
    # l, y, their upstream columns and the probe are drawn first, in the order of test_gpu_cnf_train._edge, so the rows
    # (and the ones dropped) are the same under every mask; the penalty columns and their upstream follow
    la, ya, Gly = g.normal(size=(n, 1)) * 0.1, g.normal(size=(n, d)), 0.5 + g.normal(size=(n, d + 1))
    eps = g.normal(size=(n, d)).astype(np.float32) if hutch else None
    ra, Gr = g.normal(size=(n, r)) * 0.1, 0.5 + g.normal(size=(n, r))
    if g_zero_reg:
        Gr[:] = 0.0
    xa = np.concatenate([la, ra, ya], 1).astype(np.float32)
    G = np.concatenate([Gly[:, :1], Gr, Gly[:, 1:]], 1).astype(np.float32)
    ts = _grids(direction, steps)
    keep, fmin = rr.usable_rows(Ws, bs, xa, ts, mask, eps, tol=1e-5)
    dropped = int((~keep).sum())
    assert dropped <= n / 4, f"{dropped} of {n} drawn rows within 1e-5 of a kink"
    xa, G = xa[keep][:B], G[keep][:B]
    eps = None if eps is None else eps[keep][:B]
    assert len(xa) == B, (len(xa), B)
    out64, gp64, gx64 = rr.grads_for_upstream(Ws, bs, xa, ts, G, mask, eps)
    S = _row_sums(Ws, bs, xa, ts, G, mask) if B > 16 * CG_MAXGRID else None
    for a in (xa, G, ts, out64, gx64, *gp64, *Ws, *bs, *(S or ()), *(() if eps is None else (eps,))):
        a.setflags(write=False)
    return Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped, fmin, S


def _row_sums(Ws, bs, xa, ts, G, mask, chunk=512):
    """Per parameter tensor: sum over the rows of |the row's float64 contribution| (test_gpu_cnf_train._row_sums)."""
    params = tuple(tr.as_params(Ws, bs, requires_grad=False))
    X, Gt = torch.tensor(np.asarray(xa, np.float64)), torch.tensor(np.asarray(G, np.float64))

    def row_term(ps, x, g):
        return (rr.euler_solve(list(ps), x[None], ts, mask)[0] * g).sum()

    per_row = torch.func.vmap(torch.func.grad(row_term), in_dims=(None, 0, 0))
    S = [np.zeros(tuple(p.shape)) for p in params]
    for a in range(0, len(X), chunk):
        for acc, q in zip(S, per_row(params, X[a:a + chunk], Gt[a:a + chunk])):
            acc += q.abs().sum(0).numpy()
    return S


def _make(Ws, bs, mask, eps, dev):
    m = cr.make_mlp(Ws, bs, device=dev)
    e, f = COEFFS[mask]
    cnf = cfm_amd.RegularizedCNF(m, squared_l2_reg=e, jacobian_frobenius_reg=f,
                                 estimator="exact" if eps is None else "hutch_gaussian",
                                 noise=None if eps is None else torch.tensor(eps, device=dev))
    return m, cnf


def _hip_grads(Ws, bs, xa, G, eps, ts, mask, x_grad=True):
    dev = torch.device("cuda")
    m, cnf = _make(Ws, bs, mask, eps, dev)
    x = torch.tensor(xa, device=dev, requires_grad=x_grad)
    out = cnf.solve(x, torch.tensor(ts))
    lins = m._linears()
    ps = [p for l in lins for p in (l.weight, l.bias)]
    g = torch.autograd.grad((out * torch.tensor(G, device=dev)).sum(), ps + ([x] if x_grad else []))
    return cnf, m, out.detach(), [q.detach().cpu().double().numpy() for q in g]


def _report(tag, got, gp64, gx64, S=None):
    """Every ratio is printed before anything is asserted."""
    bad, line = [], []
    for n, a, b, acc in zip(NAMES, got, gp64 + [gx64], (S or [None] * 8) + [None]):
        scale, err = float(np.abs(b).max()), float(np.abs(a - b).max())
        floor = 0.0 if acc is None else ROUNDING * float(acc.max())
        line.append(f"{n} {err / scale:.2e}" + ("" if acc is None else f" (2^-24 S = {floor / scale:.1e})"))
        if not np.all(np.isfinite(a)) or err > max(BOUND * scale, floor):
            bad.append((n, err / scale, floor / scale))
    print(f"{tag}: " + " ".join(line))
    assert not bad, bad


def _check_forward(out, xa, eps, ts, mask, Ws, bs, out64, tag):
    """Columns l and y: the bits of DifferentiableCNF.solve on the same inputs; e and f: within 1e-5 max|column| of float64."""
    dev = torch.device("cuda")
    r = rr.n_reg(mask)
    m = cr.make_mlp(Ws, bs, device=dev)
    plain = cfm_amd.DifferentiableCNF(m, estimator="exact" if eps is None else "hutch_gaussian",
                                      noise=None if eps is None else torch.tensor(eps, device=dev))
    keep = [0] + list(range(1 + r, xa.shape[1]))
    want = plain.solve(torch.tensor(np.ascontiguousarray(xa[:, keep]), device=dev), torch.tensor(ts))
    assert plain.last_path == "hip"
    assert torch.equal(out[:, keep], want.detach()), tag
    got = out.cpu().double().numpy()
    for k in range(1, 1 + r):
        err = float(np.abs(got[:, k] - out64[:, k]).max() / np.abs(out64[:, k]).max())
        print(f"{tag}: column {k} {err:.2e}")
        assert err <= BOUND, (tag, k, err)


def _run(shape, mask, hutch, direction):
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped, fmin, S = _case(shape, mask, hutch, direction)
    assert len(xa) == shape[2] and len(ts) == shape[3] + 1
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, mask)
    assert cnf.last_path == "hip"
    assert np.all(np.isfinite(out.cpu().numpy()))
    tag = f"{_sid(shape)} mask {mask} {'hutch' if hutch else 'exact'} {direction}"
    _check_forward(out, xa, eps, ts, mask, Ws, bs, out64, tag)
    _report(f"{tag}: dropped {dropped}, min |J|_F/d {fmin:.1e}", got, gp64, gx64, S)


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("mask", [1, 2, 3], ids=["e", "f", "ef"])
@pytest.mark.parametrize("shape", CASES, ids=_sid)
def test_gradient_and_forward_against_float64(shape, mask, direction):
    _run(shape, mask, False, direction)


@pytest.mark.parametrize("shape", CASES_D63, ids=_sid)
def test_63_directions(shape):
    _run(shape, 3, False, "down")


def test_grid_stride_and_256_partials():
    assert -(-STRIDE[2] // 16) > CG_MAXGRID and STRIDE[2] % 16 != 0
    _run(STRIDE, 3, False, "down")


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("shape", CASES[:2], ids=_sid)
def test_hutchinson_with_the_kinetic_penalty(shape, direction):
    _run(shape, 1, True, direction)


def test_zero_upstream_on_the_penalty_columns():
    """ce = cf = 0: the penalties' seeds vanish and what is left is the parent's gradient, through the new sweep."""
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, dropped, fmin, S = _case(CASES[0], 3, False, "down", True)
    assert not G[:, 1:3].any()
    cnf, m, out, got = _hip_grads(Ws, bs, xa, G, eps, ts, 3)
    assert cnf.last_path == "hip"
    _report("zero upstream on e and f", got, gp64, gx64)


def test_two_backward_calls_at_4101_rows_give_the_same_bits():
    Ws, bs, xa, G, eps, ts, *_ = _case(STRIDE, 3, False, "down")
    a = _hip_grads(Ws, bs, xa, G, eps, ts, 3)[3]
    b = _hip_grads(Ws, bs, xa, G, eps, ts, 3)[3]
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


def test_state_without_requires_grad_keeps_the_parameter_gradients_bits():
    Ws, bs, xa, G, eps, ts, out64, gp64, gx64, *_ = _case(CASES[1], 3, False, "up")
    with_x = _hip_grads(Ws, bs, xa, G, eps, ts, 3)
    without = _hip_grads(Ws, bs, xa, G, eps, ts, 3, x_grad=False)
    assert with_x[0].last_path == without[0].last_path == "hip"
    assert len(with_x[3]) == 9 and len(without[3]) == 8
    for p, q in zip(with_x[3], without[3]):
        assert np.array_equal(p, q)


def test_loss_on_the_hip_path_is_the_generic_path_s():
    from cfm_amd import _lib
    dev = torch.device("cuda")
    Ws, bs, xa, G, eps, ts, *_ = _case(CASES[0], 3, False, "down")
    x = torch.tensor(np.ascontiguousarray(xa[:, 3:]), device=dev)

    def run(fused):
        m, cnf = _make(Ws, bs, 3, None, dev)
        lib = _lib.load()
        lib.cfm_ode_set_fused(1 if fused else 0)
        try:
            reg, nll = cnf.loss(x, steps=8)
            ps = [p for l in m._linears() for p in (l.weight, l.bias)]
            g = torch.autograd.grad(reg + nll, ps)
        finally:
            lib.cfm_ode_set_fused(1)
        assert cnf.last_path == ("hip" if fused else "generic")
        return float(reg), float(nll), [q.cpu().double().numpy() for q in g]

    hip, gen = run(True), run(False)
    for k in (0, 1):
        print(f"loss[{k}]: hip {hip[k]:.8f} generic {gen[k]:.8f}")
        assert abs(hip[k] - gen[k]) <= BOUND * abs(gen[k])
    for n, a, b in zip(NAMES, hip[2], gen[2]):
        r = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"loss gradient {n}: {r:.2e}")
        assert r <= BOUND, (n, r)


def test_jacobian_penalty_with_a_hutchinson_estimator_goes_generic():
    dev = torch.device("cuda")
    Ws, bs = cr.mlp_params(2, 16, 1)
    m = cr.make_mlp(Ws, bs, device=dev)
    cnf = cfm_amd.RegularizedCNF(m, jacobian_frobenius_reg=0.5, estimator="hutch_rademacher")
    out = cnf.solve(torch.zeros(5, 4, device=dev), torch.tensor([1.0, 0.5, 0.0]))
    assert cnf.last_path == "generic" and out.shape == (5, 4)


# the forward's own stride: cfm_ode_euler_cnf_reg_mlp_f32 is launched on at most 4096 workgroups (the gradient's 256 above)
FWD_BIG = 16 * 4096 + 5
FWD_ROWS = (slice(0, 16), slice(16 * 2051, 16 * 2052), slice(FWD_BIG - 21, FWD_BIG))


def test_second_grid_pass_of_the_forward_solve():
    """B = 16 * 4096 + 5, d = 2, hidden widths (33, 16, 24), both penalties, exact trace, three output times on a non-uniform
    grid (an Euler solve steps exactly its t_span): workgroup 0 of ode_small_euler_reg runs tile 4096 after tile 0, on the
    three tile buffers and the row-sum scratch of its first pass.  Rows of a tile do not interact (the row sums run over
    columns and directions), so the first tile, a middle one and the last full tile with the 5-row tail are bit-equal —
    every column [l, e, f, y] at every output time — to the same rows solved alone; the tail is within 1e-5 max|column| of
    the float64 restatement at every output time."""
    from cfm_amd.cnf import TRACE_EXACT, augmented_euler_hip
    dev = torch.device("cuda")
    d, mask = 2, 3
    Ws, bs = cr.mlp_params(d, (33, 16, 24), 1)
    m = cr.make_mlp(Ws, bs, device=dev)
    x = torch.randn(FWD_BIG, d, generator=torch.Generator().manual_seed(2)).to(dev)
    ts = np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32)
    with torch.no_grad():
        big, nfe = augmented_euler_hip(m, x, torch.tensor(ts), TRACE_EXACT, mask)
        big = big.cpu()
        assert big.shape == (4, FWD_BIG, 3 + d) and nfe == 3 and bool(torch.isfinite(big).all())
        for rows in FWD_ROWS:
            alone = augmented_euler_hip(m, x[rows].contiguous(), torch.tensor(ts), TRACE_EXACT, mask)[0].cpu()
            assert torch.equal(big[:, rows], alone), (rows, float((big[:, rows] - alone).abs().max()))
    tail = FWD_ROWS[-1]
    xa = torch.cat([torch.zeros((21, 3), dtype=torch.float64), x[tail].double().cpu()], 1)
    params = tr.as_params(Ws, bs, requires_grad=False)
    for k in range(1, 4):
        with torch.no_grad():
            want = rr.euler_solve(params, xa, ts[:k + 1], mask).numpy()
        got = big[k, tail].double().numpy()
        for c in range(3 + d):
            err = float(np.abs(got[:, c] - want[:, c]).max() / np.abs(want[:, c]).max())
            print(f"forward B={FWD_BIG} t={ts[k]} column {c}: {err:.2e}")
            assert err <= BOUND, (k, c, err)
