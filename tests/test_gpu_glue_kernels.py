"""GPU: the small kernels that run once per training step (csrc/sample.hip, csrc/elem.hip, the Adam launch of
csrc/mlp_train.hip, the elementwise tails of csrc/cost.hip) at the branches their other tests never enter: grid strides
above the block caps, scalar fallbacks on misaligned pointers, optional outputs, draws ON the steps of a cdf, more Adam
tensors than grid rows, betas on the other side of ATen's lerp switch.  Inputs and references: tests/glue_cases.py (pinned on
the CPU by tests/test_glue_cases_host.py).  Index and bit results are compared exactly; every tolerance is derived next to
its assertion."""

import numpy as np
import pytest
import torch

import cfm_oracle as oracle
import glue_cases as cases

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _L():
    from cfm_amd import _lib
    return _lib, _lib.load()


def _ot():
    import cfm_amd.optimal_transport as ot
    return ot


def _cpu(a):
    return torch.from_numpy(np.array(a))                      # a writable copy: the case tables are read-only


def _dev(a, dev):
    return _cpu(a).to(dev)


@pytest.fixture(scope="module", autouse=True)
def _drop_large_inputs():
    yield
    _cache.clear()
    cases.xt_inputs.cache_clear()


def _off4(x):
    """A contiguous copy of x whose base pointer sits 4 bytes past a 16-byte boundary."""
    assert x.element_size() == 4
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    v = flat[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _assert_same(got, ref, what):
    """Whole-tensor bit comparison; on failure the first bad flat index (the signature of a stride bug)."""
    if torch.equal(got, ref):
        return
    bad = torch.nonzero((got != ref).reshape(-1))
    k = int(bad[0])
    raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} entries differ, first bad flat index {k} "
                         f"(shape {tuple(got.shape)}): {got.reshape(-1)[k].item()!r} != {ref.reshape(-1)[k].item()!r}")


# =============================================================================== 1. plan sampling on cdf steps
@pytest.mark.parametrize("B0,B1", cases.PLAN_SHAPES)
def test_sample_pi_on_cdf_steps(dev, B0, B1):
    """cfm_plan_sample_pi_f64 on a dyadic plan: every partial sum is exact in any order, so the pair drawn must be
    divmod(searchsorted(cumsum(P), u * T, side="right"), B1) for u on, one ulp below and one ulp above each step, for
    u = 0 over the leading empty rows / columns and for u = nextafter(1, 0)."""
    ot = _ot()
    P = cases.dyadic_plan(B0, B1)
    pd = _dev(P, dev)
    u = cases.shuffled(cases.step_draws(P.ravel(), seed=B0))
    i, j = ot.sample_pi(pd, _dev(u, dev))
    io, jo = cases.sample_pi_ref(P, u)
    i, j = i.cpu().numpy(), j.cpu().numpy()
    bad = np.flatnonzero((i != io) | (j != jo))
    assert bad.size == 0, (bad.size, u.size, [(float(u[k]).hex(), int(i[k]), int(j[k]), int(io[k]), int(jo[k])) for k in bad[:5]])
    assert (P[i, j] > 0).all()
    for n in cases.DRAW_COUNTS:                               # 4 draws per workgroup: none, a partial one, partial last
        un = np.resize(u, n)
        a, b = ot.sample_pi(pd, _dev(un, dev))
        ao, bo = cases.sample_pi_ref(P, un) if n else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        assert a.shape == (n,) and np.array_equal(a.cpu().numpy(), ao) and np.array_equal(b.cpu().numpy(), bo), n
    assert torch.equal(pd, _dev(P, dev))                      # the plan is read, never written


@pytest.mark.parametrize("B0,B1", cases.PLAN_SHAPES)
def test_sample_rows_pi_on_cdf_steps(dev, B0, B1):
    """cfm_plan_sample_rows_pi_f64: the same steps per row (every row's total a power of two); rows below 0 and past
    B0 - 1 are clamped; a row without mass returns B1 - 1 (the fallback documented in sd_sample_rows)."""
    ot = _ot()
    P = cases.dyadic_plan(B0, B1, per_row=True)
    pd = _dev(P, dev)
    rows, u = cases.row_step_cases(P, seed=B1)
    order = np.random.default_rng(0).permutation(len(rows))
    rows, u = rows[order], u[order]
    j = ot.sample_rows_pi(pd, _dev(rows, dev), _dev(u, dev)).cpu().numpy()
    jo = cases.sample_rows_ref(P, rows, u)
    bad = np.flatnonzero(j != jo)
    assert bad.size == 0, (bad.size, len(u), [(int(rows[k]), float(u[k]).hex(), int(j[k]), int(jo[k])) for k in bad[:5]])
    empty = ~P.any(axis=1)
    assert (j[empty[rows]] == B1 - 1).all()
    # clamped rows draw what rows 0 and B0 - 1 draw
    uu = np.resize(u, 12)
    for r_out, r_in in ((-7, 0), (B0 + 5, B0 - 1), (-2 ** 40, 0), (2 ** 40, B0 - 1)):
        a = ot.sample_rows_pi(pd, _dev(np.full(12, r_out, dtype=np.int64), dev), _dev(uu, dev)).cpu().numpy()
        b = ot.sample_rows_pi(pd, _dev(np.full(12, r_in, dtype=np.int64), dev), _dev(uu, dev)).cpu().numpy()
        assert np.array_equal(a, b) and np.array_equal(a, cases.sample_rows_ref(P, np.full(12, r_in), uu)), r_out
    # an all-zero plan row, asked for directly
    Z = P.copy()
    Z[0] = 0.0
    z = ot.sample_rows_pi(_dev(Z, dev), _dev(np.zeros(5, dtype=np.int64), dev), _dev(np.resize(u, 5), dev))
    assert (z.cpu().numpy() == B1 - 1).all()
    for n in cases.DRAW_COUNTS:
        rn, un = np.resize(rows, n), np.resize(u, n)
        a = ot.sample_rows_pi(pd, _dev(rn, dev), _dev(un, dev))
        assert a.shape == (n,) and np.array_equal(a.cpu().numpy(), cases.sample_rows_ref(P, rn, un)), n


@pytest.mark.parametrize("B", cases.PERM_SIZES)
def test_sample_perm_on_cdf_steps(dev, B):
    """cfm_plan_sample_perm at u = k / B, its neighbours, 0 and nextafter(1, 0): i is the first m with (m + 1) / B > u
    in float64 (the kernel's stated definition, through both of its +-1 corrections), j = perm[i]."""
    ot = _ot()
    perm = np.random.default_rng(B).permutation(B)
    u = cases.shuffled(cases.perm_step_draws(B), seed=B)
    i, j = ot.sample_perm(_dev(perm.astype(np.int32), dev), _dev(u, dev), B)
    io, jo = cases.sample_perm_ref(perm, u)
    i, j = i.cpu().numpy(), j.cpu().numpy()
    bad = np.flatnonzero(i != io)
    assert bad.size == 0, (bad.size, [(float(u[k]).hex(), int(i[k]), int(io[k])) for k in bad[:5]])
    assert np.array_equal(j, perm[i]) and np.array_equal(j, jo)


def test_sample_map_without_replacement_matches_numpy(dev):
    """OTPlanSampler.sample_map(replace=False) with n == nnz on a dyadic permutation-like plan: numpy's rejection loop
    runs several rounds (>= 3 for this seed: tests/test_glue_cases_host.py); same indices, same number of uniforms
    consumed, and the caller's plan is not modified."""
    from cfm_amd.optimal_transport import OTPlanSampler
    P, perm = cases.perm_plan_dyadic(64)
    keep = P.copy()
    np.random.seed(11)
    ref = np.random.choice(64 * 64, p=(P / P.sum()).ravel(), size=64, replace=False)
    after_ref = np.random.random_sample()
    _, rounds = cases.choice_noreplace((P / P.sum()).ravel(), 64, np.random.RandomState(11).random_sample)
    assert rounds >= 3
    np.random.seed(11)
    i, j = OTPlanSampler(method="exact").sample_map(P, 64, replace=False)
    after = np.random.random_sample()
    assert np.array_equal(i * 64 + j, ref)
    assert after == after_ref
    assert np.array_equal(P, keep)
    assert sorted(i.tolist()) == list(range(64)) and np.array_equal(j, perm[i])


# =============================================================================== 2. x_t / u_t through the C entry
METHOD_SIGMA = [(m, s) for m in cases.VARIANTS for s in cases.variant_sigmas(m)]
_cache = {}


def _coefs(method, t, sigma):
    """The per-sample scalars the Python wrapper hands over: the tensor library's cos / sin (VP), its sqrt (SB)."""
    if method == "vp":
        ang = np.pi / 2 * t
        return torch.cos(ang), torch.sin(ang)
    if method == "sb":
        return sigma * torch.sqrt(t * (1 - t)), None
    return None, None


def _xt_call(variant, x0, x1, t, eps, sigma, B, d, i=None, j=None, c0=None, c1=None, xin=None, xt=None, ut=None,
             x0g=None, x1g=None):
    _lib, lib = _L()
    p = _lib.ptr
    return lib.cfm_sample_xt_ut_f32(variant, p(x0), p(x1), p(i), p(j), p(t), p(eps), float(sigma), p(c0), p(c1), p(xin),
                                    B, d, p(xt), p(ut), p(x0g), p(x1g), _lib.stream_ptr())


def _xt_case(dev, B, d, n0=None, n1=None):
    """Device and host copies of cases.xt_inputs, uploaded once per shape."""
    key = (B, d, n0, n1)
    if key not in _cache:
        if len(_cache) >= 2:
            _cache.clear()
        host = tuple(_cpu(a) for a in cases.xt_inputs(B, d, n0, n1))
        _cache[key] = (host, tuple(a.to(dev) for a in host))
    return _cache[key]


def _run_and_check(dev, method, sigma, B, d, n0=None, n1=None, gathered=False):
    (x0, x1, eps, t, i, j), (x0d, x1d, epsd, td, idd, jdd) = _xt_case(dev, B, d, n0, n1)
    c0, c1 = _coefs(method, t, sigma)
    c0d, c1d = (None if c is None else c.to(dev) for c in (c0, c1))
    xt = torch.full((B, d), float("nan"), device=dev)
    ut = torch.full((B, d), float("nan"), device=dev)
    x0g = torch.full((B, d), float("nan"), device=dev) if gathered else None
    x1g = torch.full((B, d), float("nan"), device=dev) if gathered else None
    rc = _xt_call(cases.VARIANTS[method], x0d, x1d, td, epsd, sigma, B, d, i=idd, j=jdd, c0=c0d, c1=c1d, xt=xt, ut=ut,
                  x0g=x0g, x1g=x1g)
    assert rc == 0
    a0, a1 = x0[i], x1[j]
    xo, uo = oracle.xt_ut(method, a0, a1, t, eps, sigma)
    _assert_same(xt.cpu(), xo, f"{method} sigma {sigma} xt")
    _assert_same(ut.cpu(), uo, f"{method} sigma {sigma} ut")
    if gathered:
        _assert_same(x0g.cpu(), a0, "x0g")
        _assert_same(x1g.cpu(), a1, "x1g")


@pytest.mark.parametrize("d", [4100, 1023])
@pytest.mark.parametrize("method,sigma", METHOD_SIGMA)
def test_xt_ut_grid_stride(dev, method, sigma, d):
    """B = 2051: d = 4100 gives 2051 * 1025 = 2 102 275 float4 items, d = 1023 gives 2 098 173 scalar items; both exceed
    the 8192 * 256 = 2 097 152 of one sweep of the capped grid, so the last items are reached by the stride only."""
    _run_and_check(dev, method, sigma, 2051, d)


@pytest.mark.parametrize("d", [8, 7])
@pytest.mark.parametrize("n0,n1", [(None, None), (300, 41)])
@pytest.mark.parametrize("method,sigma", METHOD_SIGMA)
def test_xt_ut_gathered_outputs_and_larger_clouds(dev, method, sigma, n0, n1, d):
    """x0g / x1g given (vector path d = 8, scalar path d = 7): they hold x0[i], x1[j].  Source clouds of 300 and 41 rows
    against B = 96 draws whose indices reach the last row of each."""
    _run_and_check(dev, method, sigma, 96, d, n0, n1, gathered=True)


@pytest.mark.parametrize("method,sigma", METHOD_SIGMA)
def test_xt_ut_misaligned_pointers_take_the_scalar_path(dev, method, sigma):
    """d % 4 == 0 but one pointer 4 bytes past a 16-byte boundary: the scalar kernel, bit-equal to the aligned call."""
    B, d = 33, 8
    (x0, x1, eps, t, i, j), (x0d, x1d, epsd, td, idd, jdd) = _xt_case(dev, B, d)
    v = cases.VARIANTS[method]
    c0, c1 = (None if c is None else c.to(dev) for c in _coefs(method, t, sigma))
    xo, uo = oracle.xt_ut(method, x0[i], x1[j], t, eps, sigma)

    def run(which, with_xin):
        a = dict(x0=x0d, x1=x1d, eps=None if with_xin else epsd, xin=xo.to(dev) if with_xin else None,
                 xt=None if with_xin else torch.full((B, d), float("nan"), device=dev),
                 ut=torch.full((B, d), float("nan"), device=dev))
        if which is not None:
            a[which] = _off4(a[which])
        else:
            assert all(z is None or z.data_ptr() % 16 == 0 for z in a.values())
        assert _xt_call(v, a["x0"], a["x1"], td, a["eps"], sigma, B, d, i=idd, j=jdd, c0=c0, c1=c1, xin=a["xin"],
                        xt=a["xt"], ut=a["ut"]) == 0
        return (None if a["xt"] is None else a["xt"].cpu()), a["ut"].cpu()

    xt_al, ut_al = run(None, False)
    _assert_same(xt_al, xo, "aligned xt")
    _assert_same(ut_al, uo, "aligned ut")
    for which in ("x0", "x1", "eps", "xt", "ut"):
        xt_m, ut_m = run(which, False)
        _assert_same(xt_m, xt_al, f"xt with {which} misaligned")
        _assert_same(ut_m, ut_al, f"ut with {which} misaligned")
    _, ut_in = run(None, True)                                  # compute_conditional_flow on a given x_t
    _assert_same(ut_in, uo, "ut from xin")
    _, ut_in_m = run("xin", True)
    _assert_same(ut_in_m, ut_in, "ut with xin misaligned")


def test_xt_ut_sb_without_c0_is_correctly_rounded(dev):
    """SB with c0 = NULL: the kernel's own sigma * sqrtf(t * (1 - t)) against float32 NumPy, one rounded operation at a
    time in the kernel's order (np.sqrt on float32 is correctly rounded), on 4096 values of torch.rand's grid plus 0,
    0.5 and 1 - 2^-24."""
    sigma, d = 0.5, 3
    t = cases.sb_t_grid()
    B = t.size
    rng = np.random.default_rng(3)
    x0, x1, eps = (rng.standard_normal((B, d), dtype=np.float32) for _ in range(3))
    xt = torch.full((B, d), float("nan"), device=dev)
    ut = torch.full((B, d), float("nan"), device=dev)
    assert _xt_call(cases.VARIANTS["sb"], _dev(x0, dev), _dev(x1, dev), _dev(t, dev), _dev(eps, dev), sigma, B, d,
                    xt=xt, ut=ut) == 0
    xr, ur = cases.sb_ref_f32(x0, x1, t, eps, sigma)
    _assert_same(xt.cpu(), torch.from_numpy(xr), "sb xt, device sqrt")
    _assert_same(ut.cpu(), torch.from_numpy(ur), "sb ut, device sqrt")


def _bits_equal_nan(a, b):
    a, b = a.contiguous(), b.contiguous()
    same = a.view(torch.int32) == b.view(torch.int32)
    return bool((same | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("d", [8, 7])
@pytest.mark.parametrize("method,sigma", METHOD_SIGMA)
def test_xt_ut_endpoints(dev, method, sigma, d):
    """t in {0, 1}: SB divides by 1e-8, Target by sigma (at sigma = 0 and t = 1 that is 0 / 0: the NaNs must be where
    the oracle has them).  Bit patterns compared, NaN == NaN."""
    B = 64
    (x0, x1, eps, _, i, j), (x0d, x1d, epsd, _, idd, jdd) = _xt_case(dev, 96, d)
    t = (torch.arange(B) % 2).float()
    c0, c1 = (None if c is None else c.to(dev) for c in _coefs(method, t, sigma))
    xt = torch.full((B, d), float("nan"), device=dev)
    ut = torch.full((B, d), float("nan"), device=dev)
    assert _xt_call(cases.VARIANTS[method], x0d, x1d, t.to(dev), epsd, sigma, B, d, c0=c0, c1=c1, xt=xt, ut=ut) == 0
    xo, uo = oracle.xt_ut(method, x0[:B], x1[:B], t, eps[:B], sigma)
    assert _bits_equal_nan(xt.cpu(), xo), method
    assert _bits_equal_nan(ut.cpu(), uo), method
    if method == "target" and sigma == 0:
        assert not torch.isfinite(uo[1::2]).any()              # the case is what it claims to be
    else:
        assert torch.isfinite(uo).all()


def test_xt_ut_contract(dev):
    B, d = 4, 8
    x = torch.randn(B, d, device=dev)
    t = torch.rand(B, device=dev)
    xt = torch.full((B, d), 7.0, device=dev)
    ut = torch.full((B, d), 7.0, device=dev)
    ok = dict(x0=x, x1=x, t=t, eps=x, sigma=0.5, B=B, d=d, xt=xt, ut=ut)
    assert _xt_call(0, **{**ok, "B": 0}) == 0                   # B == 0: nothing to do, nothing written
    torch.cuda.synchronize()
    assert bool((xt == 7.0).all()) and bool((ut == 7.0).all())
    assert _xt_call(4, **ok) == EINVAL                          # unknown variant
    assert _xt_call(-1, **ok) == EINVAL
    assert _xt_call(3, **ok) == EINVAL                          # VP without c0 / c1
    assert _xt_call(3, **ok, c0=t) == EINVAL
    assert _xt_call(0, **{**ok, "eps": None}) == EINVAL         # neither xin nor eps
    assert _xt_call(0, **{**ok, "d": 0}) == EINVAL
    torch.cuda.synchronize()
    assert bool((xt == 7.0).all()) and bool((ut == 7.0).all())
    assert _xt_call(0, **ok) == 0                               # and the accepted call still runs
    assert not bool((ut == 7.0).all())


# =============================================================================== 3. row gather
def _gather_call(src, idx, n, row_bytes, out):
    _lib, lib = _L()
    return lib.cfm_gather_rows(_lib.ptr(src), _lib.ptr(idx), n, row_bytes, _lib.ptr(out), _lib.stream_ptr())


@pytest.mark.parametrize("shape,dtype", [((37, 2048), torch.float32), ((37, 513), torch.uint8)])
def test_gather_rows_grid_stride(dev, shape, dtype):
    """n = 4099: rows of 2048 floats are 4099 * 512 = 2 098 688 16-byte items, rows of 513 bytes 2 102 787 byte items;
    both exceed the 8192 * 256 of one sweep."""
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 255, shape, generator=g).to(dtype)
    idx = torch.randint(0, shape[0], (4099,), generator=g)
    idx[0], idx[-1] = shape[0] - 1, 0
    out = _ot().gather_rows(src.to(dev), idx.to(dev))
    _assert_same(out.cpu(), src[idx], "gather")


def test_gather_rows_misaligned_base_takes_the_byte_path(dev):
    """64-byte rows, source (then output) base 4 bytes off the 16-byte grid: same result as the aligned call."""
    g = torch.Generator().manual_seed(2)
    src = torch.randn(50, 16, generator=g).to(dev)
    idx = torch.randint(0, 50, (77,), generator=g).to(dev)
    ref = src[idx]
    out = torch.zeros(77, 16, device=dev)
    assert _gather_call(src, idx, 77, 64, out) == 0 and torch.equal(out, ref)          # aligned: 16-byte path
    out = torch.zeros(77, 16, device=dev)
    assert _gather_call(_off4(src), idx, 77, 64, out) == 0 and torch.equal(out, ref)
    out = _off4(torch.zeros(77, 16, device=dev))
    assert _gather_call(src, idx, 77, 64, out) == 0 and torch.equal(out, ref)
    out = _off4(torch.zeros(77, 16, device=dev))
    assert _gather_call(_off4(src), idx, 77, 64, out) == 0 and torch.equal(out, ref)


@pytest.mark.parametrize("shape,dtype", [((40, 3), torch.bool), ((40,), torch.uint8), ((40, 5), torch.float16),
                                          ((40, 4), torch.int32), ((40, 3), torch.float64), ((9, 2, 3, 5), torch.float32),
                                          ((40,), torch.bool), ((40, 8), torch.float16)])
def test_gather_rows_dtypes_ranks_and_index_patterns(dev, shape, dtype):
    ot = _ot()
    g = torch.Generator().manual_seed(3)
    if dtype == torch.bool:
        src = torch.rand(*shape, generator=g) < 0.5
    elif dtype.is_floating_point:
        src = (torch.randn(*shape, generator=g) * 100).to(dtype)
    else:
        src = torch.randint(0, 200, shape, generator=g).to(dtype)
    n_rows = shape[0]
    pats = [torch.randint(0, n_rows, (77,), generator=g), torch.full((50,), n_rows - 1), torch.arange(n_rows - 1, -1, -1),
            torch.zeros(0, dtype=torch.int64)]
    for idx in pats:
        out = ot.gather_rows(src.to(dev), idx.to(dev))
        assert out.dtype == dtype and out.shape == (idx.numel(),) + tuple(shape[1:])
        assert torch.equal(out.cpu(), src[idx])


def test_gather_rows_source_larger_than_the_draw(dev):
    g = torch.Generator().manual_seed(4)
    src = torch.randn(5000, 7, generator=g)
    idx = torch.tensor([4999, 0, 2500])
    assert torch.equal(_ot().gather_rows(src.to(dev), idx.to(dev)).cpu(), src[idx])


def test_gather_rows_source_past_2_31_bytes(dev):
    """524 300 rows of 4096 bytes: the last rows start past byte 2^31 (the size_t address arithmetic).  Only the rows
    that are read are initialised."""
    rows, rb = 524300, 4096
    assert (rows - 1) * rb > 2 ** 31
    src = torch.empty((rows, rb), dtype=torch.uint8, device=dev)
    idx = torch.tensor([rows - 1, 524288, 0, rows - 2], device=dev)
    g = torch.Generator().manual_seed(5)
    fill = torch.randint(0, 256, (4, rb), generator=g).to(torch.uint8)
    src[idx] = fill.to(dev)
    out = _ot().gather_rows(src, idx)
    assert torch.equal(out.cpu(), fill)


def test_take_rows_keeps_the_graph(dev):
    """A tensor that requires grad takes the differentiable index path; its gradient scatters back (with repeats)."""
    ot = _ot()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(20, 5, generator=g).to(dev).requires_grad_(True)
    idx = torch.tensor([3, 3, 19, 0, 3, 7], device=dev)
    w = torch.randint(-4, 5, (6, 5), generator=g).float().to(dev)          # integers: the scatter sum is exact
    out = ot.take_rows(x, idx)
    assert out.requires_grad and torch.equal(out.detach(), x.detach()[idx])
    (out * w).sum().backward()
    ref = torch.zeros(20, 5, device=dev).index_add_(0, idx, w)
    assert torch.equal(x.grad, ref)
    with torch.no_grad():                                                     # no graph wanted: the copy kernel
        out2 = ot.take_rows(x, idx)
    assert not out2.requires_grad and torch.equal(out2, x.detach()[idx])
    assert torch.equal(ot.take_rows(x.detach(), idx), x.detach()[idx])


# =============================================================================== 4. FusedAdam
def _adam_pair(dev, betas, eps, seed=0):
    from cfm_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=g) for n in cases.ADAM_NUMELS]
    out = []
    for cls in (FusedAdam, torch.optim.Adam):
        ps = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
        groups = [dict(params=ps[0::2], **cases.ADAM_GROUPS[0]), dict(params=ps[1::2], **cases.ADAM_GROUPS[1])]
        out.append((ps, cls(groups, betas=betas, eps=eps)))
    return init, out[0], out[1]


def _step_grads(g, dev):
    """One step's gradients: N(0, 1) times 10^k, k in [-4, 1] per tensor."""
    total = sum(cases.ADAM_NUMELS)
    flat = torch.randn(total, generator=g)
    parts = list(torch.split(flat, cases.ADAM_NUMELS))
    parts = [p * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g)) for p in parts]
    return parts, [p.to(dev) for p in parts]


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def _deviation(ps, ref64):
    """max over tensors of max |p - ref| / max(1, max |ref|): the measure of the existing one-step bound."""
    return max(float(np.abs(p.detach().cpu().double().numpy() - r).max() / max(1.0, np.abs(r).max()))
               for p, r in zip(ps, ref64))


@pytest.mark.parametrize("eps", cases.ADAM_EPS)
@pytest.mark.parametrize("betas", cases.ADAM_BETAS)
def test_fused_adam_bit_equal_over_40_tensors_and_20_steps(dev, betas, eps):
    """40 tensors in two groups (20 each: more than the 16 grid rows; numels around 256 and 65 536, the block and the
    x-sweep), 20 steps: parameters and both moments bit-equal to torch.optim.Adam after every step.  betas (0.5, .) and
    (0, .) put 1 - beta1 on the other side of ATen's lerp switch (|w| >= 0.5: g - (g - m) * (1 - w)).  Against float64:
    the existing 1e-6 * max(1, |p|) after step 1; after step 20 at most 4 x what torch.optim.Adam itself deviates from
    the same float64 iteration (measured on the reference, printed).

    Measured on an MI355X at step 20, max over tensors of |p - float64| / max(1, |float64|): torch 2.7e-07 .. 4.1e-07 over
    the eight cases, FusedAdam the same figures (bit-equal).  With the single-form lerp the kernel had before, the
    beta1 = 0.5 and beta1 = 0 cases failed at step 2 (exp_avg: 163 432 resp. 118 544 of 368 234 entries off by one ulp)."""
    init, (pa, oa), (pb, ob) = _adam_pair(dev, betas, eps)
    hyper = [cases.ADAM_GROUPS[k % 2] for k in range(len(pa))]
    p64 = [x.double().numpy() for x in init]
    m64 = [np.zeros_like(x) for x in p64]
    v64 = [np.zeros_like(x) for x in p64]
    g = torch.Generator().manual_seed(5)
    for step in range(1, cases.ADAM_STEPS + 1):
        host, devg = _step_grads(g, dev)
        for a, b, gr in zip(pa, pb, devg):
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step(); ob.step()
        for name in ("exp_avg", "exp_avg_sq"):
            _assert_same(_flat([oa.state[p][name] for p in pa]), _flat([ob.state[p][name] for p in pb]),
                         f"{name} betas {betas} eps {eps} step {step}")
        _assert_same(_flat(pa), _flat(pb), f"param betas {betas} eps {eps} step {step}")
        assert all(int(oa.state[p]["step"]) == step for p in pa)
        for k, h in enumerate(hyper):
            p64[k], m64[k], v64[k] = oracle.adam_step_f64(p64[k], host[k].double().numpy(), m64[k], v64[k], step, lr=h["lr"],
                                                          beta1=betas[0], beta2=betas[1], eps=eps,
                                                          weight_decay=h["weight_decay"])
        if step in (1, cases.ADAM_STEPS):
            dev_fused, dev_torch = _deviation(pa, p64), _deviation(pb, p64)
            print(f"adam betas {betas} eps {eps} step {step}: torch vs float64 {dev_torch:.3e}, fused vs float64 {dev_fused:.3e}")
            if step == 1:
                assert dev_fused <= 1e-6
            else:
                assert dev_fused <= 4.0 * dev_torch, (dev_fused, dev_torch)


def test_fused_adam_grad_scale(dev):
    """step(grad_scale=0.25) == a step on gradients scaled beforehand (a power of two: exact), and .grad is left scaled."""
    from cfm_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(8)
    init = [torch.randn(n, generator=g) for n in (1, 257, 70001)]
    grads = [torch.randn(n, generator=g) for n in (1, 257, 70001)]
    pa = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
    pb = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
    oa, ob = FusedAdam(pa, lr=1e-3, weight_decay=0.01), FusedAdam(pb, lr=1e-3, weight_decay=0.01)
    for _ in range(3):
        for a, b, gr in zip(pa, pb, grads):
            a.grad, b.grad = gr.to(dev).clone(), (gr * 0.25).to(dev)
        oa.step(grad_scale=0.25); ob.step()
        for a, b, gr in zip(pa, pb, grads):
            assert torch.equal(a, b) and torch.equal(a.grad, (gr * 0.25).to(dev))
            assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])


def test_fused_adam_missing_grads_mixed_steps_and_pointer_table(dev):
    from cfm_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(9)
    init = [torch.randn(n, generator=g) for n in (300, 5, 1000)]
    pa = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
    pb = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
    oa, ob = FusedAdam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    # a parameter without a gradient is skipped; the others step as torch's do
    for ps in (pa, pb):
        ps[0].grad, ps[2].grad = torch.ones(300, device=dev), torch.full((1000,), -2.0, device=dev)
    oa.step(); ob.step()
    assert torch.equal(pa[1], init[1].to(dev)) and not oa.state[pa[1]]
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    # now the skipped one gets a gradient: its step count (0) disagrees with the group's (1)
    pa[1].grad = torch.ones(5, device=dev)
    with pytest.raises(NotImplementedError):
        oa.step()
    # set_to_none gradients come back at new addresses: the pointer table is rebuilt; same addresses: it is reused
    qa = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
    qb = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
    fa, fb = FusedAdam(qa, lr=1e-3), torch.optim.Adam(qb, lr=1e-3)
    held = []
    for step in range(3):
        grads = [torch.randn(x.shape, generator=g).to(dev) for x in init]
        for a, b, gr in zip(qa, qb, grads):
            a.grad, b.grad = gr.clone(), gr.clone()
        held.append([a.grad for a in qa])                          # keep the old buffers alive: the new ones differ
        fa.step(); fb.step()
        key, table = fa._tables[0]
        assert [k[1] for k in key] == [a.grad.data_ptr() for a in qa]
        for a, gr in zip(qa, grads):
            a.grad.copy_(gr * 0.5)
        for b, gr in zip(qb, grads):
            b.grad.copy_(gr * 0.5)
        fa.step(); fb.step()
        assert fa._tables[0][1] is table                           # same pointers: not rebuilt
        assert all(torch.equal(a, b) for a, b in zip(qa, qb))
        fa.zero_grad(set_to_none=True); fb.zero_grad(set_to_none=True)
        assert all(a.grad is None for a in qa)
    assert len({h[0].data_ptr() for h in held}) == 3


# =============================================================================== 5. RBF sums
def _rbf_call(D, n, gam, ng, out):
    _lib, lib = _L()
    return lib.cfm_rbf_mix_sum_f32(_lib.ptr(D), n, _lib.ptr(gam), ng, _lib.ptr(out), _lib.stream_ptr())


@pytest.mark.parametrize("sigmas", [[s] for s in cases.RBF_SIGMAS] + [cases.RBF_SIGMAS])
@pytest.mark.parametrize("n", cases.RBF_SIZES)
def test_rbf_mix_sum_vs_float64(dev, n, sigmas):
    """cfm_rbf_mix_sum_f32 against float64 NumPy on the same fp32 D and fp32 gammas, relative 1e-6: every term is
    non-negative (no cancellation); per term expf within 2 ulp (2.4e-7), the rounded argument at most x e^-x 2^-24 <=
    2.2e-8 of the largest term, n_gamma fp32 adds (<= 5 * 6e-8); fp64 accumulation adds nothing visible: below 6e-7.
    out is accumulated into: 3.5 comes back as 3.5 + sum."""
    D = cases.rbf_distances(n)
    gam = cases.rbf_gammas(sigmas)
    ref = cases.rbf_sum_f64(D, gam)
    out = torch.full((1,), 3.5, dtype=torch.float64, device=dev)
    assert _rbf_call(_dev(D, dev), n, _dev(gam, dev), len(sigmas), out) == 0
    got = float(out.cpu()) - 3.5
    print(f"rbf n {n} sigmas {sigmas}: sum {ref:.9e} rel err {abs(got - ref) / ref:.2e}")
    assert ref >= n / 7.0                                           # the exact zeros of D alone contribute 1 each
    assert abs(got - ref) <= cases.RBF_RTOL * ref + 2.0 ** -50 * (3.5 + ref)


def test_rbf_mix_sum_underflow_and_contract(dev):
    gam = _dev(cases.rbf_gammas(cases.RBF_SIGMAS), dev)
    D = torch.tensor([1e9, 3e38, 2.5e6] * 100, device=dev)          # gamma_min * D >= 125: every term is 0 in fp32
    assert cases.rbf_sum_f64(D.cpu().numpy(), gam.cpu().numpy()) < 1e-50
    out = torch.full((1,), 3.5, dtype=torch.float64, device=dev)
    assert _rbf_call(D, 300, gam, 5, out) == 0
    assert float(out.cpu()) == 3.5
    assert _rbf_call(D, 0, gam, 5, out) == 0 and float(out.cpu()) == 3.5                # n == 0
    assert _rbf_call(D, 300, gam, 0, out) == EINVAL and float(out.cpu()) == 3.5
    assert _rbf_call(None, 300, gam, 5, out) == EINVAL
    Z = torch.zeros(257, device=dev)                                # all zeros: exactly n * n_gamma
    assert _rbf_call(Z, 257, gam, 5, out) == 0 and float(out.cpu()) == 3.5 + 5 * 257


@pytest.mark.parametrize("d", [1, 8, 9, 50])
@pytest.mark.parametrize("m", [1, 2, 300, 725])
def test_mix_rbf_mmd2_absolute_bound(dev, m, d):
    """metrics.mix_rbf_mmd2 against float64 from float64 distances.  The MMD is a difference of three large sums, so the
    bound is absolute (cases.mmd2_abs_bound: the kernel sums' 1e-6 plus what the cost kernel's own relative bound can
    move each exp)."""
    from cfm_amd.metrics import mix_rbf_mmd2
    X, Y = cases.mmd_clouds(m, d)
    ref, sums = cases.mmd2_ref(X, Y, cases.RBF_SIGMAS)
    got = float(mix_rbf_mmd2(_cpu(X), _cpu(Y), cases.RBF_SIGMAS))
    bound = cases.mmd2_abs_bound(sums, m, d, len(cases.RBF_SIGMAS))
    print(f"mmd m {m} d {d}: ref {ref:.9e} got {got:.9e} err {abs(got - ref):.2e} bound {bound:.2e}")
    assert abs(got - ref) <= bound
    same = float(mix_rbf_mmd2(_cpu(X), _cpu(X), cases.RBF_SIGMAS))
    assert abs(same) <= 1e-12
    with pytest.raises(NotImplementedError):
        mix_rbf_mmd2(_cpu(X), _cpu(Y), cases.RBF_SIGMAS, biased=False)


# =============================================================================== 6. cost tails
@pytest.mark.parametrize("max_at", ["first", "last"])
def test_cost_tails_above_the_block_caps(dev, max_at):
    """normalize=True and squared=False at 1025 x 1025 (1 050 625 entries: max_reduce_f32 strides past 2048 blocks,
    scale_inv / sqrt_inplace past 4096): Mn bit-equal to M / M.max() with a maximum of exactly 1, M1 bit-equal to the
    correctly rounded float32 sqrt of M; the maximum sits at entry 0 or at the last entry (reached by the stride only)."""
    ot = _ot()
    B0, B1, _ = cases.COST_TAIL_SHAPE
    x0, x1 = (_dev(a, dev) for a in cases.cost_tail_clouds(max_at))
    M = ot.cost_matrix(x0, x1).cpu().numpy()
    at = np.unravel_index(M.argmax(), M.shape)
    assert at == ((0, 0) if max_at == "first" else (B0 - 1, B1 - 1))
    Mn = ot.cost_matrix(x0, x1, normalize=True).cpu().numpy()
    assert Mn.max() == 1.0 and Mn[at] == 1.0
    np.testing.assert_array_equal(Mn, M / M.max())
    M1 = ot.cost_matrix(x0, x1, squared=False).cpu().numpy()
    assert M1.dtype == np.float32
    np.testing.assert_array_equal(M1, np.sqrt(M))
    M1n = ot.cost_matrix(x0, x1, squared=False, normalize=True).cpu().numpy()
    assert M1n.max() == 1.0 and M1n[at] == 1.0
