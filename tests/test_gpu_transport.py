"""GPU: cfm_transport_exact_f32 — exact OT between uniform marginals of different sizes without the lcm expansion
(round 6: primal-dual phases with a tree push, optional assignment warm start).  Checked against an independent LP
solver (scipy.optimize.linprog / HiGHS) on the same fp32 matrix: equal optimal cost, exact marginals; cold start and
warm start must agree; sizes up to B0 + B1 = 2048.  The second half runs the solver at its edges: B0 + B1 = 2048 exactly
(8 x 2040 and its transpose: p = 255, q = 1; one supplier; 1024 x 1024), large common divisors, both sides of the
LDS-staging decision (130 x 138 / 130 x 139), the C entry's refusals, and constant / tied / badly scaled costs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lp_cost(M):
    from scipy.optimize import linprog
    import scipy.sparse as sp
    B0, B1 = M.shape
    A = sp.vstack([sp.kron(sp.eye(B0), np.ones((1, B1))), sp.kron(np.ones((1, B0)), sp.eye(B1))]).tocsr()
    b = np.concatenate([np.full(B0, 1.0 / B0), np.full(B1, 1.0 / B1)])
    r = linprog(M.astype(np.float64).ravel(), A_eq=A, b_eq=b, bounds=(0, None), method="highs")
    assert r.status == 0
    return float(r.fun)


def _cloud_cost(B0, B1, d, seed, dev):
    import cfm_amd.optimal_transport as ot
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B0, d, generator=g); x1 = torch.randn(B1, d, generator=g) * 0.7 + 0.5
    return ot.cost_matrix(x0.to(dev), x1.to(dev))


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("B0,B1,d", [(127, 128, 2), (128, 127, 2), (100, 60, 16), (37, 50, 3), (255, 256, 8), (300, 257, 4),
                                     (3, 2, 1), (1, 5, 2), (97, 211, 5), (125, 128, 2), (2, 2, 1), (64, 64, 3)])
def test_transport_cost_equals_the_lp_optimum(B0, B1, d, warm):
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    M = _cloud_cost(B0, B1, d, 100 * B0 + B1, dev)
    plan, cost, info = ot.transport_exact(M, warm_start=warm, return_info=True)
    P = plan.cpu().numpy(); Mh = M.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(P.sum(1), 1.0 / B0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(P.sum(0), 1.0 / B1, rtol=0, atol=1e-15)
    assert (P >= 0).all()
    assert cost == pytest.approx(float((P * Mh).sum()), rel=1e-12)
    assert cost == pytest.approx(_lp_cost(M.cpu().numpy()), rel=1e-9, abs=1e-12)
    if warm and B0 != B1:
        assert info["warm_start_used"]
        if abs(B0 - B1) == 1:
            assert info["phases"] == 1            # one forest into the one open column carries every row's last unit


def test_transport_is_deterministic_and_staged_equals_global():
    """Same input, same plan (the pushes are integer sums, the returns go in row order); and the LDS-staged form
    (127 x 128 fits) and the global-memory form of the same kernel (140 x 163 does not fit), each against the LP."""
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    M = _cloud_cost(127, 128, 2, 5, dev)
    p1, c1, i1 = ot.transport_exact(M, warm_start=False, return_info=True)
    p2, c2, i2 = ot.transport_exact(M, warm_start=False, return_info=True)
    assert i1["staged"] and torch.equal(p1, p2) and c1 == c2 and i1["phases"] == i2["phases"]
    M2 = _cloud_cost(140, 163, 2, 6, dev)
    p3, c3, i3 = ot.transport_exact(M2, warm_start=False, return_info=True)
    p4, c4, i4 = ot.transport_exact(M2, warm_start=False, return_info=True)
    assert not i3["staged"] and torch.equal(p3, p4) and c3 == c4
    assert c3 == pytest.approx(_lp_cost(M2.cpu().numpy()), rel=1e-9)


@pytest.mark.parametrize("B0,B1,d", [(511, 512, 2), (1000, 1001, 8), (1023, 1025, 3), (700, 1300, 4)])
def test_transport_at_the_sizes_round_5_refused(B0, B1, d):
    """B0 + B1 up to 2048 (round 5: 512).  Certified in fp64 by the solver's own pass; checked here against the
    dual bound it certifies with: cost == sum_i u_i / B0 + sum_j v_j / B1 cannot be recomputed from outside, so the
    independent check is the LP for 511 x 512 and, beyond, agreement of cold and warm start on the unique optimal cost."""
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    M = _cloud_cost(B0, B1, d, B0 + 7 * B1, dev)
    plan, cost, info = ot.transport_exact(M, return_info=True)
    P = plan.cpu().numpy()
    np.testing.assert_allclose(P.sum(1), 1.0 / B0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(P.sum(0), 1.0 / B1, rtol=0, atol=1e-15)
    if B0 * B1 <= 300000:
        assert cost == pytest.approx(_lp_cost(M.cpu().numpy()), rel=1e-9)
    else:
        _, cost2, info2 = ot.transport_exact(M, warm_start=not info["warm_start_used"], return_info=True)
        assert cost == pytest.approx(cost2, rel=1e-12)
    print(f"{B0}x{B1}: phases {info['phases']} sweeps {info['sweeps']} support {info['support']} warm {info['warm_start_used']}")


def test_an_invalid_or_suboptimal_warm_start_is_ignored():
    """sigma is validated on the device (distinct, in range) and its duals must exist (label correcting must converge):
    a permutation that is NOT optimal has a negative cycle and is dropped; the result is the optimum either way."""
    import ctypes
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    from cfm_amd._lib import check, ptr, stream_ptr
    dev = _lib.require_gpu()
    lib = _lib.load()
    B0, B1 = 63, 64
    M = _cloud_cost(B0, B1, 2, 9, dev)
    ref = _lp_cost(M.cpu().numpy())
    for sigma in (torch.arange(B0, dtype=torch.int32),                       # valid, not optimal
                  torch.zeros(B0, dtype=torch.int32),                        # not distinct
                  torch.full((B0,), 99, dtype=torch.int32)):                 # out of range
        plan = torch.empty((B0, B1), dtype=torch.float64, device=dev)
        tot = torch.empty(1, dtype=torch.float64, device=dev); info = torch.empty(8, dtype=torch.int32, device=dev)
        ws = _lib.workspace(_lib.OP_TRANSPORT, B0, B1, 0, dev)
        check(lib.cfm_transport_exact_f32(ptr(M), B0, B1, ptr(sigma.to(dev)), ptr(plan), ptr(tot), ptr(info), ptr(ws), stream_ptr()), "tp")
        st = info.cpu()
        assert int(st[0]) == 1 and not (int(st[7]) & 2)
        assert float(tot.cpu()[0]) == pytest.approx(ref, rel=1e-9)


def test_wasserstein_between_eval_sets_of_1000_and_1500_points():
    """The reference's evaluation call wasserstein(x0, x1) on sets of different sizes (optimal_transport.py:286-292): lcm 3000
    — the expanded assignment route; checked against SciPy's LSAP on the expanded matrix (an independent exact solver
    on the same fp32 costs) and, at 100 vs 150, against HiGHS."""
    import cfm_amd.optimal_transport as ot
    import cfm_oracle as oracle
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1000, 2, generator=g); y = torch.randn(1500, 2, generator=g) * 0.8 + 0.4
    M = ot.cost_matrix(x.to(dev), y.to(dev)).cpu().numpy().astype(np.float64)
    _, ref_cost = oracle.exact_plan_rect(M)
    assert ot.wasserstein(x, y, method="exact", power=2) == pytest.approx(np.sqrt(ref_cost), rel=1e-9)
    Ms = ot.cost_matrix(x[:100].to(dev), y[:150].to(dev)).cpu().numpy()
    assert ot.wasserstein(x[:100], y[:150], method="exact", power=2) == pytest.approx(np.sqrt(_lp_cost(Ms)), rel=1e-6)


def test_rectangular_exact_plan_beyond_the_lcm_bound_goes_through_the_transport_solver():
    """exact_plan_rect / OTPlanSampler('exact') / wasserstein for 127 vs 128 (lcm 16256 > 8192): no NotImplementedError
    any more; the plan is a transport plan with the LP's cost."""
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(127, 2, generator=g); x1 = torch.randn(128, 2, generator=g) + 1.0
    M = ot.cost_matrix(x0.to(dev), x1.to(dev))
    plan, cost = ot.exact_plan_rect(M)
    ref = _lp_cost(M.cpu().numpy())
    assert cost == pytest.approx(ref, rel=1e-9)
    s = ot.OTPlanSampler(method="exact")
    pi = s.get_map(x0, x1)
    assert pi.shape == (127, 128) and np.allclose(pi.sum(1), 1 / 127) and np.allclose(pi.sum(0), 1 / 128)
    w2 = ot.wasserstein(x0, x1, method="exact", power=2)
    assert w2 == pytest.approx(np.sqrt(ref), rel=1e-6)


def test_transport_with_ties_and_sizes_it_refuses():
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    r = np.random.RandomState(0)
    M = torch.from_numpy(r.randint(0, 3, (45, 64)).astype(np.float32)).to(dev)       # massively tied
    plan, cost = ot.transport_exact(M)
    assert cost == pytest.approx(_lp_cost(M.cpu().numpy()), rel=1e-9, abs=1e-12)
    big = torch.rand(1500, 1501, device=dev)
    with pytest.raises(NotImplementedError):
        ot.exact_plan_rect(big)


# ---------------------------------------------------------------- the solver at its edges
# Every case below goes through _check_transport: exact marginals (1e-15), plan >= 0, cost == sum P M (1e-12), cost ==
# the reference (1e-9: HiGHS on the same fp32 matrix, or the value known in closed form), cold start == forced warm
# start wherever a warm start exists (B0 != B1).  SUPPORT collects support / (R + C) per case: the arc list holds
# TP_ARC_PER_NODE = 6 arcs per node and is rebuilt once fewer than R + C slots are free, so a ratio above 5 means the
# rebuild ran; the largest ratio seen is printed (and recorded in DESIGN.md 4.7).
SUPPORT = {}


def _check_one(M, Mh, ref, warm, what):
    import cfm_amd.optimal_transport as ot
    B0, B1 = M.shape
    plan, cost, info = ot.transport_exact(M, warm_start=warm, return_info=True)
    P = plan.cpu().numpy()
    np.testing.assert_allclose(P.sum(1), 1.0 / B0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(P.sum(0), 1.0 / B1, rtol=0, atol=1e-15)
    assert (P >= 0).all()
    assert cost == pytest.approx(float((P * Mh).sum()), rel=1e-12, abs=0.0)
    gap = abs(cost - ref) / abs(ref) if ref != 0.0 else abs(cost)
    ratio = info["support"] / (B0 + B1)
    SUPPORT[what + (" warm" if warm else " cold")] = ratio
    print(f"{what} {'warm' if warm else 'cold'}: phases {info['phases']} sweeps {info['sweeps']} support {info['support']} "
          f"(x{ratio:.3f} of R + C; largest so far x{max(SUPPORT.values()):.3f}) staged {info['staged']} "
          f"cost gap {gap:.2e}")
    assert gap <= 1e-9, (what, cost, ref)
    assert info["warm_start_used"] == bool(warm)
    return cost, info


def _check_transport(M, ref, what):
    Mh = M.cpu().numpy().astype(np.float64)
    cold, info = _check_one(M, Mh, ref, False, what)
    if M.shape[0] != M.shape[1]:
        warm, _ = _check_one(M, Mh, ref, True, what)
        assert warm == pytest.approx(cold, rel=1e-12, abs=0.0)
    return cold, info


@pytest.mark.parametrize("B0,B1", [(8, 2040), (2040, 8), (1, 2047), (2047, 1)])
def test_transport_at_the_size_bound_with_an_extreme_ratio(B0, B1):
    """B0 + B1 = 2048 = TP_NMAX exactly.  8 vs 2040: gcd 8, every row supplies p = 255 units and every column takes
    q = 1 (ratio 255), in both orientations (2040 x 8 goes through the transposed copy); 1 vs 2047: a single supplier
    (the plan is the uniform row: cost = mean of M), staged in LDS by the size formula."""
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    M = _cloud_cost(B0, B1, 2, 100 * B0 + B1, dev)
    ref = _lp_cost(M.cpu().numpy())
    if min(B0, B1) == 1:
        assert ref == pytest.approx(float(M.cpu().numpy().astype(np.float64).mean()), rel=1e-9)
    _, info = _check_transport(M, ref, f"{B0}x{B1}")
    assert info["staged"] == (min(B0, B1) == 1)


def test_transport_square_at_the_size_bound():
    """1024 x 1024 (p = q = 1: an assignment problem, no warm start exists) against SciPy's LSAP on the same fp32
    matrix: cost = the assignment's total / 1024."""
    from scipy.optimize import linear_sum_assignment
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    B = 1024
    M = _cloud_cost(B, B, 2, 100 * B + B, dev)
    Mh = M.cpu().numpy().astype(np.float64)
    r, c = linear_sum_assignment(Mh)
    _check_transport(M, float(Mh[r, c].sum()) / B, f"{B}x{B}")


@pytest.mark.parametrize("B0,B1", [(48, 180), (90, 150)])
def test_transport_with_a_large_common_divisor(B0, B1):
    """gcd 12 (p / q = 15 / 4) and gcd 30 (5 / 3): exact_plan_rect would take the lcm route for these (lcm 720, 450),
    so transport_exact is called directly."""
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    M = _cloud_cost(B0, B1, 3, 100 * B0 + B1, dev)
    _check_transport(M, _lp_cost(M.cpu().numpy()), f"{B0}x{B1}")


def test_transport_on_both_sides_of_the_staging_decision():
    """Node state + staged matrix and flows <= 158 KiB = 161 792 B: 130 x 138 needs 161 384 and is staged in LDS,
    130 x 139 needs 162 492 and works in global memory."""
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    staged = {}
    for B0, B1 in ((130, 138), (130, 139)):
        M = _cloud_cost(B0, B1, 2, 100 * B0 + B1, dev)
        _, info = _check_transport(M, _lp_cost(M.cpu().numpy()), f"{B0}x{B1}")
        staged[B1] = info["staged"]
    assert staged == {138: True, 139: False}


def test_transport_c_entry_refusals():
    """CFM_EINVAL (-1): B0 + B1 = 2049, B0 = 0, a null plan; CFM_EALIGN (-2): a workspace pointer off by 8.  All four
    return before anything is launched; exact_plan_rect turns 1025 vs 1024 into NotImplementedError."""
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    from cfm_amd._lib import ptr, stream_ptr
    dev = _lib.require_gpu()
    lib = _lib.load()
    B0, B1 = 1025, 1024
    M = torch.rand(B0, B1, device=dev)
    plan = torch.empty((B0, B1), dtype=torch.float64, device=dev)
    tot = torch.empty(1, dtype=torch.float64, device=dev); info = torch.empty(8, dtype=torch.int32, device=dev)
    ws = torch.empty(8 * B0 * B1 + (1 << 20), dtype=torch.uint8, device=dev)      # larger than any layout of this shape
    assert ws.data_ptr() % 16 == 0

    def call(b0, b1, plan_, ws_):
        return lib.cfm_transport_exact_f32(ptr(M), b0, b1, ptr(None), ptr(plan_), ptr(tot), ptr(info), ptr(ws_), stream_ptr())
    assert call(B0, B1, plan, ws) == -1
    assert call(0, B1, plan, ws) == -1
    assert call(63, 64, None, ws) == -1
    assert call(63, 64, plan, ws[8:]) == -2
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError):
        ot.exact_plan_rect(M)


def _tied_cloud_cost(B0, B1, seed, dev):
    """every x1 row four times: columns in identical groups of four, the regime of the lcm expansion"""
    import cfm_amd.optimal_transport as ot
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B0, 2, generator=g)
    x1 = (torch.randn(B1 // 4, 2, generator=g) * 0.7 + 0.5).repeat_interleave(4, dim=0)
    assert x1.shape[0] == B1
    return ot.cost_matrix(x0.to(dev), x1.to(dev))


@pytest.mark.parametrize("B0,B1", [(45, 64), (8, 200)])
def test_transport_cost_structure(B0, B1):
    """Constant, tied and badly scaled costs.  The certificate's tolerance is 1e-10 * max |M|, so it must follow the scale.

    Scaled matrices: s M is rounded to fp32 again (each entry moves by at most 2^-24 relative, all entries >= 0), so the
    two optima satisfy |opt(s M) / s - opt(M)| <= 2^-24 (1 + 2^-24) opt(M) and no closer; that is asserted as the
    sanity check of the scale, and the 1e-9 bound is asserted against HiGHS on the SAME scaled fp32 matrix."""
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    cost, _ = _check_transport(torch.zeros(B0, B1, device=dev), 0.0, f"{B0}x{B1} zeros")
    assert cost == 0.0
    cost, _ = _check_transport(torch.full((B0, B1), 3.0, device=dev), 3.0, f"{B0}x{B1} constant 3")
    assert cost == pytest.approx(3.0, rel=1e-12, abs=0.0)
    Mt = _tied_cloud_cost(B0, B1, 100 * B0 + B1, dev)
    _check_transport(Mt, _lp_cost(Mt.cpu().numpy()), f"{B0}x{B1} x1 rows four times")
    M = _cloud_cost(B0, B1, 2, 100 * B0 + B1, dev)
    base, _ = _check_transport(M, _lp_cost(M.cpu().numpy()), f"{B0}x{B1} cloud")
    for s in (1e6, 1e-6):
        Ms = (M * s).contiguous()
        # (HiGHS works to absolute tolerances: it gets the matrix at O(1), rescaled in float64 — the same LP)
        ref = _lp_cost(Ms.cpu().numpy().astype(np.float64) / s) * s
        cs, _ = _check_transport(Ms, ref, f"{B0}x{B1} cloud * {s:g}")
        assert abs(cs / s - base) <= 2.0 ** -24 * (1 + 2.0 ** -24) * base + 1e-15 * base
