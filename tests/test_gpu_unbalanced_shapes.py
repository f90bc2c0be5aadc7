"""GPU: cfm_unbalanced_sinkhorn_f64 / cfm_partial_entropic_f64 at the shapes where the device code of
csrc/unbalanced.hip branches (tests/ub_shape_cases.py maps shape -> branch): odd B1 (scalar row path), B1 > 512 with a
partial group (second / third trip of the double2 row path), ragged strips and column tiles, an empty and a 3-row
strip, a second round of the deciding wave's row scan (both solvers), a revert to the previous iterate in the middle of
the loop at both parities of the ping-pong buffers, max_iter = 0 and an even iteration cap.

Reference: oracle/cfm_oracle.py in float64 NumPy on the SAME fp32 matrix, read back from the device; partial against
the full-matrix q1 / q2 / q3 form, not the vector form the kernel carries.  Bound: RTOL = 1e-9 of the largest entry, as
in tests/test_gpu_unbalanced.py; tests/test_unbalanced_shapes_host.py shows on the CPU that the inputs are conditioned
two orders inside it (the oracle against itself in the reversed summation order: <= 3.8e-15).

Partial, row and column sums: after 21 / 40 Dykstra iterations the ITERATE still exceeds a marginal by up to 8.3e-3 in
the oracle itself (the inequality holds at the fixed point only), so the sums are held to the larger of the marginal
and the oracle's own sum, + 1e-12; test_partial_converged_respects_the_marginals runs one case to the fixed point and
asserts the inequality against the marginal alone.

Measured on the device (largest |plan - oracle| / max oracle): unbalanced <= 1.3e-15 and partial <= 2.1e-15 over the
table (both at 2049 x 66), the mid-loop reverts 1.2e-16 / 2.0e-16, max_iter = 0 and 12 <= 8.0e-16; every iteration
count and status equal to the oracle's.  The tests print each figure."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import ub_shape_cases as cases

pytestmark = pytest.mark.gpu

RTOL = cases.RTOL


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _ot():
    import cfm_amd.optimal_transport as ot
    return ot


@functools.lru_cache(maxsize=None)
def _case(B0, B1):
    """(x0, x1, device fp32 cost matrix, the same matrix on the host): built once per shape, never written to."""
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    x0, x1 = cases.clouds(B0, B1)
    M = _ot().cost_matrix(torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev))
    Mh = M.cpu().numpy()
    Mh.setflags(write=False)
    return x0, x1, M, Mh


@functools.lru_cache(maxsize=None)
def _unb_ref(B0, B1, reg, reg_m, max_iter=1000):
    G, log = cases.unbalanced_ref(_case(B0, B1)[3], reg, reg_m, numItermax=max_iter)
    G.setflags(write=False)
    return G, log


@functools.lru_cache(maxsize=None)
def _par_ref(B0, B1, m, max_iter):
    G, log = cases.partial_ref(_case(B0, B1)[3], cases.PAR_REG, m, max_iter)
    G.setflags(write=False)
    return G, log


def _assert_close(p, ref, what):
    gap = cases.rel_gap(p, ref)
    print(f"{what}: |plan - oracle| / max = {gap:.2e}")
    assert np.isfinite(p).all() and gap <= RTOL, (what, gap)


def _assert_partial_plan(p, ref, m, B0, B1, what):
    _assert_close(p, ref, what)
    assert abs(p.sum() - m) < 1e-12
    assert (p.sum(1) <= np.maximum(1.0 / B0, ref.sum(1)) + 1e-12).all()
    assert (p.sum(0) <= np.maximum(1.0 / B1, ref.sum(0)) + 1e-12).all()


@pytest.mark.parametrize("reg,reg_m", cases.UNB_PARAMS)
@pytest.mark.parametrize("B0,B1", cases.SHAPES)
def test_unbalanced_edge_shape(dev, B0, B1, reg, reg_m):
    _, _, M, _ = _case(B0, B1)
    ref, log = _unb_ref(B0, B1, reg, reg_m)
    plan, info = _ot().unbalanced_plan(M, reg, reg_m)
    _assert_close(plan.cpu().numpy(), ref, f"unbalanced {B0}x{B1} reg {reg} reg_m {reg_m} ({log['iters']} iterations)")
    assert info.tolist()[:2] == [log["iters"], log["status"]] and log["status"] == 0
    assert info.tolist()[2:] == [0, 0]


def test_unbalanced_stopping_error_sees_rows_beyond_1024(dev):
    """The deciding wave's second round of 1024 rows DECIDES here: row 1099 is an outlier whose scaling carries the
    check of iteration 10 over stop_thr = 8e-3 (1.20e-2 with it, 5.43e-3 over rows 0..1023 alone; shown on the CPU in
    tests/test_unbalanced_shapes_host.py) — 21 iterations; a scan that missed the row would return after 11."""
    x0, x1 = cases.outlier_clouds()
    M = _ot().cost_matrix(torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev))
    reg, reg_m, thr = cases.OUTLIER_REG, cases.OUTLIER_REG_M, cases.OUTLIER_STOP_THR
    ref, log = cases.unbalanced_ref(M.cpu().numpy(), reg, reg_m, stopThr=thr)
    assert (log["iters"], log["status"]) == (cases.OUTLIER_ITERS, 0)
    plan, info = _ot().unbalanced_plan(M, reg, reg_m, stop_thr=thr)
    assert info.tolist() == [cases.OUTLIER_ITERS, 0, 0, 0]
    _assert_close(plan.cpu().numpy(), ref, "unbalanced 1100x130, outlier in row 1099, stop_thr 8e-3")


@pytest.mark.parametrize("m", cases.PAR_MASSES)
@pytest.mark.parametrize("B0,B1", cases.SHAPES)
def test_partial_edge_shape(dev, B0, B1, m):
    _, _, M, _ = _case(B0, B1)
    n = cases.partial_max_iter(B0, B1)
    ref, log = _par_ref(B0, B1, m, n)
    plan, info = _ot().partial_plan(M, cases.PAR_REG, m=m, max_iter=n, stop_thr=cases.PAR_STOP_THR)
    _assert_partial_plan(plan.cpu().numpy(), ref, m, B0, B1, f"partial {B0}x{B1} m {m} ({n} iterations)")
    assert info.tolist() == [log["iters"], log["status"], 0, 0] and log["iters"] == n and log["status"] == 0


def test_partial_converged_respects_the_marginals(dev):
    """(33, 65), m = 0.7, 1000 iterations: at the fixed point no row or column carries more than its marginal."""
    B0, B1, m = 33, 65, 0.7
    _, _, M, _ = _case(B0, B1)
    ref, log = _par_ref(B0, B1, m, 1000)
    plan, info = _ot().partial_plan(M, cases.PAR_REG, m=m, max_iter=1000, stop_thr=cases.PAR_STOP_THR)
    p = plan.cpu().numpy()
    _assert_close(p, ref, "partial 33x65 m 0.7 (1000 iterations)")
    assert info.tolist() == [1000, 0, 0, 0] == [log["iters"], log["status"], 0, 0]
    assert abs(p.sum() - m) < 1e-12
    assert (p.sum(1) <= 1.0 / B0 + 1e-12).all() and (p.sum(0) <= 1.0 / B1 + 1e-12).all()


def test_max_iter_zero_returns_the_initial_iterate(dev):
    """No iteration: unbalanced u = 1 / B0, v = 1 / B1 -> K / (B0 B1); partial -> K m / sum K."""
    B0, B1 = 33, 65
    _, _, M, Mh = _case(B0, B1)
    ot = _ot()
    for reg, reg_m in cases.UNB_PARAMS:
        K = np.exp(Mh.astype(np.float64) / -reg)
        plan, info = ot.unbalanced_plan(M, reg, reg_m, max_iter=0)
        ref, log = _unb_ref(B0, B1, reg, reg_m, 0)
        p = plan.cpu().numpy()
        _assert_close(p, ref, f"unbalanced max_iter 0 reg {reg}")
        _assert_close(p, K / (B0 * B1), f"unbalanced max_iter 0 reg {reg}, closed form")
        assert info.tolist() == [0, 0, 0, 0] and log["iters"] == 0
    K = np.exp(Mh.astype(np.float64) / -cases.PAR_REG)
    for m in cases.PAR_MASSES:
        plan, info = ot.partial_plan(M, cases.PAR_REG, m=m, max_iter=0)
        ref, log = _par_ref(B0, B1, m, 0)
        p = plan.cpu().numpy()
        _assert_close(p, ref, f"partial max_iter 0 m {m}")
        _assert_close(p, K * (m / K.sum()), f"partial max_iter 0 m {m}, closed form")
        assert info.tolist() == [0, 0, 0, 0] and log["iters"] == 0


@pytest.mark.parametrize("B0,B1", [(96, 257), (40, 514)])
def test_even_iteration_cap_returns_buffer_zero(dev, B0, B1):
    """max_iter = 12: the loop ends at the cap after a non-check iteration, the result sits in buffer 12 & 1 = 0."""
    _, _, M, _ = _case(B0, B1)
    ot = _ot()
    for reg, reg_m in cases.UNB_PARAMS:
        ref, log = _unb_ref(B0, B1, reg, reg_m, 12)
        plan, info = ot.unbalanced_plan(M, reg, reg_m, max_iter=12)
        _assert_close(plan.cpu().numpy(), ref, f"unbalanced {B0}x{B1} reg {reg} max_iter 12")
        assert info.tolist() == [12, 0, 0, 0] and (log["iters"], log["status"]) == (12, 0)
    for m in cases.PAR_MASSES:
        ref, log = _par_ref(B0, B1, m, 12)
        plan, info = ot.partial_plan(M, cases.PAR_REG, m=m, max_iter=12, stop_thr=cases.PAR_STOP_THR)
        _assert_partial_plan(plan.cpu().numpy(), ref, m, B0, B1, f"partial {B0}x{B1} m {m} max_iter 12")
        assert info.tolist() == [12, 0, 0, 0] and (log["iters"], log["status"]) == (12, 0)


@pytest.mark.parametrize("parity", ["even", "odd"])
def test_mid_loop_revert_returns_the_previous_iterate(dev, golden_dir, parity):
    """A numerical error at iteration cpt >= 1 (an overflowing scaling: the oracle's own arithmetic on a recorded input,
    tests/golden/make_ub_revert_golden.py) -> status 1, iterations cpt, and the iterate of cpt - 1, which sits in
    buffer cpt & 1: one recorded input per parity."""
    z = np.load(os.path.join(golden_dir, "ub_revert_cases.npz"))
    Mh, reg, reg_m = z[f"{parity}_M"], float(z[f"{parity}_reg"]), float(z[f"{parity}_reg_m"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref, log = cases.unbalanced_ref(Mh, reg, reg_m)
    assert log["status"] == 1 and log["iters"] == int(z[f"{parity}_iters"]) >= 1
    assert (log["iters"] & 1) == (1 if parity == "odd" else 0)
    plan, info = _ot().unbalanced_plan(torch.from_numpy(Mh).to(dev), reg, reg_m)
    assert info.tolist()[:2] == [log["iters"], 1]
    _assert_close(plan.cpu().numpy(), ref, f"revert at iteration {log['iters']} ({parity})")


@pytest.mark.parametrize("method", ["unbalanced", "partial"])
def test_public_sampler_at_an_odd_rectangle(dev, method):
    """OTPlanSampler.get_map at (96, 257) is the direct call on the same clouds; sample_map on that plan draws what
    np.random.choice draws on the flattened, normalised plan (torchcfm/optimal_transport.py:99-121)."""
    from cfm_amd.optimal_transport import OTPlanSampler
    B0, B1 = 96, 257
    x0, x1, M, _ = _case(B0, B1)
    s = OTPlanSampler(method=method, reg=0.5, reg_m=1.0)
    pi = s.get_map(torch.from_numpy(x0), torch.from_numpy(x1))
    assert pi.dtype == np.float64 and pi.shape == (B0, B1)
    if method == "unbalanced":
        direct, info = _ot().unbalanced_plan(M, 0.5, 1.0)
        assert np.array_equal(pi, direct.cpu().numpy())            # no floating-point atomics in this loop: the same bits
        _assert_close(pi, _unb_ref(B0, B1, 0.5, 1.0)[0], "get_map unbalanced 96x257")
    else:
        direct, info = _ot().partial_plan(M, 0.5)
        # (the Dykstra loop adds its column totals with floating-point atomics: the order, and the last bits, vary)
        _assert_close(pi, direct.cpu().numpy(), "get_map partial 96x257 against the direct call")
    assert info.tolist()[1:] == [0, 0, 0]
    np.random.seed(17)
    i, j = s.sample_map(pi, 300)
    np.random.seed(17)
    p = pi.flatten()
    flat = np.random.choice(pi.size, p=p / p.sum(), size=300, replace=True)
    wi, wj = np.divmod(flat, B1)
    assert np.array_equal(i, wi) and np.array_equal(j, wj)
