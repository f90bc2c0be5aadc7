"""CPU: the inputs of tests/test_gpu_unbalanced_shapes.py are admissible — the 1e-9 bound of the GPU tests then checks
the kernel and not the conditioning of the input.  Per shape of tests/ub_shape_cases.py, on the host-built fp32 matrix:
status 0, no zero in the Gibbs kernel, the oracle's error at the deciding check and at the one before it at least 1 %
away from the threshold (the device's iteration count cannot hang on a rounding), and the oracle with every sum taken
in the reversed order within 1e-11 of the largest entry of itself.

Measured (float64 NumPy): unbalanced 21 .. 131 iterations, smallest K 2.5e-57, closest error to the threshold 8.8e-7
against 1e-6 (40 x 514, reg 0.3); reversed order: unbalanced at most 1.2e-15 (1100 x 130), partial at most 3.8e-15
(2049 x 66, m = 0.7) of the largest entry, the mid-loop revert inputs at most 1.9e-16 (the tests print each figure)."""
import os
import warnings

import numpy as np
import pytest

import ub_shape_cases as cases


@pytest.mark.parametrize("reg,reg_m", cases.UNB_PARAMS)
@pytest.mark.parametrize("B0,B1", cases.SHAPES)
def test_unbalanced_inputs_are_admissible(B0, B1, reg, reg_m):
    _, _, M = cases.host_case(B0, B1)
    K = np.exp(M.astype(np.float64) / -reg)
    assert (K > 0.0).all()
    G, log = cases.unbalanced_ref(M, reg, reg_m)
    assert log["status"] == 0 and log["iters"] < 1000
    err, before, it = cases.unbalanced_check_errors(M, reg, reg_m)
    assert it == log["iters"] and err <= cases.UNB_STOP_THR
    assert abs(err - cases.UNB_STOP_THR) >= 0.01 * cases.UNB_STOP_THR
    if before is not None:
        assert before > cases.UNB_STOP_THR and abs(before - cases.UNB_STOP_THR) >= 0.01 * cases.UNB_STOP_THR
    Gr, logr = cases.unbalanced_ref(M, reg, reg_m, reverse=True)
    gap = cases.rel_gap(Gr, G)
    print(f"unbalanced {B0}x{B1} reg {reg} reg_m {reg_m}: iters {it} Kmin {K.min():.2e} err {err:.3e} before {before} reversed {gap:.2e}")
    assert (logr["iters"], logr["status"]) == (it, 0)
    assert gap <= cases.RTOL_REVERSED


@pytest.mark.parametrize("m", cases.PAR_MASSES)
@pytest.mark.parametrize("B0,B1", cases.SHAPES)
def test_partial_inputs_are_admissible(B0, B1, m):
    _, _, M = cases.host_case(B0, B1)
    assert (np.exp(M.astype(np.float64) / -cases.PAR_REG) > 0.0).all()
    n = cases.partial_max_iter(B0, B1)
    G, log = cases.partial_ref(M, cases.PAR_REG, m, n)
    assert (log["iters"], log["status"]) == (n, 0) and np.isfinite(G).all()
    Gr, logr = cases.partial_ref(M, cases.PAR_REG, m, n, reverse=True)
    gap = cases.rel_gap(Gr, G)
    print(f"partial {B0}x{B1} m {m}: iters {n} reversed {gap:.2e}")
    assert (logr["iters"], logr["status"]) == (n, 0)
    assert gap <= cases.RTOL_REVERSED


@pytest.mark.parametrize("B0,B1", [(96, 257), (40, 514)])
def test_even_cap_inputs_are_admissible(B0, B1):
    """max_iter = 12: both loops stop at the cap, after a non-check iteration, far from any threshold."""
    _, _, M = cases.host_case(B0, B1)
    for reg, reg_m in cases.UNB_PARAMS:
        G, log = cases.unbalanced_ref(M, reg, reg_m, numItermax=12)
        Gr, logr = cases.unbalanced_ref(M, reg, reg_m, numItermax=12, reverse=True)
        assert (log["iters"], log["status"]) == (12, 0) == (logr["iters"], logr["status"])
        assert log["err"] > 1.01 * cases.UNB_STOP_THR          # the check at iteration 10 did not stop the loop
        assert cases.rel_gap(Gr, G) <= cases.RTOL_REVERSED
    for m in cases.PAR_MASSES:
        G, log = cases.partial_ref(M, cases.PAR_REG, m, 12)
        Gr, _ = cases.partial_ref(M, cases.PAR_REG, m, 12, reverse=True)
        assert (log["iters"], log["status"]) == (12, 0) and cases.rel_gap(Gr, G) <= cases.RTOL_REVERSED


def test_outlier_input_makes_the_second_scan_round_decide():
    """(1100, 130) with row 1099 at (4, 4): the check of iteration 10 is above the threshold only through that row, so
    a scan of rows 0..1023 alone would stop at 11 iterations instead of 21; every error at least 1 % from the threshold."""
    x0, x1 = cases.outlier_clouds()
    M = cases.host_cost(x0, x1)
    reg, reg_m, thr = cases.OUTLIER_REG, cases.OUTLIER_REG_M, cases.OUTLIER_STOP_THR
    assert (np.exp(M.astype(np.float64) / -reg) > 0.0).all()
    full = cases.unbalanced_check_trace(M, reg, reg_m, 21)
    cut = cases.unbalanced_check_trace(M, reg, reg_m, 21, rows=1024)
    print(f"outlier case: errors {full} (rows 0..1023 alone: {cut}), threshold {thr}")
    assert full[1] > 1.01 * thr > 0.99 * thr > cut[1] and full[2] < 0.99 * thr and full[0] > 1.01 * thr
    G, log = cases.unbalanced_ref(M, reg, reg_m, stopThr=thr)
    assert (log["iters"], log["status"]) == (cases.OUTLIER_ITERS, 0) and log["err"] == pytest.approx(full[2], rel=1e-12)
    Gr, logr = cases.unbalanced_ref(M, reg, reg_m, stopThr=thr, reverse=True)
    assert logr["iters"] == log["iters"] and cases.rel_gap(Gr, G) <= cases.RTOL_REVERSED


def test_converged_partial_input_is_admissible():
    """(33, 65), m = 0.7, 1000 iterations (test_partial_converged_respects_the_marginals): the oracle's own plan is
    inside the marginals at the fixed point, and stable under the reversed order."""
    _, _, M = cases.host_case(33, 65)
    G, log = cases.partial_ref(M, cases.PAR_REG, 0.7, 1000)
    Gr, _ = cases.partial_ref(M, cases.PAR_REG, 0.7, 1000, reverse=True)
    assert (log["iters"], log["status"]) == (1000, 0) and cases.rel_gap(Gr, G) <= cases.RTOL_REVERSED
    assert (G.sum(1) <= 1.0 / 33 + 1e-13).all() and (G.sum(0) <= 1.0 / 65 + 1e-13).all()


@pytest.mark.parametrize("parity", ["even", "odd"])
def test_mid_loop_revert_inputs_are_what_the_search_recorded(golden_dir, parity):
    """tests/golden/ub_revert_cases.npz (tests/golden/make_ub_revert_golden.py): status 1 at the recorded iteration
    >= 1 of the recorded parity, the same in the reversed order, plans within 1e-11 of each other."""
    z = np.load(os.path.join(golden_dir, "ub_revert_cases.npz"))
    M, reg, reg_m, it = z[f"{parity}_M"], float(z[f"{parity}_reg"]), float(z[f"{parity}_reg_m"]), int(z[f"{parity}_iters"])
    assert M.dtype == np.float32 and max(M.shape) <= 8
    assert np.array_equal(M, cases.host_cost(z[f"{parity}_x0"], z[f"{parity}_x1"]))
    assert it >= 1 and (it & 1) == (1 if parity == "odd" else 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        G, log = cases.unbalanced_ref(M, reg, reg_m)
        Gr, logr = cases.unbalanced_ref(M, reg, reg_m, reverse=True)
    assert (log["iters"], log["status"]) == (it, 1) == (logr["iters"], logr["status"])
    gap = cases.rel_gap(Gr, G)
    print(f"revert {parity}: {M.shape[0]}x{M.shape[1]} reg_m {reg_m:.4g} stops at {it}, reversed {gap:.2e}")
    assert np.isfinite(G).all() and gap <= cases.RTOL_REVERSED
