"""Case table of tests/test_gpu_unbalanced_shapes.py and tests/test_unbalanced_shapes_host.py: the shapes at which
the device code of csrc/unbalanced.hip takes another branch, their seeded inputs, and the float64 references
(oracle/cfm_oracle.py) in the order NumPy sums them and in the reversed order.

Shape (B0, B1) -> what it selects in unbalanced.hip:
  (1, 1), (1, 7), (7, 1)   one row / one column: a row wave with one live lane, one strip, one column workgroup
  (5, 3)                   odd B1 below one wave: the scalar body of ub_row_dot, one trip
  (33, 65)                 odd B1, two trips of the scalar loop; two strips of 17 and 16 rows (8-row unroll plus a tail of
                           1 / no tail); a second 64-column workgroup of ub_col_fused with ONE live lane
  (96, 257), (257, 255)    odd B1 across two 256-column tiles of ub_coldot (the second: 1 column / none; odd / odd)
  (40, 514), (31, 1030)    even B1: second / third trip of the 512-column loop of ub_row_dot with a partial group of
                           double2 loads (only the inner jj < B1 guard protects the tail)
  (1100, 130)              the deciding wave of ub_col_fused<0> re-reads u in rounds of 1024 rows: a second round
  (2049, 66)               64 strips of 33 rows: the last one empty (63 * 33 > 2049), the one before it 3 rows (tail loop
                           only); the deciding wave of ub_col_fused<1> reads alpha2 in rounds of 2048 rows: a second round
"""
import functools

import numpy as np

import cfm_oracle as oracle

RTOL = 1e-9            # same fp32 cost matrix on both sides: summation order only (tests/test_gpu_unbalanced.py)
RTOL_REVERSED = 1e-11  # the oracle against itself with every sum taken in the reversed order: two orders inside RTOL

SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 65), (96, 257), (257, 255), (40, 514), (31, 1030), (1100, 130), (2049, 66)]
UNB_PARAMS = [(0.5, 1.0), (0.3, 5.0)]       # (reg, reg_m); default max_iter = 1000 and stop_thr = 1e-6
UNB_STOP_THR = 1e-6
PAR_REG = 0.5
PAR_MASSES = [1.0, 0.7]
PAR_STOP_THR = -1.0    # never met: both sides run exactly max_iter iterations


def seed_of(B0, B1):
    return 100 * B0 + B1


def clouds(B0, B1, seed=None):
    """x0 ~ N(0, I_2), x1 ~ 0.7 N(0, I_2) + 0.5, float32."""
    rng = np.random.default_rng(seed_of(B0, B1) if seed is None else seed)
    x0 = rng.standard_normal((B0, 2)).astype(np.float32)
    x1 = (0.7 * rng.standard_normal((B1, 2)) + 0.5).astype(np.float32)
    return x0, x1


def host_cost(x0, x1):
    """fp32 squared distances computed on the host (the admissibility test has no device; the GPU tests read the
    device's own matrix back instead: the two differ in the last bit, which is nothing to the conditioning)."""
    d = x0[:, None, :].astype(np.float64) - x1[None, :, :].astype(np.float64)
    return (d * d).sum(-1).astype(np.float32)


def partial_max_iter(B0, B1):
    """The full-matrix Dykstra oracle costs O(B0^2 B1) per iteration: 40 where that is cheap, 21 elsewhere (still past
    the checks at iterations 0, 10 and 20)."""
    return 40 if B0 * B0 * B1 < 3e6 else 21


def flipped(M):
    return np.ascontiguousarray(np.asarray(M)[::-1, ::-1])


def unbalanced_ref(M, reg, reg_m, reverse=False, **kw):
    """(plan, log) of the oracle; reverse: every dot product summed in the reversed order (the oracle on the matrix with
    rows and columns reversed — uniform marginals — flipped back)."""
    if not reverse:
        return oracle.sinkhorn_knopp_unbalanced(M, reg, reg_m, log=True, **kw)
    G, log = oracle.sinkhorn_knopp_unbalanced(flipped(M), reg, reg_m, log=True, **kw)
    return flipped(G), log


def partial_ref(M, reg, m, max_iter, reverse=False):
    f = oracle.entropic_partial_wasserstein
    if not reverse:
        return f(M, reg, m=m, numItermax=max_iter, stopThr=PAR_STOP_THR, log=True)
    G, log = f(flipped(M), reg, m=m, numItermax=max_iter, stopThr=PAR_STOP_THR, log=True)
    return flipped(G), log


def unbalanced_check_errors(M, reg, reg_m):
    """(err at the deciding check, err at the check before it, iterations).  The oracle checks at iterations 0, 10, 20,
    ... and leaves the loop at the head of the next one, so it stops after 10 k + 1 iterations; capped at 10 (k - 1) + 1
    it returns the error of the check before."""
    _, log = unbalanced_ref(M, reg, reg_m)
    it = log["iters"]
    assert it % 10 == 1 and it > 1, it
    before = None
    if it > 11:
        _, lb = unbalanced_ref(M, reg, reg_m, numItermax=it - 10)
        assert lb["iters"] == it - 10
        before = lb["err"]
    return log["err"], before, it


def rel_gap(p, ref):
    return float(np.abs(p - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------- the stopping error must see rows beyond 1024
# The table's (1100, 130) RUNS the second round of the deciding wave's scan of u, but its largest |u - u'| sits in row
# 337, and every row converges at the same rate: a wave that skipped rows 1024.. would stop at the same check.  Here
# row 1099 is an outlier at (4, 4) — lane 11 of the second round — whose scaling moves most at the check of iteration
# 10: err = 1.20e-2 with it, 5.43e-3 over rows 0..1023 alone.  With stop_thr = 8e-3 between the two the loop runs 21
# iterations (err 1.26e-3 at the check of iteration 20) where a scan of the first round alone gives 11.
# (The partial solver's second round, rows 2048.., only feeds the finiteness flag of alpha2: it can be run — (2049, 66)
#  does — but not made to decide anything without an overflow.)
OUTLIER_SHAPE, OUTLIER_ROW, OUTLIER_POINT = (1100, 130), 1099, (4.0, 4.0)
OUTLIER_REG, OUTLIER_REG_M, OUTLIER_STOP_THR, OUTLIER_ITERS = 0.5, 5.0, 8e-3, 21


def outlier_clouds():
    x0, x1 = clouds(*OUTLIER_SHAPE)
    x0 = x0.copy()
    x0[OUTLIER_ROW] = OUTLIER_POINT
    return x0, x1


def unbalanced_check_trace(M, reg, reg_m, iterations, rows=None):
    """The stopping errors of the unbalanced loop at iterations 0, 10, ... < `iterations` (no early exit), restated
    from the oracle; rows: the row maxima taken over the first `rows` rows only (what a truncated scan would see)."""
    K = np.exp(np.asarray(M, dtype=np.float64) / -reg)
    B0, B1 = K.shape
    u, v, fi = np.full(B0, 1.0 / B0), np.full(B1, 1.0 / B1), reg_m / (reg_m + reg)
    errs = []
    for cpt in range(iterations):
        up, vp = u, v
        u = ((1.0 / B0) / K.dot(v)) ** fi
        v = ((1.0 / B1) / K.T.dot(u)) ** fi
        if cpt % 10 == 0:
            uu, pp = u[:rows], up[:rows]
            err_u = abs(uu - pp).max() / max(abs(uu).max(), abs(pp).max(), 1.0)
            err_v = abs(v - vp).max() / max(abs(v).max(), abs(vp).max(), 1.0)
            errs.append(0.5 * (err_u + err_v))
    return errs


# ---------------------------------------------------------------- mid-loop revert (tests/golden/ub_revert_cases.npz)
def revert_cloud(B0, B1, scale, seed):
    """1-D clouds scaled by `scale`: exp(-M / reg) spans hundreds of orders of magnitude, and with a stiff reg_m the
    scalings grow until one overflows — at an iteration that depends on the input alone."""
    rng = np.random.default_rng(seed)
    x0 = (scale * rng.standard_normal((B0, 1))).astype(np.float32)
    x1 = (scale * rng.standard_normal((B1, 1))).astype(np.float32)
    return x0, x1


@functools.lru_cache(maxsize=None)
def _cached_host_case(B0, B1):
    x0, x1 = clouds(B0, B1)
    return x0, x1, host_cost(x0, x1)


def host_case(B0, B1):
    return _cached_host_case(B0, B1)
