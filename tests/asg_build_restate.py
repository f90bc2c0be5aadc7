"""NumPy restatement of the candidate-list build of the exact solver (csrc/assign_sparse.h: wide_build).

For every row i of the fp32 cost matrix M and the fp64 prices p the build keeps at most SP_K = 64 columns:

    m      = min_k (fp64(c_ik) + p_k)                                   the row minimum
    r_k    = fp32((fp64(c_ik) + p_k) - m)                               >= 0, round to nearest
    hi     = max over the 64 lanes of (min of the lane's r_k)            count(r <= hi) >= 64
    t1     = the fp32 successor of hi
    tau    = t1                        if count(r < t1) <= 64
           = the bisection's `lo`      otherwise: lo = 0, hh = t1, clo = 0; at most 48 steps while clo < 32:
                                       mid = 0.5f * (lo + hh); stop unless lo < mid < hh; cm = count(r < mid);
                                       cm <= 64 ? (lo, clo) = (mid, cm) : hh = mid
           = +inf                      if n <= 64 (every column is listed)
    members: r_k < tau, written slot-major, then by lane, as (column, bits of c_ik); the rest of the 64 entries is
             (0xffff, bits of +inf)
    cT_i   = (m + fp64(tau) * (1 - 2.4e-7)) - 1e-290                    (+inf if n <= 64)

The lane-to-column map decides `hi` and the order.  Fast path (n % 1024 == 0, n > 64): a lane holds the columns
256 j + 4 lane + e in slot 4 j + e; slow path: the columns lane + 64 t in slot t.

The bisection can end with tau = 0 (no members) or with fewer than 32 members when the costs are tied so heavily that
no fp32 threshold separates 32..64 of them: the documented exit — the bound cT stays valid, the solver relaxes such a
row densely.
"""
import numpy as np

SP_K = 64
NOCOL = 0xFFFF
INF_BITS = 0x7F800000


def is_fast(n):
    return n % 1024 == 0 and n > SP_K


def lane_slot(n):
    """(lane[k], slot[k]) of every column on the path that size n takes."""
    k = np.arange(n)
    if is_fast(n):
        return (k >> 2) & 63, 4 * (k >> 8) + (k & 3)
    return k & 63, k >> 6


def row_tau(r, lane):
    """tau of one row from its r (fp32 [n]) and the lane of every column, and how the rule ended: "all" (n <= 64),
    "t1", "window" (the bisection found 32..64 columns), or the documented exits "collapsed" (no fp32 value is left
    between lo and hh) and "cap" (48 steps)."""
    n = r.shape[0]
    if n <= SP_K:
        return np.float32(np.inf), "all"
    lmin = np.full(64, np.inf, dtype=np.float32)
    np.minimum.at(lmin, lane, r)
    hi = lmin.max()
    t1 = (hi.view(np.uint32) + np.uint32(1)).view(np.float32)
    if int((r < t1).sum()) <= SP_K:
        return t1, "t1"
    lo, hh, clo, how = np.float32(0.0), t1, 0, "cap"
    half = np.float32(0.5)
    for _ in range(48):
        if clo >= SP_K // 2:
            how = "window"
            break
        mid = np.float32(half * np.float32(lo + hh))
        if not (mid > lo and mid < hh):
            how = "collapsed"
            break
        cm = int((r < mid).sum())
        if cm <= SP_K:
            lo, clo = mid, cm
        else:
            hh = mid
    else:
        how = "window" if clo >= SP_K // 2 else "cap"
    return lo, how


def build_lists(M, p):
    """M: fp32 [n, n], p: fp64 [n] -> (cl uint32 [n, 64, 2], cT fp64 [n], tau fp32 [n], count int [n])."""
    M = np.ascontiguousarray(M, dtype=np.float32)
    p = np.ascontiguousarray(p, dtype=np.float64)
    n = M.shape[0]
    assert M.shape == (n, n) and p.shape == (n,)
    lane, slot = lane_slot(n)
    order = np.argsort(slot * 64 + lane, kind="stable")      # columns in the order the build writes them
    cl = np.empty((n, SP_K, 2), dtype=np.uint32)
    cl[:, :, 0] = NOCOL
    cl[:, :, 1] = INF_BITS
    cT = np.empty(n, dtype=np.float64)
    taus = np.empty(n, dtype=np.float32)
    counts = np.empty(n, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            s = M[i].astype(np.float64) + p
            m = s.min()
            r = (s - m).astype(np.float32)
            tau, _ = row_tau(r, lane)
            mem = order[r[order] < tau] if np.isfinite(tau) else order
            cnt = mem.shape[0]
            assert cnt <= SP_K
            cl[i, :cnt, 0] = mem.astype(np.uint32)
            cl[i, :cnt, 1] = M[i, mem].view(np.uint32)
            cT[i] = np.inf if not np.isfinite(tau) else (m + np.float64(tau) * (1.0 - 2.4e-7)) - 1e-290
            taus[i] = tau
            counts[i] = cnt
    return cl, cT, taus, counts
