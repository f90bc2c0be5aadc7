"""Restatements of cfm_amd.TrajectoryFlowMatcher for its tests (a helper module imported by test files; not a conftest).

linear : runner/src/models/cfm_module.py:173-193, :225-242 written out op by op in NumPy float32, every operation
         separately rounded in the reference's order — the result the eager path AND the fused kernel must equal bit
         for bit.  The one input taken from the tensor library is the SB path's sigma_t = sigma * sqrt(t (1 - t)): the
         matchers pass it from eager torch.sqrt (not correctly rounded on every backend), and so does the caller here.
spline : scipy.interpolate.CubicSpline(tau, y, bc_type="natural") in float64, per row (rows share the knots, so one
         vectorised CubicSpline over the stacked trajectories evaluated at each row's own time).
"""
import numpy as np

F = np.float32


def linear(X, t_select, t, eps, sigma, variant="icfm", leave=0, idx=None, sigma_t=None):
    """X [B, T, d] f32, t_select [B] int (the interval of each row), t / eps the local time and the noise, leave = the
    left-out slice while training (0: none), idx = None or int [T-1, 2, B] index pairs.  -> xt, ut, t_net (float32)."""
    X = np.asarray(X, dtype=F)
    B, T, d = X.shape
    t = np.asarray(t, dtype=F)
    eps = np.asarray(eps, dtype=F).reshape(B, d)
    k = np.asarray(t_select, dtype=np.int64)
    halved = (k + 1 == leave) if leave > 0 else np.zeros(B, dtype=bool)
    k1 = k + 1 + halved
    rb = np.arange(B)
    r0 = rb if idx is None else np.asarray(idx)[k, 0, rb]
    r1 = rb if idx is None else np.asarray(idx)[k, 1, rb]
    x0, x1 = X[r0, k], X[r1, k1]
    tp = t[:, None]
    omt = F(1) - tp
    mu = tp * x1 + omt * x0
    if variant == "icfm":
        xt = mu + F(sigma) * eps
        ut = x1 - x0
    else:
        sig = np.asarray(sigma_t, dtype=F)[:, None]
        xt = mu + sig * eps
        two_t = F(2) * tp
        ratio = (F(1) - two_t) / (two_t * omt + F(1e-8))
        ut = ratio * (xt - mu) + x1 - x0
    t_net = t.copy()
    if leave > 0:
        ut[halved] = ut[halved] / F(2)
        t_net[halved] = t_net[halved] * F(2)
    t_net = t_net + k.astype(F)
    for z in (xt, ut, t_net):
        assert z.dtype == F
    return xt, ut, t_net


def knots(T, leave=0):
    return [k for k in range(T) if not (leave > 0 and k == leave)]


def spline(X, t_select, u, eps, sigma, leave=0, chain=None):
    """float64 SciPy reference: X [B, T, d], t_select [B] knot interval among knots(T, leave), u [B] in [0, 1),
    chain = None or int [T', B] (row of X that trajectory b visits at knot q).  -> xt, ut, t_net (float64), traj."""
    from scipy.interpolate import CubicSpline
    X = np.asarray(X, dtype=np.float64)
    B, T, d = X.shape
    kn = knots(T, leave)
    tau = np.asarray(kn, dtype=np.float64)
    Xk = X[:, kn]
    if chain is not None:
        Xk = Xk[np.asarray(chain).T, np.arange(len(kn))[None, :]]
    i = np.asarray(t_select, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    t_net = tau[i] + u * (tau[i + 1] - tau[i])
    cs = CubicSpline(tau, Xk, axis=1, bc_type="natural")
    # row b at its own time: SciPy's piecewise polynomial of interval i, sum_m c[m, i] (t - tau_i)^(3 - m) (PPoly's form;
    # cs(t_net) would evaluate every row at every row's time)
    c = cs.c[:, i, np.arange(B), :]                                 # [4, B, d]
    dt = (t_net - tau[i])[:, None]
    mu = ((c[0] * dt + c[1]) * dt + c[2]) * dt + c[3]
    ut = (3.0 * c[0] * dt + 2.0 * c[1]) * dt + c[2]
    xt = mu + float(sigma) * np.asarray(eps, dtype=np.float64).reshape(B, d)
    return xt, ut, t_net, Xk


def second_derivatives(tau, y):
    """SciPy's natural-spline second derivatives at the knots, y [n, m] -> [n, m]"""
    from scipy.interpolate import CubicSpline
    tau = np.asarray(tau, dtype=np.float64)
    return CubicSpline(tau, np.asarray(y, dtype=np.float64), axis=0, bc_type="natural")(tau, 2)


def rel(got, want):
    """max|got - want| / max|want|; a reference that is zero everywhere admits no error at all"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale
