"""CPU restatements of the explicit Runge-Kutta solvers for the ODE solver tests (a helper module imported by test
files and by tests/golden/make_ode_solvers_golden.py; not a conftest).

Written like oracle/cfm_oracle.py::dopri5_trajectory and parametrised by tableau: the state is NumPy float64, the scalar
controller (t, dt, the error ratio, the step factor) is float32 exactly as in conditional-flow-matching_amd/csrc/ode.hip.
The coefficients below are this module's own copy (the tests check the package's tables against the order conditions
and against these).  `coef_dtype`: the kernels and the oracle's dopri5 round every tableau entry to float32 before use
(np.float32, the default); NeuralODE's generic path multiplies by the float64 entries (np.float64).

The two float32 powers of the controller (initial step, step factor) are taken with NumPy's scalar operator `**`, as
NeuralODE's generic path takes them; the oracle's dopri5 takes them with np.power, which is one ulp away on about a
sixth of all inputs.  With the dopri5 tableau this restatement therefore follows the oracle's to rounding (same step
sequence wherever no decision sits on a knife edge), not bit for bit.

rk4 is the 3/8 rule ("torchdyn-style rk4"; torchdyn is absent from the reference tree, so the form is unpinned).
"""
import numpy as np

import cfm_oracle as oracle

ADAPTIVE = {
    "dopri5": dict(c=oracle.DP_C, a=oracle.DP_A, e=[s - a for s, a in zip(oracle.DP_BSOL, oracle.DP_BALT)]),
    "tsit5": dict(
        c=[0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0],
        a=[[0.161],
           [-0.008480655492356989, 0.335480655492357],
           [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
           [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
           [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
           [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774]],
        e=[0.001780011052226, 0.000816434459657, -0.007880878010262, 0.144711007173263, -0.582357165452555,
           0.458082105929187, -1.0 / 66.0]),
}
FIXED = {
    "euler": dict(c=[], a=[], b=[1.0]),
    "midpoint": dict(c=[0.5], a=[[0.5]], b=[0.0, 1.0]),
    "rk4": dict(c=[1.0 / 3, 2.0 / 3, 1.0], a=[[1.0 / 3], [-1.0 / 3, 1.0], [1.0, -1.0, 1.0]],
                b=[1.0 / 8, 3.0 / 8, 3.0 / 8, 1.0 / 8]),
}


def _hn(x):
    return np.sqrt(np.mean(np.abs(x) ** 2))


# ----------------------------------------------------------------------------------------------- order conditions
def butcher(c, a, b):
    """(A [s, s] strictly lower triangular, b [s], c [s]) in float64 from the row lists (c and a start at stage 2)."""
    s = len(b)
    A = np.zeros((s, s))
    for i, row in enumerate(a):
        A[i + 1, :len(row)] = row
    return A, np.asarray(b, dtype=np.float64), np.concatenate([[0.0], np.asarray(c, dtype=np.float64)])


def order_residuals(A, b, c):
    """{order: [residual of every rooted-tree condition of that order]} through order 5 (1 + 1 + 2 + 4 + 9 = 17
    conditions; Hairer, Norsett, Wanner I, table II.2.1), with c the abscissae (the row-sum condition is separate)."""
    Ac = A @ c
    return {
        1: [b.sum() - 1.0],
        2: [b @ c - 1 / 2],
        3: [b @ c ** 2 - 1 / 3, b @ Ac - 1 / 6],
        4: [b @ c ** 3 - 1 / 4, b @ (c * Ac) - 1 / 8, b @ (A @ c ** 2) - 1 / 12, b @ (A @ Ac) - 1 / 24],
        5: [b @ c ** 4 - 1 / 5, b @ (c ** 2 * Ac) - 1 / 10, b @ (Ac * Ac) - 1 / 20, b @ (c * (A @ c ** 2)) - 1 / 15,
            b @ (c * (A @ Ac)) - 1 / 30, b @ (A @ c ** 3) - 1 / 20, b @ (A @ (c * Ac)) - 1 / 40,
            b @ (A @ (A @ c ** 2)) - 1 / 60, b @ (A @ (A @ Ac)) - 1 / 120],
    }


# ----------------------------------------------------------------------------------------------- integrators
def fixed_trajectory(f, x, t_span, scheme, coef_dtype=np.float32):
    """Explicit fixed steps exactly on t_span (dt < 0 steps backward): float64 state, float32 t / dt / stage times."""
    f32 = np.float32
    tab = FIXED[scheme]
    co = lambda v: float(coef_dtype(v))
    ts = np.asarray(t_span, dtype=np.float32)
    x = np.asarray(x, dtype=np.float64)
    sol = [x]
    for k in range(len(ts) - 1):
        t, dt = ts[k], f32(ts[k + 1] - ts[k])
        ks = [f(float(t), x)]
        for c, row in zip(tab["c"], tab["a"]):
            y = x + float(dt) * sum(co(a) * kq for a, kq in zip(row, ks))
            ks.append(f(float(f32(t + f32(c) * dt)), y))
        x = x + float(dt) * sum(co(b) * kq for b, kq in zip(tab["b"], ks))
        sol.append(x)
    return np.stack(sol)


def adaptive_trajectory(f, x, t_span, atol, rtol, tableau="tsit5", coef_dtype=np.float32, return_log=False):
    """torchdyn-style adaptive odeint with a 7-stage FSAL 5(4) pair whose last row of a is b: Hairer
    init_step (order 5), global RMS error norm over the batch, every t_span point is a step end, adapt_step with safety
    0.9 / min 0.2 / max 10 / order 5.  t_span increasing (a decreasing grid is the solve of -f(-s, y) on -t_span)."""
    f32 = np.float32
    tab = ADAPTIVE[tableau]
    TA, TC, TE = tab["a"], tab["c"], tab["e"]
    co = lambda v: float(coef_dtype(v))
    ts = np.asarray(t_span, dtype=np.float32)
    x = np.asarray(x, dtype=np.float64)
    atol, rtol = float(f32(atol)), float(f32(rtol))
    sol = [x]
    nfe = 0

    def ev(t, y):
        nonlocal nfe
        nfe += 1
        return f(float(t), y)

    t, T = f32(ts[0]), f32(ts[-1])
    k1 = ev(t, x)
    scale = atol + np.abs(x) * rtol
    d0, d1 = f32(_hn(x / scale)), f32(_hn(k1 / scale))
    h0 = f32(1e-6) if (d0 < f32(1e-5) or d1 < f32(1e-5)) else f32(f32(0.01) * d0 / d1)
    f1 = ev(f32(t + h0), x + float(h0) * k1)
    d2 = f32(f32(_hn((f1 - k1) / scale)) / h0)
    if d1 <= f32(1e-15) and d2 <= f32(1e-15):
        h1 = max(f32(1e-6), f32(h0 * f32(1e-3)))
    else:
        h1 = f32(f32(f32(0.01) / max(d1, d2)) ** (f32(1.0) / f32(6.0)))
    dt = f32(min(f32(f32(100) * h0), h1))
    ckpt, steps, log = 1, 0, []
    while t < T:
        if f32(t + dt) > T:
            dt = f32(T - t)
        dt_old, flag = dt, False
        if ckpt < len(ts) and f32(t + dt) > ts[ckpt]:
            dt_old, flag, dt = dt, True, f32(ts[ckpt] - t)
        lands = ckpt < len(ts) and (flag or f32(t + dt) == ts[ckpt])
        ks = [k1]
        y = x
        for s in range(6):
            y = x + float(dt) * sum(co(a) * k for a, k in zip(TA[s], ks))
            ks.append(ev(f32(t + f32(TC[s]) * dt), y))
        x_new = y
        err = float(dt) * sum(co(e) * k for e, k in zip(TE, ks))
        ratio = f32(_hn(err / (atol + rtol * np.maximum(np.abs(x), np.abs(x_new)))))
        steps += 1
        accept = ratio <= f32(1)
        log.append((float(t), float(dt), float(ratio), bool(accept)))
        if accept:
            if lands:
                t = f32(ts[ckpt]); sol.append(x_new); ckpt += 1
            else:
                t = f32(t + dt)
            x, k1 = x_new, ks[6]
        if flag:
            dt = f32(dt_old - dt)
        if ratio == 0:
            factor = f32(10)
        else:
            minf = f32(1.0) if ratio < f32(1) else f32(0.2)
            factor = min(f32(10), max(f32(f32(0.9) / ratio ** f32(0.2)), minf))
        dt = f32(dt * factor)
        if not dt > f32(1e-12):
            dt = f32(1e-12)
    out = np.stack(sol)
    return (out, {"steps": steps, "nfe": nfe, "log": log}) if return_log else out


def ratios_clear_of_one(log, lo=0.99, hi=1.01):
    """No step attempt of the log has its error ratio in [lo, hi]: float32 state arithmetic (errors ~1e-6 relative in
    the ratio) cannot then flip an accept / reject decision of the float64 restatement."""
    r = np.asarray([l[2] for l in log], dtype=np.float64)
    return bool(np.all((r < lo) | (r > hi)))


def assert_same_log(log, recorded):
    """A log integrated here against a recorded one (rows t, dt, ratio, accept): the same decisions, t and dt to
    float32 rounding, the ratios to 1e-3 relative.  The ratio is a cancellation (an error estimate ~1e-6 of the stage
    values), so another BLAS's float64 summation order moves it by up to ~1e-5 relative; 1e-3 is still ten times
    inside the 1 % band that ratios_clear_of_one keeps free around 1."""
    a, b = np.asarray(log, dtype=np.float64), np.asarray(recorded, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a[:, 3], b[:, 3])
    np.testing.assert_allclose(a[:, :2], b[:, :2], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(a[:, 2], b[:, 2], rtol=1e-3)
