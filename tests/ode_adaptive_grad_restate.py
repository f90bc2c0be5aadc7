"""Restatement of the recurrence of ACCEPTED steps of an adaptive solve (dopri5, tsit5) of an MLP field and of its
gradient, for the tests of AdaptiveDifferentiableNeuralODE (a helper module imported by test files; not a conftest).

A step log [n_accepted, 4] of (t, dt, t_k1, out) is replayed: per step the six stages of the pair's tableau (row 6 of a is
b; the seventh slope feeds only the error estimate and the next step's k_1), k_1 at tsign * t_k1, stage s >= 2 at
tsign * (t + c dt) with that time formed in float32 as the solvers form it, the stage coefficient tsign * dt; the step end
is slice `out` of the trajectory when out >= 0.  Everything else is float64 (or the dtype of the inputs: the float32
replay measures what float32 arithmetic alone does to the gradient), the tableau entries included
(cfm_amd.ode.ADAPTIVE_TABLEAUS; the kernels round them to float32)."""
import functools

import numpy as np
import torch

from cfm_amd.ode import ADAPTIVE_TABLEAUS
from cnf_restate import min_abs_preactivation, mlp_params, smooth_mlp_params
from cnf_train_restate import ALPHA, SCALE, as_params
from ode_grad_restate import field

SOLVERS = ("dopri5", "tsit5")


def step_times(log, solver, tsign):
    """Per accepted step: (h, [the six field times]) as floats; h = tsign * dt, times in float32 arithmetic."""
    c = [np.float32(v) for v in ADAPTIVE_TABLEAUS[solver]["c"]]
    sg = np.float32(tsign)
    out = []
    for t, dt, tk1, _ in np.asarray(log, np.float64):
        t, dt, tk1 = np.float32(t), np.float32(dt), np.float32(tk1)
        out.append((float(sg * dt), [float(sg * tk1)] + [float(sg * np.float32(t + c[s] * dt)) for s in range(5)]))
    return out


def replay(params, x, log, n_t, solver, tsign, stage_points=False):
    """The trajectory [n_t, B, d] of the logged recurrence (a torch tensor in x's dtype; differentiable when params / x
    are).  With stage_points also the list of (field time, Y) of every stage of every step."""
    a = ADAPTIVE_TABLEAUS[solver]["a"]
    outs = [int(o) for o in np.asarray(log, np.float64)[:, 3]]
    traj, pts, y = [None] * n_t, [], x
    traj[0] = x
    for (h, times), out in zip(step_times(log, solver, tsign), outs):
        ks = []
        for s in range(6):
            Y = y if s == 0 else y + h * sum(float(aq) * k for aq, k in zip(a[s - 1], ks))
            pts.append((times[s], Y))
            ks.append(field(params, Y, times[s]))
        y = y + h * sum(float(aq) * k for aq, k in zip(a[5], ks))
        if out >= 0:
            traj[out] = y
    assert all(v is not None for v in traj), "the log does not land on every t_span point"
    traj = torch.stack(traj)
    return (traj, pts) if stage_points else traj


def grads_for_upstream(Ws, bs, x, log, G, solver, tsign, dtype=torch.float64):
    """(trajectory, [dW0, db0, ..., dW3, db3], d/dx) of sum(G * replay) as float64 numpy, by autograd in `dtype`."""
    params = [p.detach().to(dtype).requires_grad_(True) for p in as_params(Ws, bs, False)]
    xt = torch.tensor(np.asarray(x, np.float64)).to(dtype).requires_grad_(True)
    Gt = torch.as_tensor(np.asarray(G, np.float64)).to(dtype)
    traj = replay(params, xt, log, len(G), solver, tsign)
    g = torch.autograd.grad((traj * Gt).sum(), params + [xt], allow_unused=True)
    g = [torch.zeros_like(p) if q is None else q for p, q in zip(params + [xt], g)]
    return traj.detach().double().numpy(), [q.double().numpy() for q in g[:-1]], g[-1].double().numpy()


def reverse_sweep(Ws, bs, x, log, G, solver, tsign):
    """The reverse sweep the kernel runs, written out in float64 numpy without autograd: lam = 0; per step
    n = n_accepted - 1 .. 0: lam += G[out] (out >= 0), the stages forward from y_n, then per stage s = 6 .. 1
    kb_s = h (b_s lam + sum_{r>s} a_rs Yb_r) and one vector-Jacobian product, lam += sum Yb; at the end lam += G[0].
    Returns ([dW0, db0, ..., dW3, db3], d/dx)."""
    W = [np.asarray(w, np.float64) for w in Ws]
    b = [np.asarray(v, np.float64) for v in bs]
    x, G = np.asarray(x, np.float64), np.asarray(G, np.float64)
    d = x.shape[1]
    tab = ADAPTIVE_TABLEAUS[solver]
    a = [[]] + [list(r) for r in tab["a"][:5]]
    bq = list(tab["a"][5])
    NS = 6

    def hidden(Y, t):
        hs, s = [np.concatenate([Y, np.full((len(Y), 1), t)], 1)], []
        for l in range(3):
            z = hs[l] @ W[l].T + b[l]
            s.append(np.where(z > 0, SCALE, SCALE * ALPHA * np.exp(np.minimum(z, 0.0))))
            hs.append(np.where(z > 0, SCALE * z, SCALE * ALPHA * np.expm1(np.minimum(z, 0.0))))
        return hs, s

    def stages(y, h, times):
        Ys, hss, ss, ks = [], [], [], []
        for s in range(NS):
            Y = y if s == 0 else y + h * sum(a[s][q] * ks[q] for q in range(s))
            hs, sl = hidden(Y, times[s])
            Ys.append(Y); hss.append(hs); ss.append(sl)
            ks.append(hs[3] @ W[3].T + b[3])
        return Ys, hss, ss, ks

    steps = step_times(log, solver, tsign)
    outs = [int(o) for o in np.asarray(log, np.float64)[:, 3]]
    ys = [x]
    for h, times in steps:
        ks = stages(ys[-1], h, times)[3]
        ys.append(ys[-1] + h * sum(bq[q] * ks[q] for q in range(NS)))
    lam = np.zeros_like(x)
    dW, db = [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b]
    for n in reversed(range(len(steps))):
        h, times = steps[n]
        if outs[n] >= 0:
            lam = lam + G[outs[n]]
        Ys, hss, ss, _ = stages(ys[n], h, times)
        Yb = [None] * NS
        for s in reversed(range(NS)):
            kb = h * (bq[s] * lam + sum(a[r][s] * Yb[r] for r in range(s + 1, NS)))
            dW[3] += kb.T @ hss[s][3]
            db[3] += kb.sum(0)
            hb = kb @ W[3]
            for l in (2, 1, 0):
                zb = hb * ss[s][l]
                dW[l] += zb.T @ hss[s][l]          # (column d of dW[0]: time * sum zb, since hs[0][:, d] = the field time)
                db[l] += zb.sum(0)
                hb = zb @ W[l]
            Yb[s] = hb[:, :d]
        lam = lam + sum(Yb)
    return [g for pair in zip(dW, db) for g in pair], lam + G[0]


def kink_distance(Ws, bs, x, log, n_t, solver, tsign):
    """Per row: the smallest hidden |z| over EVERY stage point of every step of the float64 replay."""
    with torch.no_grad():
        _, pts = replay(as_params(Ws, bs, False), torch.as_tensor(np.asarray(x, np.float64)), log, n_t, solver, tsign,
                        stage_points=True)
    m = np.full(len(x), np.inf)
    for t, Y in pts:
        m = np.minimum(m, min_abs_preactivation(Ws, bs, t, Y.numpy()))
    return m


def float32_replay_ratio(Ws, bs, x, log, G, solver, tsign, rows=None):
    """What float32 arithmetic alone does to the gradient of a log: the float32 replay against the float64 one, the largest
    of max|g_32 - g_64| / max|g_64| over the eight parameter tensors and dx (dx over `rows` when given)."""
    _, gp64, gx64 = grads_for_upstream(Ws, bs, x, log, G, solver, tsign)
    _, gp32, gx32 = grads_for_upstream(Ws, bs, x, log, G, solver, tsign, dtype=torch.float32)
    if rows is not None:
        gx64, gx32 = gx64[rows], gx32[rows]
    return max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(gp32 + [gx32], gp64 + [gx64]))


# ---- the cases of tests/test_gpu_ode_adaptive_grad.py, shared with the CPU test that measures their float32 replay ------
BOX = 3.0
GPU_TOL = dict(atol=1e-6, rtol=1e-6)
W64 = (64, 64, 64)
# (d, hidden widths, B, t_span points)
GPU_SHAPES = [
    (2, W64, 48, 2),                # full tiles, endpoint grid
    (2, W64, 48, 9),                # full tiles, nine points: steps clamped onto the grid
    (5, (48, 48, 48), 19, 4),       # partial widths, partial tile
    (1, (16, 16, 16), 33, 4),       # d = 1
    (5, (33, 64, 48), 37, 4),       # non-square layers
    (63, (33, 33, 33), 17, 3),      # the time in column 63 of W0
]
STRIDE_SHAPE = (2, W64, 16 * 256 + 5, 3)      # more tiles than the backward has workgroups (CG_MAXGRID = 256), partial last tile


def streamed_shape(limit):
    """Just above `limit`, the rows the recording forward keeps in registers (8192 on the MI355X)."""
    return (2, (16, 16, 16), limit + 5, 2)


def grid(direction, n_t):
    w = 1.0 + 0.6 * np.sin(1.7 * np.arange(n_t - 1) + 0.3)          # 0 -> 1, non-uniform
    ts = np.concatenate([[0.0], np.cumsum(w) / w.sum()]).astype(np.float32)
    ts[-1] = 1.0
    return np.ascontiguousarray(ts[::-1]) if direction == "down" else ts


@functools.lru_cache(maxsize=None)
def smooth_case(shape, last_only=False, seed=1):
    """fp32 inputs of one case: a smooth net, states inside half its box, G.  Computed once, shared, never written to."""
    d, w, B, n_t = shape
    Ws, bs = smooth_mlp_params(d, w, seed, box=BOX)
    g = np.random.default_rng(seed)
    x = g.uniform(-1.5, 1.5, size=(B, d)).astype(np.float32)
    G = (0.5 + g.normal(size=(n_t, B, d))).astype(np.float32)
    if last_only:
        G[:-1] = 0.0
    for a in (x, G, *Ws, *bs):
        a.setflags(write=False)
    return Ws, bs, x, G


# The default-initialised net, per tableau: (seed, scale of the last layer, atol = rtol).  Chosen on the generic CPU path
# alone so that the controller rejects attempts and at most a quarter of the rows come within 1e-5 of a kink: dopri5
# rejects 2 of 8 attempts (controller ratios 1.04 and 1.22) and 7 of 48 rows do; tsit5 rejects 1 of 7 (ratio 2.25) and 9 do.
DEFAULT_NET = {"dopri5": (1, 16.0, 1e-4), "tsit5": (1, 16.0, 3e-4)}


def default_case(solver):
    """(Ws, bs, x, G, ts, tol) of the default-initialised case: d = 2, w = 64, B = 48, four points, increasing."""
    seed, scale, tol = DEFAULT_NET[solver]
    Ws, bs = mlp_params(2, 64, seed, out_scale=scale)
    g = np.random.default_rng(seed)
    x = g.normal(size=(48, 2)).astype(np.float32)
    G = (0.5 + g.normal(size=(4, 48, 2))).astype(np.float32)
    return Ws, bs, x, G, grid("up", 4), tol
