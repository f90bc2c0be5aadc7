"""fp64 restatement of the plain fixed-step solves (euler, midpoint, rk4) of an MLP field and of their gradient, for the
tests of DifferentiableNeuralODE (a helper module imported by test files; not a conftest).

The field is the explicit layer chain of cnf_train_restate (z_l = W_{l-1} h_{l-1} + b, h_l = selu(z_l)).  The grid is
taken as the solvers take it: float32 points, h = tspan[n + 1] - tspan[n] and the stage times t_n + c_s h in float32
arithmetic; everything else is float64, the tableau entries included (cfm_amd.ode.FIXED_TABLEAUS; the kernels round them
to float32, 3e-8 relative on the two inexact ones of rk4, far below every bound the tests hold)."""
import numpy as np
import torch

from cfm_amd.ode import FIXED_TABLEAUS
from cnf_restate import min_abs_preactivation
from cnf_train_restate import ALPHA, SCALE, as_params, selu, selu_slope  # noqa: F401  (selu_slope: re-exported)

SCHEMES = ("euler", "midpoint", "rk4")


def grid_steps(ts, scheme):
    """Per step n: (h, [stage times]) as floats, computed in float32 as the solvers do."""
    ts = np.asarray(ts, np.float32)
    c = [np.float32(0.0)] + [np.float32(v) for v in FIXED_TABLEAUS[scheme]["c"]]
    out = []
    for n in range(len(ts) - 1):
        h = np.float32(ts[n + 1] - ts[n])
        out.append((float(h), [float(ts[n])] + [float(np.float32(ts[n] + cs * h)) for cs in c[1:]]))
    return out


def field(params, y, t):
    W = params[0::2]; b = params[1::2]
    h = torch.cat([y, torch.full_like(y[:, :1], float(t))], 1)
    for l in range(3):
        h = selu(h @ W[l].T + b[l])
    return h @ W[3].T + b[3]


def solve(params, x, ts, scheme, stage_points=False):
    """The trajectory [n_t, B, d] of the recurrence (a torch tensor; differentiable when params / x are).  With
    stage_points also the list of (t, Y) of every stage of every step."""
    tab = FIXED_TABLEAUS[scheme]
    rows = [[]] + [list(r) for r in tab["a"]]
    ys, pts = [x], []
    for h, tsg in grid_steps(ts, scheme):
        y, ks = ys[-1], []
        for s, t in enumerate(tsg):
            Y = y if s == 0 else y + h * sum(float(a) * k for a, k in zip(rows[s], ks))
            pts.append((t, Y))
            ks.append(field(params, Y, t))
        ys.append(y + h * sum(float(bq) * k for bq, k in zip(tab["b"], ks)))
    traj = torch.stack(ys)
    return (traj, pts) if stage_points else traj


def grads_for_upstream(Ws, bs, x, ts, G, scheme):
    """(trajectory, [dW0, db0, ..., dW3, db3], d/dx) of sum(G * trajectory) in float64 numpy, by autograd."""
    params = as_params(Ws, bs)
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    traj = solve(params, xt, ts, scheme)
    g = torch.autograd.grad((traj * torch.as_tensor(np.asarray(G, np.float64))).sum(), params + [xt], allow_unused=True)
    g = [torch.zeros_like(p) if q is None else q for p, q in zip(params + [xt], g)]
    return traj.detach().numpy(), [q.numpy() for q in g[:-1]], g[-1].numpy()


def reverse_sweep(Ws, bs, x, ts, G, scheme):
    """The reverse sweep the kernel runs, written out in float64 numpy without autograd: the stages
    forward from y_n, then per stage s = NS .. 1  kb_s = h (b_s lam + sum_{r>s} a_rs Yb_r) and one vector-Jacobian product.
    Returns ([dW0, db0, ..., dW3, db3], d/dx)."""
    W = [np.asarray(w, np.float64) for w in Ws]
    b = [np.asarray(v, np.float64) for v in bs]
    x, G = np.asarray(x, np.float64), np.asarray(G, np.float64)
    d = x.shape[1]
    tab = FIXED_TABLEAUS[scheme]
    a = [[]] + [list(r) for r in tab["a"]]
    bq = list(tab["b"])
    NS = len(bq)

    def hidden(Y, t):
        hs, s = [np.concatenate([Y, np.full((len(Y), 1), t)], 1)], []
        for l in range(3):
            z = hs[l] @ W[l].T + b[l]
            s.append(np.where(z > 0, SCALE, SCALE * ALPHA * np.exp(np.minimum(z, 0.0))))
            hs.append(np.where(z > 0, SCALE * z, SCALE * ALPHA * np.expm1(np.minimum(z, 0.0))))
        return hs, s

    def stages(y, h, tsg):
        Ys, hss, ss, ks = [], [], [], []
        for s in range(NS):
            Y = y if s == 0 else y + h * sum(a[s][q] * ks[q] for q in range(s))
            hs, sl = hidden(Y, tsg[s])
            Ys.append(Y); hss.append(hs); ss.append(sl)
            ks.append(hs[3] @ W[3].T + b[3])
        return Ys, hss, ss, ks

    steps = grid_steps(ts, scheme)
    ys = [x]
    for h, tsg in steps:
        ks = stages(ys[-1], h, tsg)[3]
        ys.append(ys[-1] + h * sum(bq[q] * ks[q] for q in range(NS)))
    lam = G[len(steps)].copy()
    dW, db = [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b]
    for n in reversed(range(len(steps))):
        h, tsg = steps[n]
        Ys, hss, ss, _ = stages(ys[n], h, tsg)
        Yb = [None] * NS
        for s in reversed(range(NS)):
            kb = h * (bq[s] * lam + sum(a[r][s] * Yb[r] for r in range(s + 1, NS)))
            dW[3] += kb.T @ hss[s][3]
            db[3] += kb.sum(0)
            hb = kb @ W[3]
            for l in (2, 1, 0):
                zb = hb * ss[s][l]
                dW[l] += zb.T @ hss[s][l]          # (column d of dW[0]: t_s * sum zb, since hs[0][:, d] = t_s)
                db[l] += zb.sum(0)
                hb = zb @ W[l]
            Yb[s] = hb[:, :d]
        lam = lam + sum(Yb) + G[n]
    return [g for pair in zip(dW, db) for g in pair], lam


def kink_free_rows(Ws, bs, x, ts, scheme, tol=1e-5):
    """Rows whose smallest hidden |z| over EVERY stage point of every step of the float64 solve stays >= tol (mask)."""
    with torch.no_grad():
        _, pts = solve(as_params(Ws, bs, False), torch.as_tensor(np.asarray(x, np.float64)), ts, scheme, stage_points=True)
    m = np.full(len(x), np.inf)
    for t, Y in pts:
        m = np.minimum(m, min_abs_preactivation(Ws, bs, t, Y.numpy()))
    return m >= tol
