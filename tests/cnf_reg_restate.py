"""fp64 restatement of the regularised CNF solve (state [l, (e), (f), y]) and a written-out reverse sweep of it, for the
regularised-CNF tests (a helper module imported by test files; not a conftest).

The field is the explicit layer chain of cnf_train_restate.py with the two penalties' integrands added:
|v|^2 (SquaredL2Reg) and ||J||_F / d (JacobianFrobeniusReg), J e_k = W_3 T_3^k.  reg_mask: bit 0 = e, bit 1 = f."""
import numpy as np
import torch

import cnf_train_restate as tr

SCALE, ALPHA = tr.SCALE, tr.ALPHA


def n_reg(mask):
    return (mask & 1) + (mask >> 1 & 1)


def field_all(params, y, t, eps=None):
    """(v, div, |v|^2, ||J||_F / d) at (y [B, d], t); div = tr J (eps None) or eps^T J eps; J by the explicit tangents."""
    W = params[0::2]; b = params[1::2]
    d = y.shape[1]
    h = torch.cat([y, torch.full_like(y[:, :1], float(t))], 1)
    s = []
    for l in range(3):
        z = h @ W[l].T + b[l]
        s.append(tr.selu_slope(z))
        h = tr.selu(z)
    v = h @ W[3].T + b[3]
    cols = []
    for k in range(d):
        T = s[0] * W[0][:, k]
        T = s[1] * (T @ W[1].T)
        T = s[2] * (T @ W[2].T)
        cols.append(T @ W[3].T)                      # J e_k  [B, d]
    J = torch.stack(cols, 2)                         # J[b, i, k]
    if eps is None:
        div = torch.diagonal(J, dim1=1, dim2=2).sum(1)
    else:
        div = torch.einsum("bi,bik,bk->b", eps, J, eps)
    return v, div, (v * v).sum(1), torch.norm(J.reshape(len(y), -1), p=2, dim=1) / d


def euler_solve(params, x_aug, ts, mask, eps=None, trajectory=False):
    """The final state [l, (e), (f), y] over the grid ts (floats, either direction)."""
    r = n_reg(mask)
    cols = [x_aug[:, k] for k in range(1 + r)]
    y = x_aug[:, 1 + r:]
    ys, fmin = [y], None
    for n in range(len(ts) - 1):
        h = float(ts[n + 1]) - float(ts[n])
        v, div, e, f = field_all(params, y, float(ts[n]), eps)
        cols[0] = cols[0] - h * div
        k = 1
        if mask & 1:
            cols[k] = cols[k] + h * e
            k += 1
        if mask & 2:
            cols[k] = cols[k] + h * f
        fmin = f.detach() if fmin is None else torch.minimum(fmin, f.detach())
        y = y + h * v
        ys.append(y)
    out = torch.cat([torch.stack(cols, 1), y], 1)
    return (out, ys, fmin) if trajectory else out


def grads_for_upstream(Ws, bs, x_aug, ts, G, mask, eps=None, dtype=np.float64):
    """(final state, [dW0, db0, ..., dW3, db3], d/dx_aug) of sum(G * solve) by autograd through the restatement, in
    `dtype` (float64: the reference; float32: torch's own fp32 figure for a case)."""
    tt = torch.float64 if dtype == np.float64 else torch.float32
    params = [p.to(tt).detach().requires_grad_(True) for p in tr.as_params(Ws, bs, False)]
    xa = torch.tensor(np.asarray(x_aug, dtype), requires_grad=True)
    e = None if eps is None else torch.tensor(np.asarray(eps, dtype))
    out = euler_solve(params, xa, ts, mask, e)
    g = torch.autograd.grad((out * torch.as_tensor(np.asarray(G, dtype))).sum(), params + [xa], allow_unused=True)
    g = [torch.zeros_like(p) if q is None else q for p, q in zip(params + [xa], g)]
    return out.detach().numpy(), [q.numpy() for q in g[:-1]], g[-1].numpy()


def usable_rows(Ws, bs, x_aug, ts, mask, eps=None, tol=1e-5):
    """(mask of rows to keep, smallest ||J||_F / d met): rows whose hidden |z| stays >= tol along the float64 trajectory
    (a SELU kink) and whose ||J||_F / d stays >= tol (the kink of the norm at J = 0)."""
    from cnf_restate import min_abs_preactivation
    with torch.no_grad():
        _, ys, fmin = euler_solve(tr.as_params(Ws, bs, False), torch.as_tensor(np.asarray(x_aug, np.float64)), ts, mask,
                                  None if eps is None else torch.as_tensor(np.asarray(eps, np.float64)), trajectory=True)
    m = np.full(len(x_aug), np.inf)
    for n in range(len(ts) - 1):
        m = np.minimum(m, min_abs_preactivation(Ws, bs, float(ts[n]), ys[n].numpy()))
    fmin = fmin.numpy() if fmin is not None else np.full(len(x_aug), np.inf)
    return (m >= tol) & (fmin >= tol), float(fmin.min())


# ---- the reverse sweep, written out in numpy (the kernel's algorithm: DESIGN.md 4.13) ----------------------------------
def _selu(z):
    return np.where(z > 0, SCALE * z, SCALE * ALPHA * np.expm1(np.minimum(z, 0.0)))


def _slope(z):
    return np.where(z > 0, SCALE, SCALE * ALPHA * np.exp(np.minimum(z, 0.0)))


def reverse_sweep(Ws, bs, x_aug, ts, G, mask, eps=None):
    """([dW0, db0, ..., dW3, db3], d/dx_aug) of sum(G * solve) by the seeds of the issue: per step g = a.v - c tr J +
    ce |v|^2 + cf sqrt(S)/d; output cotangent h (a + 2 ce v); direction cotangent h (-c w_k + cf J_k / (d sqrt(S)))."""
    W = [np.asarray(w, np.float64) for w in Ws]; b = [np.asarray(q, np.float64) for q in bs]
    x_aug = np.asarray(x_aug, np.float64); G = np.asarray(G, np.float64)
    r = n_reg(mask)
    B, d = len(x_aug), x_aug.shape[1] - 1 - r
    ys = [x_aug[:, 1 + r:]]
    for n in range(len(ts) - 1):                                   # forward: the checkpoints y_n
        hcat = np.concatenate([ys[-1], np.full((B, 1), float(ts[n]))], 1)
        for l in range(3):
            hcat = _selu(hcat @ W[l].T + b[l])
        ys.append(ys[-1] + (float(ts[n + 1]) - float(ts[n])) * (hcat @ W[3].T + b[3]))
    c = G[:, 0]
    ce = G[:, 1] if mask & 1 else np.zeros(B)
    cf = G[:, 1 + (mask & 1)] if mask & 2 else np.zeros(B)
    a = G[:, 1 + r:].copy()
    dW = [np.zeros_like(w) for w in W]; db = [np.zeros_like(q) for q in b]
    for n in range(len(ts) - 2, -1, -1):
        t, h = float(ts[n]), float(ts[n + 1]) - float(ts[n])
        y = ys[n]
        hs = [np.concatenate([y, np.full((B, 1), t)], 1)]
        s, q = [], []
        for l in range(3):
            z = hs[-1] @ W[l].T + b[l]
            s.append(_slope(z)); q.append(np.where(z > 0, 0.0, _slope(z)))
            hs.append(_selu(z))
        v = hs[3] @ W[3].T + b[3]
        # tangents of every direction
        dirs = [(np.eye(d)[k][None].repeat(B, 0), None) for k in range(d)] if eps is None else [(np.asarray(eps, np.float64), None)]
        U, T = [], []
        for tau, _ in dirs:
            Uk, Tk = [], [np.concatenate([tau, np.zeros((B, 1))], 1)]
            for l in range(3):
                Uk.append(Tk[-1] @ W[l].T)
                Tk.append(s[l] * Uk[-1])
            U.append(Uk); T.append(Tk)
        Jc = [Tk[3] @ W[3].T for Tk in T]                          # J tau_k  [B, d]
        S = sum((j * j).sum(1) for j in Jc) if eps is None else None
        sb = [np.zeros_like(x) for x in s]
        for k, (tau, _) in enumerate(dirs):
            Jb = -(h * c)[:, None] * tau                           # w_k = tau_k (e_k, or eps)
            if mask & 2:
                rs = np.where(S > 0, h * cf / (d * np.sqrt(np.where(S > 0, S, 1.0))), 0.0)
                Jb = Jb + rs[:, None] * Jc[k]
            dW[3] += Jb.T @ T[k][3]
            Tb = Jb @ W[3]
            for l in (2, 1, 0):
                sb[l] += Tb * U[k][l]
                Ub = s[l] * Tb
                dW[l] += Ub.T @ T[k][l]
                Tb = Ub @ W[l]
        vb = h * (a + 2.0 * ce[:, None] * v)
        dW[3] += vb.T @ hs[3]; db[3] += vb.sum(0)
        hb = vb @ W[3]
        for l in (2, 1, 0):
            zb = hb * s[l] + sb[l] * q[l]
            dW[l] += zb.T @ hs[l]; db[l] += zb.sum(0)
            hb = zb @ W[l]
        a = a + hb[:, :d]
    gx = np.concatenate([G[:, :1 + r], a], 1)
    out = []
    for w, q in zip(dW, db):
        out += [w, q]
    return out, gx
