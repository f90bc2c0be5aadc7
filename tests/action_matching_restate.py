"""CPU restatement of the action-matching loss and its parameter gradient (a helper module imported by test files; not
a conftest).

The action net s is Linear-SELU-Linear-SELU-Linear-SELU-Linear with dims [d + 1, n1, n2, n3, 1].  Per row
    l = s(x0, 0) - s(x1, 1) + 1/2 |grad_x s(xt, t)|^2 + d/dt s(xt, t),      loss = mean l
(ActionMatchingLitModule.step, runner/src/models/cfm_module.py:670-694).  `sweeps` is the float64 numpy statement of what
csrc/action_grad.h runs, with no autograd in it: two plain backwards at the endpoints and, at the interior point, the
primal forward, the reverse sweep, the tangent of the chain along w = (g_x, 1) and the second-order pull-backs zeta_l.
`autograd_loss_and_grads` is torch.autograd on the reference's formulation, the independent reference of the CPU
tests."""
import numpy as np
import torch

from grad_field_restate import _curv, _selu, _slope, action_params, make_action  # noqa: F401

NAMES = ["dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3"]
WIDTHS = [(64, 64, 64), (33, 33, 33), (64, 17, 40)]


def _f64(Ws, bs):
    return [np.asarray(w, np.float64) for w in Ws], [np.asarray(v, np.float64) for v in bs]


def _chain(W, b, u):
    """z_l and h_l (h_0 = u) of the three hidden layers, and the value s [B]"""
    h, zs = [u], []
    for l in range(3):
        zs.append(h[-1] @ W[l].T + b[l])
        h.append(_selu(zs[-1]))
    return zs, h, h[3] @ W[3][0] + b[3][0]


def _pairs(W, b, x0, x1, xt, t):
    """Per row: the loss terms, and for each of the eight tensors a list of factor pairs (Z [B, n], H [B, k]) such that
    the tensor's gradient is sum_pairs Z^T H / B; row r contributes sum_pairs outer(Z[r], H[r]) / B."""
    B, d = x0.shape
    one = np.ones((B, 1))
    pairs = [[] for _ in range(8)]
    # ---- the endpoints: a plain backward with cotangent c ----
    ends = []
    for x, tc, c in ((x0, 0.0, 1.0), (x1, 1.0, -1.0)):
        zs, h, s = _chain(W, b, np.concatenate([x, np.full((B, 1), tc)], 1))
        ends.append(s)
        pairs[6].append((c * one, h[3]))
        hb = c * one * W[3]                                    # [B, n3]
        for l in (3, 2, 1):
            zb = hb * _slope(zs[l - 1])
            pairs[2 * (l - 1)].append((zb, h[l - 1]))
            pairs[2 * (l - 1) + 1].append((zb, one))
            hb = zb @ W[l - 1]
    # ---- the interior point ----
    u = np.concatenate([xt, t.reshape(B, 1)], 1)
    zs, h, _ = _chain(W, b, u)
    s1, s2, s3 = (_slope(z) for z in zs)
    q1, q2, q3 = (_curv(z) for z in zs)
    g3 = s3 * W[3][0]
    hb2 = g3 @ W[2]
    g2 = s2 * hb2
    hb1 = g2 @ W[1]
    g1 = s1 * hb1
    g = g1 @ W[0]                                              # [B, d + 1]: g_x and g_t
    gx, gt = g[:, :d], g[:, d]
    w = np.concatenate([gx, one], 1)
    dz1 = w @ W[0].T
    dh1 = s1 * dz1
    dz2 = dh1 @ W[1].T
    dh2 = s2 * dz2
    dz3 = dh2 @ W[2].T
    dh3 = s3 * dz3
    zeta3 = W[3][0] * q3 * dz3
    zeta2 = s2 * (zeta3 @ W[2]) + hb2 * q2 * dz2
    zeta1 = s1 * (zeta2 @ W[1]) + hb1 * q1 * dz1
    pairs[6].append((one, dh3))
    pairs[4] += [(g3, dh2), (zeta3, h[2])]
    pairs[5].append((zeta3, one))
    pairs[2] += [(g2, dh1), (zeta2, h[1])]
    pairs[3].append((zeta2, one))
    pairs[0] += [(g1, w), (zeta1, u)]
    pairs[1].append((zeta1, one))
    terms = (ends[0], ends[1], 0.5 * (gx * gx).sum(1), gt)
    return terms, pairs


def sweeps(Ws, bs, x0, x1, xt, t, scales=False):
    """loss and [dW0, db0, ..., dW3, db3] in float64 (db3 an exact 0).  With scales: also the scale of the loss's
    rounding, mean over the rows of |s(x0, 0)| + |s(x1, 1)| + 1/2 |g_x|^2 + |g_t|, and per tensor S, the sum over the
    rows of |the row's contribution| to each element."""
    W, b = _f64(Ws, bs)
    x0, x1, xt, t = (np.asarray(v, np.float64) for v in (x0, x1, xt, t))
    B = len(x0)
    (a0, a1, half, gt), pairs = _pairs(W, b, x0, x1, xt, t)
    loss = float(np.mean(a0 - a1 + half + gt))
    grads = []
    for k in range(7):
        g = sum(Z.T @ H for Z, H in pairs[k]) / B
        grads.append(g.reshape(np.shape(Ws[k // 2]) if k % 2 == 0 else np.shape(bs[k // 2])))
    grads.append(np.zeros(np.shape(bs[3])))
    if not scales:
        return loss, grads
    lscale = float(np.mean(np.abs(a0) + np.abs(a1) + half + np.abs(gt)))
    S = []
    for k in range(7):
        acc = 0.0
        for r0 in range(0, B, 128):
            sl = slice(r0, r0 + 128)
            acc = acc + np.abs(sum(Z[sl, :, None] * H[sl, None, :] for Z, H in pairs[k])).sum(0)
        S.append((acc / B).reshape(grads[k].shape))
    S.append(np.zeros_like(grads[7]))
    return loss, grads, lscale, S


def restated_loss(Ws, bs, x0, x1, xt, t):
    W, b = _f64(Ws, bs)
    x0, x1, xt, t = (np.asarray(v, np.float64) for v in (x0, x1, xt, t))
    (a0, a1, half, gt), _ = _pairs(W, b, x0, x1, xt, t)
    return float(np.mean(a0 - a1 + half + gt))


def min_abs_preactivation(Ws, bs, x0, x1, xt, t):
    """Per row: the smallest |z| over the hidden pre-activations of the three evaluation points (float64)."""
    W, b = _f64(Ws, bs)
    x0, x1, xt, t = (np.asarray(v, np.float64) for v in (x0, x1, xt, t))
    B = len(x0)
    m = np.full(B, np.inf)
    for u in (np.concatenate([x0, np.zeros((B, 1))], 1), np.concatenate([x1, np.ones((B, 1))], 1),
              np.concatenate([xt, t.reshape(B, 1)], 1)):
        for z in _chain(W, b, u)[0]:
            m = np.minimum(m, np.abs(z).min(1))
    return m


def draw(B, d, seed, ends=False):
    """x0 ~ 1.5 N(0, I), x1 ~ N(0.5, I), t ~ U[0, 1] as float32 (ends: the first row at t = 0, the second at t = 1) and
    the reference's interpolant xt, computed in float32 in the reference's operation order."""
    g = np.random.default_rng(seed)
    x0 = (1.5 * g.normal(size=(B, d))).astype(np.float32)
    x1 = (0.5 + g.normal(size=(B, d))).astype(np.float32)
    t = g.uniform(size=B).astype(np.float32)
    if ends:
        t[0], t[1] = 0.0, 1.0
    xt = t[:, None] * x1 + (np.float32(1) - t[:, None]) * x0
    return x0, x1, t, xt.astype(np.float32)


def kink_free(Ws, bs, x0, x1, xt, t, tol=1e-5):
    return min_abs_preactivation(Ws, bs, x0, x1, xt, t) > tol


def autograd_loss_and_grads(Ws, bs, x0, x1, xt, t):
    """The reference's formulation (cfm_module.py:686-694) under torch.autograd in float64: loss, eight gradients."""
    W = [torch.from_numpy(np.asarray(w, np.float64)).clone().requires_grad_(True) for w in Ws]
    b = [torch.from_numpy(np.asarray(v, np.float64)).clone().requires_grad_(True) for v in bs]

    def energy(h):
        for l in range(4):
            h = torch.nn.functional.linear(h, W[l], b[l])
            if l < 3:
                h = torch.nn.functional.selu(h)
        return h

    x0, x1, xt = (torch.from_numpy(np.asarray(v, np.float64)) for v in (x0, x1, xt))
    tt = torch.from_numpy(np.asarray(t, np.float64)).reshape(-1, 1)
    xt = xt.clone().requires_grad_(True)
    tt = tt.clone().requires_grad_(True)
    st = torch.sum(energy(torch.cat([xt, tt], dim=-1)))
    dsdx, dsdt = torch.autograd.grad(st, (xt, tt), create_graph=True)
    a0 = energy(torch.cat([x0, torch.zeros(x0.shape[0], 1, dtype=torch.float64)], dim=-1))
    a1 = energy(torch.cat([x1, torch.ones(x1.shape[0], 1, dtype=torch.float64)], dim=-1))
    loss = (a0 - a1 + 0.5 * (dsdx ** 2).sum(1, keepdims=True) + dsdt).mean()
    ps = [p for l in range(4) for p in (W[l], b[l])]
    got = torch.autograd.grad(loss, ps, allow_unused=True)
    return float(loss.detach()), [None if q is None else q.numpy() for q in got]
