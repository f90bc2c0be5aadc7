"""numpy float64 restatement of the ICNN optimal-transport objectives, written out sweep by sweep: the
forward, the transport map, both losses, the W2 means and every parameter gradient through the hand-derived formulas,
the g-step's double backward included.  tests/test_icnn_host.py pins it to float64 autograd through the reference's own
class (tests/golden/icnn_reference.json); tests/test_gpu_icnn.py measures the kernels against it.

Parameters are a dict under the state-dict names.  By levels l = 0 .. L-1 (0-based here):
    IN[0] = Wzs.0.weight, b[0] = Wzs.0.bias, IN[l] = Wxs.{l-1}.weight, b[l] = Wxs.{l-1}.bias, HZ[l-1] = Wzs.{l}.weight,
    wz = Wzs.L.weight[0], wx = Wxs.{L-1}.weight[0]
    a[0] = IN[0] x + b[0],  a[l] = HZ[l-1] h[l-1] + IN[l] x + b[l],  h[l] = sp(a[l]),  out = wz . h[L-1] + wx . x
Gradients come as per-row contributions summed in chunks, so that S = sum over rows of |row contribution| (the bound of
DESIGN.md 4.9) falls out of the same sweep.
"""
import numpy as np

THRESHOLD = 20.0
CHUNK = 256


def names(L):
    """state-dict keys in parameters() order"""
    out = ["Wzs.0.weight", "Wzs.0.bias"] + [f"Wzs.{l}.weight" for l in range(1, L + 1)]
    for l in range(L - 1):
        out += [f"Wxs.{l}.weight", f"Wxs.{l}.bias"]
    return out + [f"Wxs.{L - 1}.weight"]


def shapes(d, H, L):
    sh = {"Wzs.0.weight": (H, d), "Wzs.0.bias": (H,), f"Wzs.{L}.weight": (1, H), f"Wxs.{L - 1}.weight": (1, d)}
    for l in range(1, L):
        sh[f"Wzs.{l}.weight"] = (H, H)
        sh[f"Wxs.{l - 1}.weight"] = (H, d)
        sh[f"Wxs.{l - 1}.bias"] = (H,)
    return sh


def gen_params(seed, d, H, L, sign=0, scale=1.0):
    """seeded float64 parameters with both signs in Wzs (sign 0), or every Wzs entry negative (sign -1)"""
    rng = np.random.default_rng(seed)
    P = {}
    for k in names(L):
        sh = shapes(d, H, L)[k]
        fan = sh[-1] if len(sh) == 2 else H
        v = rng.standard_normal(sh) * scale / np.sqrt(max(fan, 1))
        if sign < 0 and k.startswith("Wzs.") and k.endswith(".weight"):
            v = -np.abs(v) - 0.01
        P[k] = v
    return P


def gen_data(seed, B, d, scale=1.0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, d)) * scale, rng.standard_normal((B, d)) * scale + 0.5


def unpack(P):
    L = sum(1 for k in P if k.startswith("Wzs.") and k.endswith(".weight")) - 1
    IN = [P["Wzs.0.weight"]] + [P[f"Wxs.{l}.weight"] for l in range(L - 1)]
    b = [P["Wzs.0.bias"]] + [P[f"Wxs.{l}.bias"] for l in range(L - 1)]
    HZ = [P[f"Wzs.{l}.weight"] for l in range(1, L)]
    return L, IN, b, HZ, P[f"Wzs.{L}.weight"][0], P[f"Wxs.{L - 1}.weight"][0]


def _pack(L, dIN, db, dHZ, dwz, dwx):
    G = {"Wzs.0.weight": dIN[0], "Wzs.0.bias": db[0], f"Wzs.{L}.weight": dwz[:, None, :], f"Wxs.{L - 1}.weight": dwx[:, None, :]}
    for l in range(1, L):
        G[f"Wzs.{l}.weight"] = dHZ[l - 1]
        G[f"Wxs.{l - 1}.weight"] = dIN[l]
        G[f"Wxs.{l - 1}.bias"] = db[l]
    return G


def softplus(z):
    return np.where(z > THRESHOLD, z, np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))))


def sigma(z):
    e = np.exp(-np.abs(z))
    r = 1.0 / (1.0 + e)
    return np.where(z > THRESHOLD, 1.0, np.where(z >= 0, r, e * r))


def sigma_slope(z):
    e = np.exp(-np.abs(z))
    r = 1.0 / (1.0 + e)
    return np.where(z > THRESHOLD, 0.0, r * (e * r))


def forward(P, x):
    """out [B], the pre-activations a[l] and the activations h[l]"""
    L, IN, b, HZ, wz, wx = unpack(P)
    a, h = [], []
    for l in range(L):
        z = x @ IN[l].T + b[l]
        if l > 0:
            z = h[l - 1] @ HZ[l - 1].T + z
        a.append(z)
        h.append(softplus(z))
    return h[-1] @ wz + x @ wx, a, h


def reverse(P, a):
    """ab[l] = s[l] * hb[l] with hb[L-1] = wz, hb[l-1] = ab[l] HZ[l-1]; also hb"""
    L, IN, b, HZ, wz, wx = unpack(P)
    ab, hbs = [None] * L, [None] * L
    hb = np.broadcast_to(wz, a[-1].shape)
    for l in range(L - 1, -1, -1):
        hbs[l] = hb
        ab[l] = sigma(a[l]) * hb
        if l > 0:
            hb = ab[l] @ HZ[l - 1]
    return ab, hbs


def transport(P, x, with_S=False):
    """grad_x out [B, d]; with_S: also the per-element sum of |layer summands|"""
    L, IN, b, HZ, wz, wx = unpack(P)
    _, a, _ = forward(P, x)
    ab, _ = reverse(P, a)
    terms = [ab[l] @ IN[l] for l in range(L)] + [np.broadcast_to(wx, x.shape)]
    g = sum(terms)
    return (g, sum(np.abs(t) for t in terms)) if with_S else g


def _rows_plain(P, x, c):
    """per-row contributions [rows, ...] of the plain backward of sum_r c_r out_r"""
    L, IN, b, HZ, wz, wx = unpack(P)
    _, a, h = forward(P, x)
    ab, _ = reverse(P, a)
    ab = [t * c[:, None] for t in ab]
    dIN = [ab[l][:, :, None] * x[:, None, :] for l in range(L)]
    db = list(ab)
    dHZ = [ab[l][:, :, None] * h[l - 1][:, None, :] for l in range(1, L)]
    return _pack(L, dIN, db, dHZ, c[:, None] * h[-1], c[:, None] * x)


def _rows_directional(P, y, w):
    """per-row contributions of the parameter gradient of sum_r w_r . grad_y out(y_r), w fixed"""
    L, IN, b, HZ, wz, wx = unpack(P)
    _, a, h = forward(P, y)
    s = [sigma(z) for z in a]
    q = [sigma_slope(z) for z in a]
    ab, hb = reverse(P, a)
    da, dh = [], []
    for l in range(L):
        t = w @ IN[l].T
        if l > 0:
            t = dh[l - 1] @ HZ[l - 1].T + t
        da.append(t)
        dh.append(s[l] * t)
    zeta = [None] * L
    ht = np.zeros_like(a[-1])
    for l in range(L - 1, -1, -1):
        zeta[l] = s[l] * ht + q[l] * da[l] * hb[l]
        if l > 0:
            ht = zeta[l] @ HZ[l - 1]
    dIN = [ab[l][:, :, None] * w[:, None, :] + zeta[l][:, :, None] * y[:, None, :] for l in range(L)]
    dHZ = [ab[l][:, :, None] * dh[l - 1][:, None, :] + zeta[l][:, :, None] * h[l - 1][:, None, :] for l in range(1, L)]
    return _pack(L, dIN, list(zeta), dHZ, dh[-1], w)


def _sum_rows(fn, B):
    """(sum over rows, sum over rows of |.|) of the per-row dicts fn(lo, hi), in chunks"""
    G, S = None, None
    for lo in range(0, B, CHUNK):
        R = fn(lo, min(B, lo + CHUNK))
        g = {k: v.sum(0) for k, v in R.items()}
        s = {k: np.abs(v).sum(0) for k, v in R.items()}
        G = g if G is None else {k: G[k] + g[k] for k in g}
        S = s if S is None else {k: S[k] + s[k] for k in s}
    return G, S


def penalty(P, reg):
    return reg * sum(np.sum(np.maximum(-v, 0.0) ** 2) / 2 for k, v in P.items() if k.startswith("Wzs.") and k.endswith(".weight"))


def _add_penalty(P, G, reg):
    for k in G:
        if reg > 0 and k.startswith("Wzs.") and k.endswith(".weight"):
            G[k] = G[k] - reg * np.maximum(-P[k], 0.0)
    return G


def f_step(Pf, Pg, x, y, reg):
    """loss_f, its gradient on f, S per tensor (largest per-element sum over rows of |row contribution| / B), and the
    mean of the summed |terms| of the loss"""
    B = x.shape[0]
    p = transport(Pg, y)
    fx, fp = forward(Pf, x)[0], forward(Pf, p)[0]
    one = np.ones(B)

    def rows(lo, hi):
        a_, b_ = _rows_plain(Pf, x[lo:hi], one[lo:hi]), _rows_plain(Pf, p[lo:hi], -one[lo:hi])
        return {k: a_[k] + b_[k] for k in a_}

    G, S = _sum_rows(rows, B)
    G = _add_penalty(Pf, {k: v / B for k, v in G.items()}, reg)
    pen = penalty(Pf, reg) if reg > 0 else 0.0
    return np.mean(fx - fp) + pen, G, {k: v.max() / B for k, v in S.items()}, np.mean(np.abs(fx) + np.abs(fp)) + pen


def g_step(Pf, Pg, x, y, reg):
    """loss_g, its gradient on g (f constant), S per tensor, the mean of the summed |terms|; also p and w"""
    B = y.shape[0]
    p = transport(Pg, y)
    fp = forward(Pf, p)[0]
    w = transport(Pf, p) - y
    yp = np.sum(y * p, 1)
    G, S = _sum_rows(lambda lo, hi: _rows_directional(Pg, y[lo:hi], w[lo:hi]), B)
    G = _add_penalty(Pg, {k: v / B for k, v in G.items()}, reg)
    pen = penalty(Pg, reg) if reg > 0 else 0.0
    return np.mean(fp - yp) + pen, G, {k: v.max() / B for k, v in S.items()}, np.mean(np.abs(fp) + np.abs(yp)) + pen, p, w


def w2(Pf, Pg, x, y):
    """(w2, f_loss, g_loss) of compute_w2 and the means of the summed |terms| of each"""
    p = transport(Pg, y)
    fx, fp = forward(Pf, x)[0], forward(Pf, p)[0]
    yp, xx, yy = np.sum(y * p, 1), np.sum(x * x, 1), np.sum(y * y, 1)
    vals = (np.mean(fp - fx - yp + 0.5 * xx + 0.5 * yy), np.mean(fx - fp), np.mean(fp - yp))
    mags = (np.mean(np.abs(fp) + np.abs(fx) + np.abs(yp) + 0.5 * xx + 0.5 * yy), np.mean(np.abs(fx) + np.abs(fp)),
            np.mean(np.abs(fp) + np.abs(yp)))
    return vals, mags


def golden_case():
    """the case of tests/golden/icnn_reference.json: d = 2, dimh = 8, L = 4, B = 6, both signs in Wzs"""
    d, H, L, B = 2, 8, 4, 6
    x, y = gen_data(5, B, d)
    return gen_params(3, d, H, L), gen_params(4, d, H, L), x, y, 0.1
