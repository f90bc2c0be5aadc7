"""CPU restatement of the action-matching field v = grad_x s(x, t) and its Laplacian (a helper module imported by test
files; not a conftest).

The action net s is Linear-SELU-Linear-SELU-Linear-SELU-Linear with dims [d + 1, n1, n2, n3, 1] (what
GradModel(MLP(dim=d, out_dim=1, time_varying=True)) differentiates: torchcfm/models/models.py:24-32).  grad_field below is
the float64 numpy statement of the sweeps the kernels run (csrc/grad_field.h), with no autograd in it; autograd_field is
torch.autograd through the same net, the independent reference of the CPU tests."""
import numpy as np
import torch

SCALE = 1.0507009873554805
ALPHA = 1.6732632423543772


def _selu(z):
    return np.where(z > 0, SCALE * z, SCALE * ALPHA * np.expm1(z))


def _slope(z):
    """selu'(z), the z = 0 side as elu_backward takes it"""
    return np.where(z > 0, SCALE, SCALE * ALPHA * np.exp(z))


def _curv(z):
    """selu''(z) as PyTorch's double backward takes it: the slope itself for z <= 0, else 0"""
    return np.where(z > 0, 0.0, SCALE * ALPHA * np.exp(z))


# ------------------------------------------------------------------------------------------------------ action nets
def action_params(d, widths, seed, out_scale=1.0):
    """Weights / biases (float32 numpy) of a seeded, default-initialised action net [d + 1, *widths, 1]; W3 scaled."""
    torch.manual_seed(seed)
    dims = [d + 1] + list(widths) + [1]
    lins = [torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])]
    Ws = [l.weight.detach().numpy().astype(np.float32).copy() for l in lins]
    bs = [l.bias.detach().numpy().astype(np.float32).copy() for l in lins]
    Ws[3] *= np.float32(out_scale)
    return Ws, bs


def smooth_action_params(d, w, seed, box=3.0, margin=0.2, out_scale=1.0):
    """A seeded action net whose hidden pre-activations are all negative (at most -margin) for x in [-box, box]^d and t
    in [-1, 1] (biases shifted down, layer by layer, from a dense sample of that box, as cnf_restate.smooth_mlp_params
    does for a field net; t covers both signs because a reverse solve evaluates the net at -s): SELU stays on its
    smooth branch, so v and the error estimate of an adaptive solve see no jump there."""
    Ws, bs = action_params(d, (w, w, w), seed, out_scale=out_scale)
    g = np.random.default_rng(seed)
    h = np.concatenate([g.uniform(-box, box, (8192, d)), g.uniform(-1.0, 1.0, (8192, 1))], 1)
    corners = np.array(np.meshgrid(*([[-box, box]] * d))).reshape(d, -1).T if d <= 6 else np.zeros((0, d))
    for tc in (-1.0, 0.0, 1.0):
        h = np.concatenate([h, np.concatenate([corners, np.full((len(corners), 1), tc)], 1)], 0)
    for l in range(3):
        z = h @ Ws[l].astype(np.float64).T + bs[l].astype(np.float64)
        bs[l] = (bs[l] - (z.max(0) + margin)).astype(np.float32)
        z = h @ Ws[l].astype(np.float64).T + bs[l].astype(np.float64)
        h = _selu(z)
    return Ws, bs


def negated_action_params(Ws, bs):
    """The action net whose time column (W0[:, d]) and last layer are negated: its gradient field is -v(-t, x), bit
    for bit."""
    d = Ws[0].shape[1] - 1
    Wn = [W.copy() for W in Ws]; bn = [b.copy() for b in bs]
    Wn[0][:, d] = -Wn[0][:, d]
    Wn[3] = -Wn[3]; bn[3] = -bn[3]
    return Wn, bn


def make_action(Ws, bs, device=None, dtype=torch.float32):
    """cfm_amd.MLP(dim=d, out_dim=1, time_varying=True) carrying these layers (any hidden widths)."""
    import cfm_amd
    d = Ws[0].shape[1] - 1
    m = cfm_amd.MLP(dim=d, out_dim=1, w=Ws[0].shape[0], time_varying=True)
    k = 0
    for idx, mod in enumerate(m.net):
        if isinstance(mod, torch.nn.Linear):
            lin = torch.nn.Linear(Ws[k].shape[1], Ws[k].shape[0])
            lin.weight.data = torch.from_numpy(np.ascontiguousarray(Ws[k])).to(dtype)
            lin.bias.data = torch.from_numpy(np.ascontiguousarray(bs[k])).to(dtype)
            m.net[idx] = lin
            k += 1
    return m.to(device) if device is not None else m


# ------------------------------------------------------------------------------------------------------ the field
def _forward(Ws, bs, t, x):
    d = Ws[0].shape[1] - 1
    W = [np.asarray(w, np.float64) for w in Ws]
    b = [np.asarray(v, np.float64) for v in bs]
    x = np.asarray(x, np.float64)
    z1 = x @ W[0][:, :d].T + float(t) * W[0][:, d] + b[0]
    z2 = _selu(z1) @ W[1].T + b[1]
    z3 = _selu(z2) @ W[2].T + b[2]
    return W, (z1, z2, z3)


def grad_field(Ws, bs, t, x, laplacian=False):
    """v [B, d] (and lap [B] = tr dv/dx) of the float64 action net at rows x [B, d] and scalar t: a forward sweep, a
    reverse sweep, and per direction k the tangent of both."""
    d = Ws[0].shape[1] - 1
    W, (z1, z2, z3) = _forward(Ws, bs, t, x)
    s1, s2, s3 = _slope(z1), _slope(z2), _slope(z3)
    g3 = s3 * W[3][0]
    hb2 = g3 @ W[2]
    g2 = s2 * hb2
    hb1 = g2 @ W[1]
    g1 = s1 * hb1
    v = g1 @ W[0][:, :d]
    if not laplacian:
        return v
    q1, q2, q3 = _curv(z1), _curv(z2), _curv(z3)
    lap = np.zeros(len(v))
    for k in range(d):
        dz1 = W[0][:, k][None]
        dz2 = (s1 * dz1) @ W[1].T
        dz3 = (s2 * dz2) @ W[2].T
        dg3 = W[3][0] * q3 * dz3
        dg2 = s2 * (dg3 @ W[2]) + hb2 * q2 * dz2
        dg1 = s1 * (dg2 @ W[1]) + hb1 * q1 * dz1
        lap += dg1 @ W[0][:, k]
    return v, lap


def laplacian_terms(Ws, bs, t, x):
    """Per row: (sum_k |H_kk|, sum_k of the magnitudes of the terms whose sum is H_kk), H the Hessian of s in x.  The
    second is the scale of fp32 rounding in the Laplacian: the sweeps above with every weight and every intermediate
    replaced by its absolute value (slopes and curvatures are positive), so an entry that cancels to far below its terms
    is held to the terms' rounding, as cnf_restate.abs_jacobian does for tr J."""
    d = Ws[0].shape[1] - 1
    W, (z1, z2, z3) = _forward(Ws, bs, t, x)
    Wa = [np.abs(w) for w in W]
    s1, s2, s3 = _slope(z1), _slope(z2), _slope(z3)
    q1, q2, q3 = _curv(z1), _curv(z2), _curv(z3)
    hb2 = (s3 * W[3][0]) @ W[2]
    hb1 = (s2 * hb2) @ W[1]
    ahb2 = (s3 * Wa[3][0]) @ Wa[2]
    ahb1 = (s2 * ahb2) @ Wa[1]
    diag = np.zeros(len(z1)); mag = np.zeros(len(z1))
    for k in range(d):
        dz1 = W[0][:, k][None]
        dz2 = (s1 * dz1) @ W[1].T
        dz3 = (s2 * dz2) @ W[2].T
        dg2 = s2 * ((W[3][0] * q3 * dz3) @ W[2]) + hb2 * q2 * dz2
        dg1 = s1 * (dg2 @ W[1]) + hb1 * q1 * dz1
        diag += np.abs(dg1 @ W[0][:, k])
        az1 = Wa[0][:, k][None]
        az2 = (s1 * az1) @ Wa[1].T
        az3 = (s2 * az2) @ Wa[2].T
        ag2 = s2 * ((Wa[3][0] * q3 * az3) @ Wa[2]) + ahb2 * q2 * az2
        ag1 = s1 * (ag2 @ Wa[1]) + ahb1 * q1 * az1
        mag += ag1 @ Wa[0][:, k]
    return diag, mag


def min_abs_preactivation(Ws, bs, t, x):
    """Per row: the smallest |z| over the hidden pre-activations (float64).  selu' jumps at z = 0 from 1.758 to 1.051,
    so v itself is discontinuous there: an fp32 evaluation within rounding of a kink may take either side."""
    _, zs = _forward(Ws, bs, t, x)
    return np.minimum.reduce([np.abs(z).min(1) for z in zs])


def field_np(Ws, bs):
    """float64 numpy f(t, y) of torch_wrapper(GradModel(action)) on a [B, d] state."""
    return lambda t, y: grad_field(Ws, bs, t, y)


def aug_field_np(Ws, bs):
    """The float64 augmented field of a [B, 1 + d] state in the layout of the reference's CNF: column 0 carries
    -tr(dv/dx) = -lap s, columns 1.. carry v."""
    def F(t, Y):
        Y = np.asarray(Y, np.float64)
        v, lap = grad_field(Ws, bs, t, Y[:, 1:], laplacian=True)
        return np.concatenate([-lap[:, None], v], 1)
    return F


class KinkWatch:
    """Wraps a float64 field of an integrator and records, per row, the smallest |pre-activation| over every point the
    integrator evaluates it at (the stage points of the solve): rows with clear(1e-5) False came within reach of a
    kink somewhere along the solve.  aug: the state is [B, 1 + d]."""

    def __init__(self, Ws, bs, f, aug=False):
        self.Ws, self.bs, self.f, self.aug, self.m = Ws, bs, f, aug, None

    def __call__(self, t, y):
        yy = np.asarray(y, np.float64)
        m = min_abs_preactivation(self.Ws, self.bs, t, yy[:, 1:] if self.aug else yy)
        self.m = m if self.m is None else np.minimum(self.m, m)
        return self.f(t, y)

    def clear(self, margin=1e-5):
        return self.m > margin


# ------------------------------------------------------------------------------------------------------ autograd
def autograd_field(Ws, bs, t, x, laplacian=False):
    """The same quantities by torch.autograd through the float64 action net (independent of grad_field)."""
    W = [torch.from_numpy(np.asarray(w, np.float64)) for w in Ws]
    b = [torch.from_numpy(np.asarray(v, np.float64)) for v in bs]
    x = torch.from_numpy(np.asarray(x, np.float64)).clone().requires_grad_(True)
    h = torch.cat([x, torch.full((x.shape[0], 1), float(t), dtype=torch.float64)], 1)
    for l in range(4):
        h = torch.nn.functional.linear(h, W[l], b[l])
        if l < 3:
            h = torch.nn.functional.selu(h)
    (v,) = torch.autograd.grad(h.sum(), x, create_graph=True)
    if not laplacian:
        return v.detach().numpy()
    lap = torch.zeros(x.shape[0], dtype=torch.float64)
    for k in range(x.shape[1]):
        (gk,) = torch.autograd.grad(v[:, k].sum(), x, retain_graph=True)
        lap = lap + gk[:, k]
    return v.detach().numpy(), lap.numpy()
