"""CPU restatements for the CNF / reverse-time tests (a helper module imported by test files; not a conftest).

Builds on oracle/cfm_oracle.py: its integrators (euler_trajectory, dopri5_trajectory) take any f(t, y) on a
[B, D] state, and mlp_field_torch gives torch_wrapper(MLP) in float64."""
import numpy as np
import torch

import cfm_oracle as oracle


def mlp_params(d, w, seed, out_scale=1.0):
    """Weights / biases (float32 numpy) of a seeded, default-initialised field net; last layer scaled.  w an int: the
    layers of MLP(dim=d, time_varying=True, w=w); w a triple of hidden widths: the Linear layers [d + 1, *w, d] created
    in order under the seed (as grad_field_restate.action_params does for an action net)."""
    torch.manual_seed(seed)
    if isinstance(w, (int, np.integer)):
        import cfm_amd
        lins = cfm_amd.MLP(dim=d, time_varying=True, w=w)._linears()
    else:
        dims = [d + 1] + [int(n) for n in w] + [d]
        assert len(dims) == 5, w
        lins = [torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])]
    Ws = [l.weight.detach().numpy().astype(np.float32).copy() for l in lins]
    bs = [l.bias.detach().numpy().astype(np.float32).copy() for l in lins]
    Ws[3] *= np.float32(out_scale); bs[3] *= np.float32(out_scale)
    return Ws, bs


def smooth_mlp_params(d, w, seed, box=3.0, margin=0.2, out_scale=1.0):
    """A seeded MLP whose hidden pre-activations are all negative (at most -margin) for x in [-box, box]^d and t in
    [0, 1] (biases shifted down, layer by layer, from a dense sample of that box): SELU stays on its smooth branch,
    so tr J has no jump there and l is as well resolved by an adaptive solve as x."""
    Ws, bs = mlp_params(d, w, seed, out_scale=out_scale)
    g = np.random.default_rng(seed)
    h = np.concatenate([g.uniform(-box, box, (8192, d)), g.uniform(0.0, 1.0, (8192, 1))], 1)
    corners = np.array(np.meshgrid(*([[-box, box]] * d))).reshape(d, -1).T if d <= 6 else np.zeros((0, d))
    for tc in (0.0, 1.0):
        h = np.concatenate([h, np.concatenate([corners, np.full((len(corners), 1), tc)], 1)], 0)
    for l in range(3):
        z = h @ Ws[l].astype(np.float64).T + bs[l].astype(np.float64)
        bs[l] = (bs[l] - (z.max(0) + margin)).astype(np.float32)
        z = h @ Ws[l].astype(np.float64).T + bs[l].astype(np.float64)
        h = 1.0507009873554805 * 1.6732632423543772 * np.expm1(z)
    return Ws, bs


def make_mlp(Ws, bs, device=None, dtype=torch.float32):
    """cfm_amd.MLP(dim=d, time_varying=True) carrying these layers (any hidden widths): every Linear of MLP.net is given
    the shaped parameters and its in / out extents."""
    import cfm_amd
    d = Ws[3].shape[0]
    m = cfm_amd.MLP(dim=d, time_varying=True, w=Ws[0].shape[0])
    lins = m._linears()
    assert len(lins) == 4
    for k, l in enumerate(lins):
        l.out_features, l.in_features = Ws[k].shape
        l.weight = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(Ws[k])).to(dtype))
        l.bias = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(bs[k])).to(dtype))
    return m.to(device) if device is not None else m


def negated_mlp_params(Ws, bs):
    """The MLP whose time column (W0[:, d]) and last layer are negated: its field is -f(-t, x), bit for bit."""
    d = Ws[3].shape[0]
    Wn = [W.copy() for W in Ws]; bn = [b.copy() for b in bs]
    Wn[0][:, d] = -Wn[0][:, d]
    Wn[3] = -Wn[3]; bn[3] = -bn[3]
    return Wn, bn


def reverse(f):
    """torchdyn's reverse-time field: g(s, y) = -f(-s, y)."""
    return lambda s, y: -f(-s, y)


def mlp_field_np(Ws, bs):
    """float64 numpy f(t, y) of torch_wrapper(MLP)."""
    f = oracle.mlp_field_torch(Ws, bs)
    return lambda t, y: f(t, torch.from_numpy(np.asarray(y, dtype=np.float64))).numpy()


def divergence_f64(Ws, bs, t, y, eps=None):
    """tr(df/dx) (eps None) or eps^T (df/dx) eps of the float64 MLP field, by torch.func.jacrev."""
    f = oracle.mlp_field_torch(Ws, bs)
    y = torch.as_tensor(np.asarray(y, dtype=np.float64))
    J = torch.func.vmap(torch.func.jacrev(lambda r: f(t, r[None])[0]))(y)
    if eps is None:
        return torch.diagonal(J, dim1=-2, dim2=-1).sum(-1).numpy(), J.numpy()
    e = torch.as_tensor(np.asarray(eps, dtype=np.float64))
    return torch.einsum("bi,bij,bj->b", e, J, e).numpy(), J.numpy()


def min_abs_preactivation(Ws, bs, t, x):
    """Per row: the smallest |z| over the hidden pre-activations (float64).  selu' jumps at z = 0 (scale vs
    scale * alpha), so tr J is discontinuous there: an evaluation within rounding of a kink may take either side."""
    h = np.concatenate([np.asarray(x, np.float64), np.full((len(x), 1), float(t))], 1)
    m = np.full(len(x), np.inf)
    for l in range(3):
        z = h @ np.asarray(Ws[l], np.float64).T + np.asarray(bs[l], np.float64)
        m = np.minimum(m, np.abs(z).min(1))
        h = np.where(z > 0, 1.0507009873554805 * z, 1.0507009873554805 * 1.6732632423543772 * np.expm1(z))
    return m


def abs_jacobian(Ws, bs, t, x):
    """|W3| |S3| |W2| |S2| |W1| |S1| |W0[:, :d]| per row (float64): the magnitude of the terms whose sum is J, i.e. the
    scale of fp32 rounding in J (entries of J may cancel to far below it)."""
    d = Ws[3].shape[0]
    h = np.concatenate([np.asarray(x, np.float64), np.full((len(x), 1), float(t))], 1)
    A = np.broadcast_to(np.abs(np.asarray(Ws[0], np.float64)[:, :d]), (len(x),) + Ws[0][:, :d].shape)
    for l in range(3):
        z = h @ np.asarray(Ws[l], np.float64).T + np.asarray(bs[l], np.float64)
        s = np.where(z > 0, 1.0507009873554805, 1.0507009873554805 * 1.6732632423543772 * np.exp(z))
        A = s[:, :, None] * A
        A = np.abs(np.asarray(Ws[l + 1], np.float64))[None] @ A
        h = np.where(z > 0, 1.0507009873554805 * z, 1.0507009873554805 * 1.6732632423543772 * np.expm1(z))
    return A


def aug_field_np(Ws, bs, eps=None):
    """The float64 augmented field of a [B, 1 + d] state, in the layout of the reference's CNF: column 0 carries
    -div f(t, x) (tr J, or eps^T J eps), columns 1.. carry f(t, x)."""
    fx = mlp_field_np(Ws, bs)

    def F(t, Y):
        Y = np.asarray(Y, dtype=np.float64)
        x = Y[:, 1:]
        div, _ = divergence_f64(Ws, bs, t, x, eps)
        return np.concatenate([-div[:, None], fx(t, x)], 1)
    return F
