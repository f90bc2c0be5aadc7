"""fp64 restatement of the Euler solve of the augmented CNF state and of its loss, for the CNF training tests (a
helper module imported by test files; not a conftest).

The field is an explicit layer chain with explicit tangents (no torch.func, no nn.Module): z_l = W_{l-1} h_{l-1} + b,
s_l = selu'(z_l), T_l^k = s_l * (W_{l-1} T_{l-1}^k), div = sum_k w_k^T W_3 T_3^k with (tau_k, w_k) = (e_k, e_k) for the
exact trace and one pair (eps, eps) for Hutchinson.  Gradients come from autograd through these tensor ops."""
import numpy as np
import torch

SCALE, ALPHA = 1.0507009873554805, 1.6732632423543772


def selu(z):
    return torch.where(z > 0, SCALE * z, SCALE * ALPHA * torch.expm1(torch.clamp(z, max=0.0)))


def selu_slope(z):
    """selu'(z) with the side convention of elu_backward: scale for z > 0, scale * alpha * exp(z) otherwise; its own
    derivative under autograd is 0 for z > 0 and scale * alpha * exp(z) otherwise (PyTorch's double backward)."""
    return torch.where(z > 0, torch.full_like(z, SCALE), SCALE * ALPHA * torch.exp(torch.clamp(z, max=0.0)))


def as_params(Ws, bs, requires_grad=True):
    """float64 leaf tensors [W0, b0, W1, b1, W2, b2, W3, b3] from numpy weights / biases."""
    out = []
    for W, b in zip(Ws, bs):
        out.append(torch.tensor(np.asarray(W, np.float64), requires_grad=requires_grad))
        out.append(torch.tensor(np.asarray(b, np.float64), requires_grad=requires_grad))
    return out


def field_div(params, y, t, eps=None):
    """(v, div) of the MLP field at (y [B, d], t): div = tr J (eps None) or eps^T J eps."""
    W = params[0::2]; b = params[1::2]
    d = y.shape[1]
    h = torch.cat([y, torch.full_like(y[:, :1], float(t))], 1)
    s = []
    for l in range(3):
        z = h @ W[l].T + b[l]
        s.append(selu_slope(z))
        h = selu(z)
    v = h @ W[3].T + b[3]
    if eps is None:
        div = torch.zeros_like(y[:, 0])
        for k in range(d):
            T = s[0] * W[0][:, k]
            T = s[1] * (T @ W[1].T)
            T = s[2] * (T @ W[2].T)
            div = div + T @ W[3][k]
    else:
        T = s[0] * (eps @ W[0][:, :d].T)
        T = s[1] * (T @ W[1].T)
        T = s[2] * (T @ W[2].T)
        div = (eps * (T @ W[3].T)).sum(1)
    return v, div


def euler_solve(params, x_aug, ts, eps=None, trajectory=False):
    """The final state [l_N, y_N] of y += h v, l -= h div over the grid ts (floats, either direction)."""
    l, y = x_aug[:, 0], x_aug[:, 1:]
    ys = [y]
    for n in range(len(ts) - 1):
        h = float(ts[n + 1]) - float(ts[n])
        v, div = field_div(params, y, float(ts[n]), eps)
        y = y + h * v
        l = l - h * div
        ys.append(y)
    out = torch.cat([l[:, None], y], 1)
    return (out, ys) if trajectory else out


def standard_normal_log_prob(z):
    return -0.5 * (z * z).sum(1) - 0.5 * z.shape[1] * float(np.log(2 * np.pi))


def nll(params, x, ts, eps=None):
    """The tutorial's loss: -mean(prior(z) - l) of the solve of [0, x] over ts."""
    out = euler_solve(params, torch.cat([torch.zeros_like(x[:, :1]), x], 1), ts, eps)
    return -(standard_normal_log_prob(out[:, 1:]) - out[:, 0]).mean()


def grads_for_upstream(Ws, bs, x_aug, ts, G, eps=None):
    """(final state, [dW0, db0, ..., dW3, db3], d/dx_aug) of sum(G * solve) in float64 numpy."""
    params = as_params(Ws, bs)
    xa = torch.tensor(np.asarray(x_aug, np.float64), requires_grad=True)
    e = None if eps is None else torch.tensor(np.asarray(eps, np.float64))
    out = euler_solve(params, xa, ts, e)
    g = torch.autograd.grad((out * torch.as_tensor(np.asarray(G, np.float64))).sum(), params + [xa], allow_unused=True)
    g = [torch.zeros_like(p) if q is None else q for p, q in zip(params + [xa], g)]
    return out.detach().numpy(), [q.numpy() for q in g[:-1]], g[-1].numpy()


def kink_free_rows(Ws, bs, x_aug, ts, eps=None, tol=1e-5):
    """Rows whose smallest hidden |z| along the float64 Euler trajectory stays >= tol (boolean mask)."""
    from cnf_restate import min_abs_preactivation
    with torch.no_grad():
        _, ys = euler_solve(as_params(Ws, bs, False), torch.as_tensor(np.asarray(x_aug, np.float64)), ts,
                            None if eps is None else torch.as_tensor(np.asarray(eps, np.float64)), trajectory=True)
    m = np.full(len(x_aug), np.inf)
    for n in range(len(ts) - 1):
        m = np.minimum(m, min_abs_preactivation(Ws, bs, float(ts[n]), ys[n].numpy()))
    return m >= tol
