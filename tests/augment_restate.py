"""fp64 restatement of the solve of AugmentedVectorField's state (runner/src/models/components/augmentation.py:266-303)
with the five integrands of AugmentationModule, for the augmented-sampler tests (a helper module imported by test files;
not a conftest).

The field is the explicit layer chain of cnf_reg_restate.py (v, div, |v|^2, ||J||_F / d by explicit tangents) with the
two |v| integrands added: mean_j |v_j| (L1Reg) and |v| / sqrt(d) (L2Reg).  The state is [(l), (L1), (L2), (e), (f), y]: l with
mode 0 (exact trace) or 1 (Hutchinson probe eps), none with mode 2; mask bit 0 = e, bit 1 = f, bit 2 = L1, bit 3 = L2 (the
reference's order is not bit order).  Gradients come from autograd through these tensor ops."""
import numpy as np
import torch

import cnf_reg_restate as rr
import cnf_train_restate as tr

NAMES = ("log_prob", "L1", "L2", "squared_L2", "jacobian_frobenius")
BITS = {"L1": 4, "L2": 8, "squared_L2": 1, "jacobian_frobenius": 2}


def golden_case(seed=11, d=2, w=64, n=8, times=(0.25, 0.8)):
    """The inputs of tests/golden/augmentation_integrands.json (tools/make_augmentation_golden.py wrote it from these):
    a d-w-w-w-d net with uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)) layers and n standard-normal points, from numpy's
    seeded Generator (a stream that does not depend on the torch version), float32 values."""
    g = np.random.default_rng(seed)
    dims = [d + 1, w, w, w, d]
    Ws = [g.uniform(-1, 1, (b, a)).astype(np.float32) / np.float32(np.sqrt(a)) for a, b in zip(dims[:-1], dims[1:])]
    bs = [g.uniform(-1, 1, (b,)).astype(np.float32) / np.float32(np.sqrt(a)) for a, b in zip(dims[:-1], dims[1:])]
    return Ws, bs, g.normal(size=(n, d)).astype(np.float32), tuple(times)


def n_aug(mode, mask):
    return (mode != 2) + bin(mask & 15).count("1")


def columns(mode, mask):
    """The names of the augmented columns of a state row, in order."""
    return [n for n in NAMES if (n == "log_prob" and mode != 2) or (n != "log_prob" and mask & BITS[n])]


def integrands(params, y, t, mode, mask, eps=None):
    """(v [B, d], [the augmented columns' time derivatives, in state order]) at (y, t)."""
    v, div, e, f = rr.field_all(params, y, t, eps if mode == 1 else None)
    d = y.shape[1]
    by_name = {"log_prob": -div, "L1": v.abs().sum(1) / d, "L2": torch.sqrt((v * v).sum(1)) / d ** 0.5,
               "squared_L2": e, "jacobian_frobenius": f}
    return v, [by_name[n] for n in columns(mode, mask)]


_RK4_C = (1 / 3, 2 / 3, 1.0)          # the 3/8 rule, torchdyn's "rk4" and cfm_amd.ode.FIXED_TABLEAUS


def solve(params, state0, ts, mode, mask, eps=None, scheme="euler"):
    """Every grid point's state [B, a + d] (a list of n_t tensors).  euler: everything at (y_n, t_n).  rk4: the 3/8-rule
    tableau on the whole augmented state, the stage times formed in float32 as the generic stepper of cfm_amd.ode forms
    them (t and h are float32 grid values; every other operation is float64)."""
    a = n_aug(mode, mask)
    x = state0
    out = [x]

    def rhs(t, s):
        v, cols = integrands(params, s[:, a:], t, mode, mask, eps)
        return torch.cat([torch.stack(cols, 1), v], 1) if cols else v

    for n in range(len(ts) - 1):
        t32, h32 = np.float32(ts[n]), np.float32(ts[n + 1]) - np.float32(ts[n])
        h = float(h32)
        if scheme == "euler":
            x = x + h * rhs(float(t32), x)
        else:
            k1 = rhs(float(t32), x)
            k2 = rhs(float(t32 + np.float32(_RK4_C[0]) * h32), x + h * (k1 / 3))
            k3 = rhs(float(t32 + np.float32(_RK4_C[1]) * h32), x + h * (-k1 / 3 + k2))
            k4 = rhs(float(t32 + np.float32(_RK4_C[2]) * h32), x + h * (k1 - k2 + k3))
            x = x + h * (k1 / 8 + 3 * k2 / 8 + 3 * k3 / 8 + k4 / 8)
        out.append(x)
    return out


def trajectory64(Ws, bs, x0, ts, mode, mask, eps=None, scheme="euler"):
    """[n_t, B, a + d] in float64 numpy from zero augmented columns in front of x0 [B, d]."""
    params = tr.as_params(Ws, bs, False)
    x = torch.as_tensor(np.asarray(x0, np.float64))
    s0 = torch.cat([torch.zeros((len(x), n_aug(mode, mask)), dtype=torch.float64), x], 1)
    e = None if eps is None else torch.as_tensor(np.asarray(eps, np.float64))
    with torch.no_grad():
        return torch.stack(solve(params, s0, ts, mode, mask, e, scheme)).numpy()


def grads_for_upstream(Ws, bs, x_aug, ts, G, mode, mask, eps=None):
    """(final state, [dW0, db0, ..., dW3, db3], d/dx_aug) of sum(G * final state of the Euler solve) in float64 numpy,
    G [B, a + d] an upstream gradient on ALL columns."""
    params = tr.as_params(Ws, bs)
    xa = torch.tensor(np.asarray(x_aug, np.float64), requires_grad=True)
    e = None if eps is None else torch.tensor(np.asarray(eps, np.float64))
    out = solve(params, xa, ts, mode, mask, e)[-1]
    g = torch.autograd.grad((out * torch.as_tensor(np.asarray(G, np.float64))).sum(), params + [xa], allow_unused=True)
    g = [torch.zeros_like(p) if q is None else q for p, q in zip(params + [xa], g)]
    return out.detach().numpy(), [q.numpy() for q in g[:-1]], g[-1].numpy()


def usable_rows(Ws, bs, x_aug, ts, mode, mask, eps=None, tol=1e-5):
    """Boolean mask of the rows to keep.  A row goes if anywhere along its float64 Euler trajectory a hidden
    pre-activation is within tol of a SELU kink (cnf_train_restate.kink_free_rows), or, with the L1 column, some
    |v_j| < tol (the kink of abs), or, with the L2 column, |v| < tol (the kink of the norm), or, with the
    jacobian_frobenius column, ||J||_F / d < tol (cnf_reg_restate.usable_rows' rule for that column)."""
    a = n_aug(mode, mask)
    xa = np.asarray(x_aug, np.float64)
    ly = np.concatenate([np.zeros((len(xa), 1)), xa[:, a:]], 1)
    keep = tr.kink_free_rows(Ws, bs, ly, ts, eps if mode == 1 else None, tol=tol)
    params = tr.as_params(Ws, bs, False)
    with torch.no_grad():
        states = solve(params, torch.as_tensor(xa), ts, mode, mask, None if eps is None else torch.as_tensor(np.asarray(eps, np.float64)))
        for n in range(len(ts) - 1):
            v, div, e, f = rr.field_all(params, states[n][:, a:], float(np.float32(ts[n])))
            if mask & 4:
                keep &= (v.abs().min(1).values >= tol).numpy()
            if mask & 8:
                keep &= (torch.sqrt(e) >= tol).numpy()
            if mask & 2:
                keep &= (f >= tol).numpy()
    return keep
