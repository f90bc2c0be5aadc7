"""Continuous normalising flow of a trained vector field: the divergence-augmented field and the
log-likelihood.

Counterpart of the reference's density evaluation:

* ``CNF`` + ``autograd_trace`` of examples/2D_tutorials/model-comparison-plotting.ipynb cells 2, 4
  and 7 (the state is ``[B, 1 + d]``, column 0 carries ``-tr(dv/dx)``, integrated backward in time);
* ``cnf_wrapper`` of examples/2D_tutorials/Maximum_likelihood_CNF_tutorial.ipynb cells 3 and 4
  (estimators ``exact``, ``hutch_gaussian``, ``hutch_rademacher``; ``logprob = prior.log_prob(z) + ll``).

For ``MLP(time_varying=True)`` fields of the small-kernel envelope (4 layers, widths <= 64) on fp32
inputs the divergence runs in the HIP kernel ``cfm_mlp_divergence_f32``, and ``NeuralODE(CNF(mlp))``
integrates the augmented state in one persistent launch (``cfm_ode_euler_cnf_mlp_f32`` /
``cfm_ode_dopri5_cnf_mlp_f32``).  Anything else is evaluated with ``torch.func`` in the input's dtype.

Hutchinson probes are fixed for a whole solve (FFJORD's convention, model-comparison's ``CNF.noise``
slot): ``cnf.noise`` if set, else one draw per ``NeuralODE.trajectory`` call, kept as
``cnf.last_noise``.  The ML-CNF tutorial redraws the probe at every evaluation; that is not replicated.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .models import MLP
from .utils import torch_wrapper

ESTIMATORS = ("exact", "hutch_gaussian", "hutch_rademacher")


def _small_envelope(m, d):
    """The MLP fits the small-field kernels: 4 linear layers, widths <= 64, input [x, t] with x of width d."""
    if not (isinstance(m, MLP) and m.time_varying):
        return False
    lins = m._linears()
    if len(lins) != 4 or lins[0].in_features != d + 1 or lins[-1].out_features != d or d + 1 > 64:
        return False
    return all(l.out_features <= 64 and l.bias is not None for l in lins[:3])


class CNF(torch.nn.Module):
    """``forward(t, x)`` with x = [l, y] of shape [B, 1 + d] returns ``cat([-div, v], 1)``, v = model(y, t)."""

    def __init__(self, model, estimator="exact", noise=None):
        super().__init__()
        if estimator not in ESTIMATORS:
            raise NotImplementedError(f"estimator {estimator!r}: one of {ESTIMATORS}")
        self.model = model.model if isinstance(model, torch_wrapper) else model
        self.estimator = estimator
        self.noise = noise
        self.last_noise = None
        self._solve_noise = None

    # ---- probes ----
    def draw_noise(self, y):
        """One probe [B, d] from torch's global generator on y's device (None for the exact trace)."""
        if self.estimator == "exact":
            return None
        if self.estimator == "hutch_gaussian":
            e = torch.randn(y.shape, device=y.device, dtype=y.dtype)
        else:
            e = torch.randint(0, 2, y.shape, device=y.device).to(y.dtype) * 2 - 1
        self.last_noise = e
        return e

    def checked_noise(self, y):
        """cnf.noise as a [B, d] probe for the state columns y; a ValueError for any other shape (the kernels read
        one probe per row and column: no broadcasting)."""
        e = torch.as_tensor(self.noise)
        if tuple(e.shape) != tuple(y.shape):
            raise ValueError(f"CNF.noise has shape {tuple(e.shape)}; the state needs one probe per row: {tuple(y.shape)}")
        return e.to(device=y.device, dtype=y.dtype)

    def _probe(self, y):
        if self.estimator == "exact":
            return None
        if self.noise is not None:
            return self.checked_noise(y)
        if self._solve_noise is not None:
            return self._solve_noise.to(device=y.device, dtype=y.dtype)
        return self.draw_noise(y)

    def hip_mlp(self, d):
        """The MLP when the HIP kernels take this field at state width d, else None."""
        return self.model if _small_envelope(self.model, d) else None

    # ---- evaluation ----
    def forward(self, t, x):
        y = x[:, 1:]
        eps = self._probe(y)
        d = y.shape[1]
        m = self.hip_mlp(d)
        if (m is not None and x.dtype == torch.float32 and torch.cuda.is_available()
                and all(p.dtype == torch.float32 for p in m.parameters())):
            out = self._forward_hip(m, t, y, eps)
            if out is not None:
                return out.to(x.device)
        v, div = self._forward_func(t, y, eps)
        return torch.cat([-div[:, None], v], 1)

    def _forward_hip(self, m, t, y, eps):
        lib = _lib.load()
        dev = _lib.require_gpu()
        Wp, bp, dims, keep = m.hip_params(dev)
        yd = _lib.to_dev_f32(y, dev)
        B, d = yd.shape
        out = torch.empty((B, 1 + d), dtype=torch.float32, device=dev)
        v = torch.empty((B, d), dtype=torch.float32, device=dev)
        div = torch.empty((B,), dtype=torch.float32, device=dev)
        if eps is not None and tuple(eps.shape) != (B, d):
            raise ValueError(f"probe of shape {tuple(eps.shape)} for a state of {B} rows and {d} columns")
        ed = _lib.to_dev_f32(eps, dev) if eps is not None else None
        rc = lib.cfm_mlp_divergence_f32(Wp, bp, dims, 4, ptr(yd), B, float(torch.as_tensor(t).reshape(-1)[0]),
                                        0 if eps is None else 1, ptr(ed), ptr(v), ptr(div), None, stream_ptr())
        if rc == -1:            # CFM_EINVAL inside the envelope: the fused small-field path is switched off
            return None
        _lib.check(rc, "cfm_mlp_divergence_f32")
        out[:, 0] = -div
        out[:, 1:] = v
        return out

    def _func_field(self, t, dtype, device):
        """v(y) for ONE row y [d], through the module graph (MLP.net, never MLP.forward: its autograd.Function has
        no forward-mode rule), with the parameters in `dtype`."""
        m = self.model
        net = m.net if isinstance(m, MLP) else m
        params = {k: p.detach().to(device=device, dtype=dtype) for k, p in net.named_parameters()}
        buffers = {k: b.to(device=device) for k, b in net.named_buffers()}
        tt = torch.as_tensor(t, dtype=dtype, device=device).reshape(1)

        def f(y):
            inp = torch.cat([y, tt])[None]
            return torch.func.functional_call(net, (params, buffers), (inp,))[0]
        return f

    def _forward_func(self, t, y, eps):
        f = self._func_field(t, y.dtype, y.device)
        if eps is None:
            v = torch.func.vmap(f)(y)
            jac = torch.func.vmap(torch.func.jacrev(f))(y)
            div = torch.diagonal(jac, dim1=-2, dim2=-1).sum(-1)
        else:
            v, jv = torch.func.vmap(lambda yy, ee: torch.func.jvp(f, (yy,), (ee,)))(y, eps)
            div = (eps * jv).sum(-1)
        return v, div


def standard_normal_log_prob(z):
    d = z.shape[1]
    return -0.5 * (z * z).sum(1) - 0.5 * d * math.log(2 * math.pi)


@torch.no_grad()
def log_likelihood(model, x, t_span=None, solver="dopri5", atol=1e-5, rtol=1e-5, estimator="exact", noise=None,
                   prior_log_prob=None, return_z=False):
    """log p_1(x) of the flow of `model` ([B]): integrate [0, x] from t = 1 to t = 0 under the augmented field,
    return log p_0(z) - l(0) (default prior: the standard normal).  `model`: MLP(time_varying=True) or
    torch_wrapper(MLP).  With return_z, also z = x(0)."""
    from .ode import NeuralODE
    cnf = CNF(model, estimator=estimator, noise=noise)
    node = NeuralODE(cnf, solver=solver, atol=atol, rtol=rtol)
    ts = torch.tensor([1.0, 0.0]) if t_span is None else t_span
    aug = torch.cat([torch.zeros_like(x[:, :1]), x], 1)
    traj = node.trajectory(aug, ts)
    z, ell = traj[-1][:, 1:], traj[-1][:, 0]
    logp0 = prior_log_prob(z) if prior_log_prob is not None else standard_normal_log_prob(z)
    out = logp0 - ell
    return (out, z) if return_z else out
