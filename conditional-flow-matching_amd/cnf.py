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
``cfm_ode_dopri5_cnf_mlp_f32``).  For the action-matching field ``GradModel(MLP(dim, out_dim=1, time_varying=True))`` of
that envelope with the exact trace, ``-div`` is minus the Laplacian of the action: one evaluation runs in
``cfm_mlp_grad_field_f32`` and a fixed-step ``NeuralODE(CNF(GradModel(mlp)))`` in ``cfm_ode_fixed_cnf_gradmlp_f32``
(DESIGN.md 4.10).  Anything else is evaluated with ``torch.func`` in the input's dtype.

Training by maximum likelihood (the tutorial's cell 5: ``NeuralODE(cnf_wrapper(model, "exact"), solver="euler",
sensitivity="adjoint")``, ``loss.backward()``) is ``DifferentiableCNF``: the Euler solve of the augmented state with a
gradient.  On the HIP path the forward is ``cfm_ode_fixed_cnf_mlp_f32`` at Euler and the backward is one launch of
``cfm_cnf_euler_grad_f32`` over the saved trajectory: the exact gradient of the recurrence the forward ran
(discretise-then-optimise).  torchdyn's ``sensitivity="adjoint"`` integrates the continuous adjoint with the same
solver instead, which differs from this by O(h); torchdyn is absent from the reference tree, so that variant is
unpinned, as the forward solvers are.

``RegularizedCNF`` adds the reference's kinetic and Jacobian penalties (``AugmentationModule`` with ``squared_l2_reg`` /
``jacobian_frobenius_reg``, ``CNFLitModule.step``) as further state columns ``[l, (e), (f), y]``: forward
``cfm_ode_euler_cnf_reg_mlp_f32``, backward one launch of ``cfm_cnf_reg_euler_grad_f32``.  It takes the
``L1`` and ``L2`` path lengths as penalties too (``l1_reg``, ``l2_reg``: state ``[l, (L1), (L2), (e), (f), y]``).

``AugmentationModule`` is the reference's class of that name: which of these columns a solve carries, with or without
the trace.  ``FlowSolver.odeint`` (sde.py) integrates them next to the trajectory, for ``ode_solver="euler"`` in one
launch of the same forward entry in its "no trace" mode.

Hutchinson probes are fixed for a whole solve (FFJORD's convention, model-comparison's ``CNF.noise``
slot): ``cnf.noise`` if set, else one draw per ``NeuralODE.trajectory`` call, kept as
``cnf.last_noise``.  The ML-CNF tutorial redraws the probe at every evaluation; that is not replicated.
"""
import contextlib
import ctypes
import math

import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .models import MLP, GradModel
from .ode import _check_t_span, _Declined, _solve_backward, _solve_forward
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

    def hip_grad(self, d):
        """The action MLP when the field is a GradModel that the gradient-field kernels take at state width d with
        the exact trace, else None."""
        if isinstance(self.model, GradModel) and self.estimator == "exact":
            return self.model.hip_action(d)
        return None

    # ---- evaluation ----
    def forward(self, t, x):
        y = x[:, 1:]
        eps = self._probe(y)
        d = y.shape[1]
        a = self.hip_grad(d)
        if a is not None and x.dim() == 2 and x.dtype == torch.float32 and torch.cuda.is_available():
            got = self.model.field_hip(a, y, float(torch.as_tensor(t).reshape(-1)[0]), laplacian=True)
            if got is not None:
                return torch.cat([-got[1][:, None], got[0]], 1).to(x.device)
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


def _probe_args(ed):
    """(mode, eps) of the augmented entries: 0 / NULL for the exact trace, 1 / the probe for a Hutchinson estimate."""
    return 0 if ed is None else 1, ptr(ed)


class _CNFEulerFunction(torch.autograd.Function):
    """[l_N, y_N] of the Euler augmented solve (cfm_ode_fixed_cnf_mlp_f32); backward: cfm_cnf_euler_grad_f32."""

    @staticmethod
    def forward(ctx, x_aug, ts, eps, dims, *params):
        ctx.eps = _lib.to_dev_f32(eps, x_aug.device) if eps is not None else None
        traj = _solve_forward(ctx, "cfm_ode_fixed_cnf_mlp_f32", x_aug, ts, dims, params,
                              (*_probe_args(ctx.eps), _lib.ODE_SCHEME["euler"]), declines=True)
        return traj[-1].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _solve_backward(ctx, "cfm_cnf_euler_grad_f32", _lib.OP_CNF_GRAD, g, _probe_args(ctx.eps), 3)


class DifferentiableCNF(CNF):
    """The Euler solve of the augmented state [l, y] with a gradient: maximum-likelihood training of a CNF.

    ``solve(x_aug, t_span)`` returns the final state [B, 1 + d], differentiable with respect to the field's parameters
    and ``x_aug``; ``nll(x)`` is the tutorial's loss.  fp32 CUDA states of a small-envelope ``MLP(time_varying=True)``
    (or ``torch_wrapper`` of one) with fp32 parameters run on the HIP kernels (``last_path == "hip"``; the value is
    bit-equal to ``NeuralODE(CNF(m), solver="euler").trajectory(...)[-1]``, the gradient is that of the recurrence,
    once differentiable).  Everything else runs the same recurrence in differentiable torch ops (``"generic"``): CPU,
    float64, other fields, the fused path switched off, and a grid of more than 3 B (1 + d) points, which
    ``cfm_ode_fixed_cnf_mlp_f32`` refuses because its workspace keeps the device copy of ``t_span`` in three state-sized
    buffers (B = 1, d = 2 with the default 100 steps is such a case).  Nothing is printed: ``last_path`` says which path
    ran.  The Hutchinson probe follows ``CNF``: ``noise`` if given, else one draw per solve (``last_noise``)."""

    def __init__(self, model, estimator="exact", noise=None, solver="euler"):
        super().__init__(model, estimator=estimator, noise=noise)
        if solver != "euler":
            raise NotImplementedError(f"solver {solver!r}: the gradient is that of the Euler recurrence "
                                      "y += h v, l -= h div (discretise-then-optimise); no other scheme has one")
        self.solver = solver
        self.last_path = None

    def solve(self, x_aug, t_span):
        if x_aug.dim() != 2 or x_aug.shape[1] < 2:
            raise ValueError(f"the state is [B, 1 + d]; got {tuple(x_aug.shape)}")
        return self._solve(x_aug, t_span, 1, _CNFEulerFunction, True, ())

    def _solve(self, x_aug, t_span, a, function, fused_ok, extra):
        """The solve of a checked state [B, a + d] whose first ``a`` columns are augmented: ``function`` (one of the
        autograd.Function pairs above, called with ``extra`` between dims and the parameters) where the HIP kernels take
        it and ``fused_ok`` holds, the generic recurrence otherwise."""
        ts = torch.as_tensor(t_span).detach().to(dtype=x_aug.dtype).cpu()
        _check_t_span(ts)
        y = x_aug[:, a:]
        eps = None
        if self.estimator != "exact":
            eps = self.checked_noise(y) if self.noise is not None else self.draw_noise(y)
        m = self.hip_mlp(y.shape[1])
        if (m is not None and x_aug.is_cuda and x_aug.dtype == torch.float32 and fused_ok
                and all(p.dtype == torch.float32 and p.device == x_aug.device for p in m.parameters())):
            params = [p for l in m._linears() for p in (l.weight, l.bias)]
            try:
                out = function.apply(x_aug, ts.numpy().copy(), eps, m.dims(), *extra, *params)
                self.last_path = "hip"
                return out
            except _Declined:
                pass
        self.last_path = "generic"
        return self._solve_generic(x_aug, ts, eps)

    def _solve_generic(self, x_aug, ts, eps):
        """The recurrence in differentiable torch ops, through the module graph (MLP.net, never MLP.forward: see
        CNF._func_field), with the parameters cast to the state's dtype."""
        m = self.model
        net = m.net if isinstance(m, MLP) else m
        l, y = x_aug[:, 0], x_aug[:, 1:]
        params = {k: p.to(device=y.device, dtype=y.dtype) for k, p in net.named_parameters()}
        buffers = {k: b.to(device=y.device) for k, b in net.named_buffers()}
        for n in range(ts.numel() - 1):
            h = float(ts[n + 1] - ts[n])
            tt = ts[n].to(device=y.device).reshape(1)

            def f(yy):
                return torch.func.functional_call(net, (params, buffers), (torch.cat([yy, tt])[None],))[0]
            if eps is None:
                v = torch.func.vmap(f)(y)
                jac = torch.func.vmap(torch.func.jacrev(f))(y)
                div = torch.diagonal(jac, dim1=-2, dim2=-1).sum(-1)
            else:
                v, jv = torch.func.vmap(lambda yy, ee: torch.func.jvp(f, (yy,), (ee,)))(y, eps)
                div = (eps * jv).sum(-1)
            y = y + h * v
            l = l - h * div
        return torch.cat([l[:, None], y], 1)

    def nll(self, x, t_span=None, steps=100, prior_log_prob=None):
        """-mean(log p_0(z) - l) of the solve of [0, x] from t = 1 to t = 0 on `steps` uniform Euler steps (or on
        `t_span`); the prior term (default: the standard normal) goes through ordinary autograd."""
        ts = torch.linspace(1.0, 0.0, int(steps) + 1, dtype=x.dtype) if t_span is None else t_span
        out = self.solve(torch.cat([torch.zeros_like(x[:, :1]), x], 1), ts)
        z, ell = out[:, 1:], out[:, 0]
        logp0 = prior_log_prob(z) if prior_log_prob is not None else standard_normal_log_prob(z)
        return -(logp0 - ell).mean()


# ---- regularised CNF training: the kinetic and Jacobian penalties as path integrals ----------------
REG_NAMES = ("squared_L2", "jacobian_frobenius")        # bit 0, bit 1 of reg_mask; the reference's order
# every regulariser column in the reference's order (augmentation.py:158-177), which is not bit order, with its reg_mask
# bit (include/cfm_gfx950.h: CFM_REG_*)
AUG_REG_BITS = (("L1", 4), ("L2", 8), ("squared_L2", 1), ("jacobian_frobenius", 2))
TRACE_EXACT, TRACE_HUTCH, TRACE_NONE = 0, 1, 2          # CFM_TRACE_*


def _mask_of(names):
    return sum(bit for n, bit in AUG_REG_BITS if n in names)


def _reg_integrands(mask, v, jac):
    """The regulariser integrands of ``mask`` at a velocity v [B, d] (jac [B, d, d]: dv/dx, read with bit 1 only), in
    the reference's order: L1Reg, L2Reg, SquaredL2Reg, JacobianFrobeniusReg of augmentation.py:21-73."""
    d = v.shape[1]
    out = []
    if mask & 4:
        out.append(v.abs().mean(1))
    if mask & 8:
        out.append(torch.norm(v, p=2, dim=1) / d ** 0.5)
    if mask & 1:
        out.append((v * v).sum(1))
    if mask & 2:
        out.append(torch.norm(jac.reshape(jac.shape[0], -1), p=2, dim=1) / d)
    return out


class AugmentationModule(torch.nn.Module):
    """The reference's ``AugmentationModule`` (runner/src/models/components/augmentation.py:137-210): which path
    integrals a solve carries in front of the state, in which order, and with which coefficients.  ``names`` /
    ``coeffs`` / ``aug_dims`` and both return shapes of ``forward`` are the reference's.  ``cnf_estimator``: None or
    ``"exact"``.  ``integrands(f, t, x)`` evaluates the columns' time derivatives for any callable field with autograd
    (what ``AugmentedVectorField`` does, :266-303); ``FlowSolver.odeint`` integrates them, in one HIP launch where it can."""

    def __init__(self, cnf_estimator=None, l1_reg=0., l2_reg=0., squared_l2_reg=0., jacobian_frobenius_reg=0.,
                 jacobian_diag_frobenius_reg=0., jacobian_off_diag_frobenius_reg=0.):
        super().__init__()
        if cnf_estimator not in (None, "exact"):
            raise ValueError(f"cnf_estimator {cnf_estimator!r}: None or 'exact' (the reference's AugmentationModule builds "
                             "the exact trace for 'exact' and none for anything else)")
        if jacobian_diag_frobenius_reg > 0. or jacobian_off_diag_frobenius_reg > 0.:
            raise NotImplementedError(
                "jacobian_diag_frobenius_reg / jacobian_off_diag_frobenius_reg are not built: the reference takes the "
                "diagonal as jac.view(N, -1)[:, ::d], which for d > 1 is the first output's gradient and not the "
                "diagonal (that would be a stride of d + 1), and no config of the reference sets either coefficient")
        self.cnf_estimator = cnf_estimator
        given = {"L1": l1_reg, "L2": l2_reg, "squared_L2": squared_l2_reg, "jacobian_frobenius": jacobian_frobenius_reg}
        self.names = (["log_prob"] if cnf_estimator == "exact" else []) + [n for n, _ in AUG_REG_BITS if given[n] > 0.]
        self.coeffs = torch.tensor(([1] if cnf_estimator == "exact" else []) + [given[n] for n, _ in AUG_REG_BITS if given[n] > 0.])
        self.aug_dims = len(self.names)
        self.reg_mask = _mask_of(self.names)

    def forward(self, x):
        """``(reg, x)`` without a trace, ``(delta_logprob, reg, x)`` with one: the regulariser columns times their
        coefficients (``zeros(1)`` when there is none)."""
        if self.cnf_estimator is None:
            if self.aug_dims == 0:
                return torch.zeros(1).type_as(x), x
            aug, x = x[:, :self.aug_dims], x[:, self.aug_dims:]
            return aug * self.coeffs.to(aug), x
        delta_logprob, aug, x = x[:, :1], x[:, 1:self.aug_dims], x[:, self.aug_dims:]
        reg = aug * self.coeffs[1:].to(aug)
        if self.aug_dims == 1:
            reg = torch.zeros(1).type_as(x)
        return delta_logprob, reg, x

    def integrands(self, f, t, x):
        """``(augs [B, aug_dims], dx [B, d])`` of the field ``f(t, x)`` at x [B, d]: the Jacobian, where a column needs
        it (log_prob, jacobian_frobenius), by one autograd.grad per output column."""
        need_jac = self.cnf_estimator == "exact" or bool(self.reg_mask & 2)
        with torch.enable_grad() if need_jac else contextlib.nullcontext():
            xin = x.detach().requires_grad_(True) if need_jac else x
            dx = f(t, xin)
            dx = dx.reshape(dx.shape[0], -1)
            jac = None
            if need_jac:
                rows = [torch.autograd.grad(dx[:, j].sum(), xin, retain_graph=True)[0] for j in range(dx.shape[1])]
                jac = torch.stack(rows, 1)                       # jac[b, j, i] = d dx_j / d x_i
        dx = dx.detach() if need_jac else dx
        cols = [-torch.diagonal(jac, dim1=1, dim2=2).sum(1)] if self.cnf_estimator == "exact" else []
        cols += _reg_integrands(self.reg_mask, dx, jac)
        augs = torch.stack(cols, 1) if cols else dx.new_zeros((dx.shape[0], 0))
        return augs, dx


def augmented_euler_hip(m, x0, t_span, mode, mask):
    """``(traj [n_t, B, a + d], nfe)`` of one launch of ``cfm_ode_euler_cnf_reg_mlp_f32`` on the MLP ``m`` from
    ``[0, .., 0, x0]`` (exact trace or none: no probe), or None where the entry declines (CFM_EINVAL inside the envelope:
    the fused path is switched off, or the grid has more than 3 B (a + d) points)."""
    lib = _lib.load()
    dev = x0.device
    Wp, bp, dims, keep = m.hip_params(dev)
    a = (mode != TRACE_NONE) + bin(mask).count("1")
    B, d = x0.shape
    state = torch.cat([torch.zeros((B, a), dtype=torch.float32, device=dev), _lib.to_dev_f32(x0, dev)], 1)
    ts, tsp, n_t = _lib.t_span_f32(t_span)
    traj = torch.empty((n_t, B, a + d), dtype=torch.float32, device=dev)
    jsq = torch.empty((max(n_t - 1, 1), B), dtype=torch.float32, device=dev) if mask & 2 else None
    ws = _lib.workspace(_lib.OP_ODE, B, max(dims[1:4]), a + d, dev)
    nfe = ctypes.c_int(0)
    rc = lib.cfm_ode_euler_cnf_reg_mlp_f32(Wp, bp, dims, 4, ptr(state), B, tsp, n_t, mode, None, mask, ptr(traj), ptr(jsq),
                                           ctypes.byref(nfe), ptr(ws), stream_ptr())
    if rc == -1:
        return None
    _lib.check(rc, "cfm_ode_euler_cnf_reg_mlp_f32")
    return traj, nfe.value


class _CNFRegEulerFunction(torch.autograd.Function):
    """The final state [l, (e), (f), y] of the regularised Euler solve (cfm_ode_euler_cnf_reg_mlp_f32); backward:
    cfm_cnf_reg_euler_grad_f32 over the saved trajectory and the saved ||J||_F^2 per (step, row)."""

    @staticmethod
    def forward(ctx, x_aug, ts, eps, dims, mask, *params):
        dev = x_aug.device
        ctx.eps = _lib.to_dev_f32(eps, dev) if eps is not None else None
        ctx.mask = mask
        ctx.jsq = torch.empty((max(ts.shape[0] - 1, 1), x_aug.shape[0]), dtype=torch.float32, device=dev) if mask & 2 else None
        traj = _solve_forward(ctx, "cfm_ode_euler_cnf_reg_mlp_f32", x_aug, ts, dims, params, (*_probe_args(ctx.eps), mask),
                              after=(ptr(ctx.jsq),), declines=True)
        return traj[-1].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _solve_backward(ctx, "cfm_cnf_reg_euler_grad_f32", _lib.OP_CNF_GRAD, g,
                               (*_probe_args(ctx.eps), ctx.mask, ptr(ctx.jsq)), 4)


class RegularizedCNF(DifferentiableCNF):
    """``DifferentiableCNF`` with the reference's path-integral regularisers (RNODE / TrajectoryNet): the state that
    ``AugmentationModule`` builds (runner/src/models/components/augmentation.py:137-210) under ``AugmentedVectorField``
    (:266-303), integrated and differentiated as ``CNFLitModule.step`` does (runner/src/models/cfm_module.py:1412-1454).

    The state is ``[l, (L1), (L2), (e), (f), y]`` of width 1 + r + d.  A column is carried only if its coefficient is > 0,
    in the reference's order (``names``): ``log_prob``; ``L1`` (+= h mean_j |v_j|, ``L1Reg``); ``L2`` (+= h |v| / sqrt(d),
    ``L2Reg``); ``squared_L2`` (e += h |v|^2, ``SquaredL2Reg``); ``jacobian_frobenius`` (f += h ||dv/dx||_F / d,
    ``JacobianFrobeniusReg``).  With every coefficient 0 this is the parent class.

    ``solve`` runs on the HIP kernels (``last_path == "hip"``: ``cfm_ode_euler_cnf_reg_mlp_f32`` forward, one launch of
    ``cfm_cnf_reg_euler_grad_f32`` backward; columns l and y are bit-equal to the parent's solve) under the parent's
    conditions, for the exact trace with any of the penalties and for a Hutchinson estimator without
    ``jacobian_frobenius``.  Everything else runs the same recurrence in differentiable torch ops (``"generic"``): CPU, float64, other
    fields, ``jacobian_frobenius`` with a Hutchinson estimator, the fused path switched off, a grid of more than
    3 B (1 + r + d) points."""

    def __init__(self, model, squared_l2_reg=0.0, jacobian_frobenius_reg=0.0, estimator="exact", noise=None, l1_reg=0.0,
                 l2_reg=0.0):
        super().__init__(model, estimator=estimator, noise=noise)
        given = {"L1": l1_reg, "L2": l2_reg, "squared_L2": squared_l2_reg, "jacobian_frobenius": jacobian_frobenius_reg}
        if min(given.values()) < 0.0:
            raise ValueError("a regularisation coefficient is >= 0 (0: the column is not carried)")
        carried = [n for n, _ in AUG_REG_BITS if given[n] > 0.0]
        self.reg_mask = _mask_of(carried)
        self.names = ["log_prob"] + carried
        self.coeffs = torch.tensor([1.0] + [float(given[n]) for n in carried])
        self.aug_dims = len(self.names)

    def solve(self, x_aug, t_span):
        if self.reg_mask == 0:
            return super().solve(x_aug, t_span)
        a = self.aug_dims
        if x_aug.dim() != 2 or x_aug.shape[1] < a + 1:
            raise ValueError(f"the state is [B, {a} + d] ({', '.join(self.names)}, x); got {tuple(x_aug.shape)}")
        return self._solve(x_aug, t_span, a, _CNFRegEulerFunction, self.estimator == "exact" or not self.reg_mask & 2,
                           (self.reg_mask,))

    def _solve_generic(self, x_aug, ts, eps):
        """The recurrence in differentiable torch ops, as the parent's (through the module graph, parameters cast to the
        state's dtype); the Jacobian's norm is torch.norm's, so its gradient is 0 where the Jacobian is."""
        if self.reg_mask == 0:
            return super()._solve_generic(x_aug, ts, eps)
        m = self.model
        grad_field = isinstance(m, GradModel)        # v = d action / dx: GradModel.forward's autograd.grad has no torch.func rule
        if grad_field:
            m = m.action
        net = m.net if isinstance(m, MLP) else m
        a = self.aug_dims
        cols = [x_aug[:, k] for k in range(a)]
        y = x_aug[:, a:]
        d = y.shape[1]
        params = {k: p.to(device=y.device, dtype=y.dtype) for k, p in net.named_parameters()}
        buffers = {k: b.to(device=y.device) for k, b in net.named_buffers()}
        for n in range(ts.numel() - 1):
            h = float(ts[n + 1] - ts[n])
            tt = ts[n].to(device=y.device).reshape(1)

            def net_of(z):
                return torch.func.functional_call(net, (params, buffers), (z[None],))[0]

            def f(yy):
                z = torch.cat([yy, tt])
                return torch.func.grad(lambda q: net_of(q).sum())(z)[:d] if grad_field else net_of(z)
            jac = None
            if eps is None or self.reg_mask & 2:
                jac = torch.func.vmap(torch.func.jacrev(f))(y)
            if eps is None:
                v = torch.func.vmap(f)(y)
                div = torch.diagonal(jac, dim1=-2, dim2=-1).sum(-1)
            else:
                v, jv = torch.func.vmap(lambda yy, ee: torch.func.jvp(f, (yy,), (ee,)))(y, eps)
                div = (eps * jv).sum(-1)
            cols[0] = cols[0] - h * div
            for k, g in enumerate(_reg_integrands(self.reg_mask, v, jac), 1):
                cols[k] = cols[k] + h * g
            y = y + h * v
        return torch.cat([torch.stack(cols, 1), y], 1)

    def split(self, state):
        """``(delta_logprob [B, 1], reg [B, r], x [B, d])`` as ``AugmentationModule.forward`` (augmentation.py:206-210):
        the regulariser columns times their coefficients; ``zeros(1)`` when none is carried."""
        a = self.aug_dims
        delta_logprob, aug, x = state[:, :1], state[:, 1:a], state[:, a:]
        reg = aug * self.coeffs[1:].to(aug)
        if a == 1:
            reg = torch.zeros(1).type_as(x)
        return delta_logprob, reg, x

    def loss(self, x, steps=100, t_span=None, prior_log_prob=None):
        """``(reg, nll)`` as ``CNFLitModule.step`` for a single time point (cfm_module.py:1437-1454): the solve of
        [0, .., 0, x] from t = 1 to t = 0 on `steps` uniform Euler steps (or on `t_span`); reg = -mean(aug * coeffs)
        over rows and columns (negative because the integration runs backward), nll = -mean(prior(z) - l)."""
        ts = torch.linspace(1.0, 0.0, int(steps) + 1, dtype=x.dtype) if t_span is None else t_span
        out = self.solve(torch.cat([torch.zeros_like(x[:, :1]).expand(-1, self.aug_dims), x], 1), ts)
        delta_logprob, reg, z = self.split(out)
        logp0 = prior_log_prob(z) if prior_log_prob is not None else standard_normal_log_prob(z)
        return torch.mean(-reg), -(logp0 - delta_logprob[:, 0]).mean()
