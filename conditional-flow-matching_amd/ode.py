"""ODE sampling — counterpart of ``torchdyn.core.NeuralODE`` as the reference uses it
(``NeuralODE(torch_wrapper(model), solver=..., sensitivity="adjoint", atol, rtol)
.trajectory(x, t_span)``: examples/2D_tutorials/Flow_matching_tutorial.ipynb cells 11/16,
examples/images/cifar10/utils_cifar.py:63-68).

When the vector field is ``torch_wrapper(MLP(time_varying=True))`` the whole solve runs in
the HIP drivers (``cfm_ode_fixed_mlp_f32`` / ``cfm_ode_adaptive_mlp_f32``); ``CNF(MLP)`` (cnf.py) of
the small-kernel envelope on fp32 ``[B, 1 + d]`` states runs in ``cfm_ode_*_cnf_mlp_f32``.  The action-matching
field ``torch_wrapper(GradModel(MLP(dim, out_dim=1, time_varying=True)))`` of that envelope (``GradModel.hip_action``)
on fp32 states runs in ``cfm_ode_fixed_gradmlp_f32`` / ``cfm_ode_adaptive_gradmlp_f32``, and ``CNF(GradModel(mlp))``
with the exact trace and a fixed-step solver in ``cfm_ode_fixed_cnf_gradmlp_f32``.  Any
other vector field (e.g. a UNet) is stepped by the same algorithm at the tensor level — host
control flow only, the field itself runs wherever the user's module runs.  ``last_path`` says
which of the two ran ("hip" / "generic").

Solvers: torchdyn's fixed-step set ``euler``, ``midpoint``, ``rk4`` (steps exactly on ``t_span``; ``atol`` / ``rtol``
are ignored, as torchdyn does) and the adaptive 5(4) pairs ``dopri5`` and ``tsit5`` (one driver, two tableaus: 7 stages,
FSAL, order-5 controller and initial step, every ``t_span`` point is a step end).  torchdyn's own default is ``tsit5``;
the default here stays ``dopri5``.  ``rk4`` is the 3/8 rule ("torchdyn-style rk4": torchdyn is absent from the reference
tree, so like ``dopri5`` its parity is unpinned).  ``nfe``: stages * (n_t - 1) for the fixed-step solvers, 2 + 6 * step
attempts for the adaptive ones.

``NeuralODE.trajectory`` carries no graph.  ``DifferentiableNeuralODE`` (fixed-step solvers) returns the same values with
one: forward ``cfm_ode_fixed_mlp_f32``, backward ``cfm_ode_fixed_grad_f32``, the gradient of the recurrence.
``AdaptiveDifferentiableNeuralODE`` does the same for ``dopri5`` / ``tsit5``: forward ``cfm_ode_adaptive_rec_mlp_f32``, which
records its accepted steps, backward ``cfm_ode_adaptive_grad_f32`` over them, the step sequence a constant.

``t_span`` is strictly monotone.  A decreasing one integrates backward in time as torchdyn does
(SURVEY.md A.4): ``g(s, x) = -f(-s, x)`` on ``s = -t_span``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .models import GradModel, time_mlp
from .utils import torch_wrapper

# Adaptive pairs: c, a (rows 2..7; row 7 = b, so stage 7's state is the solution), e (x_err = dt * sum e_i k_i).
_DP_BSOL = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
_DP_BALT = [1951 / 21600, 0, 22642 / 50085, 451 / 720, -12231 / 42400, 649 / 6300, 1 / 60]
ADAPTIVE_TABLEAUS = {
    "dopri5": dict(
        c=[1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0],
        a=[[1 / 5],
           [3 / 40, 9 / 40],
           [44 / 45, -56 / 15, 32 / 9],
           [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
           [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
           [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]],
        e=[bs - ba for bs, ba in zip(_DP_BSOL, _DP_BALT)], order=5),
    "tsit5": dict(
        c=[0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0],
        a=[[0.161],
           [-0.008480655492356989, 0.335480655492357],
           [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
           [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
           [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
           [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774]],
        e=[0.001780011052226, 0.000816434459657, -0.007880878010262, 0.144711007173263, -0.582357165452555,
           0.458082105929187, -1 / 66], order=5),
}
# Fixed-step schemes: stage s >= 2 sits at t + c[s-2] dt on x + dt * sum a[s-2][q] k_q; x_new = x + dt * sum b k.
FIXED_TABLEAUS = {
    "euler": dict(c=[], a=[], b=[1.0], order=1),
    "midpoint": dict(c=[1 / 2], a=[[1 / 2]], b=[0.0, 1.0], order=2),
    "rk4": dict(c=[1 / 3, 2 / 3, 1.0], a=[[1 / 3], [-1 / 3, 1.0], [1.0, -1.0, 1.0]], b=[1 / 8, 3 / 8, 3 / 8, 1 / 8], order=4),
}
SOLVERS = ("euler", "midpoint", "rk4", "dopri5", "tsit5")


def _hairer_norm(x):
    """RMS norm, for the step controller alone: detached, so the step sequence is a constant of any graph."""
    return x.detach().abs().pow(2).mean().sqrt()


def _check_t_span(ts):
    """Strictly monotone (either way); returns +1 / -1."""
    if ts.dim() != 1 or ts.numel() < 1:
        raise ValueError("t_span must be a 1-D grid")
    if ts.numel() < 2:
        return 1
    dts = ts[1:] - ts[:-1]
    if bool((dts > 0).all()):
        return 1
    if bool((dts < 0).all()):
        return -1
    raise ValueError("t_span must be strictly increasing or strictly decreasing")


def _solve_hip(kind, m, x, t_span, solver, atol=None, rtol=None, probe=None, second=None, fused=None):
    """One call of cfm_ode_{fixed,adaptive}_<kind>_f32 (fixed for the ODE_SCHEME solvers, adaptive for the ODE_TABLEAU ones)
    on the net ``m``: parameters, state and ``t_span`` marshalled, trajectory and workspace allocated.

    probe: ``(eps,)`` for the augmented (CNF) entries, which take ``(mode, eps)`` after the grid: eps None is the exact
    trace.  second: the other net of the pair entries, its tables after the first net's.  fused=False switches the
    one-launch form off around the call.  Returns ``(rc, entry name, traj [n_t, B, width], nfe, n_steps, ts)`` and checks
    nothing: which ``rc`` is a decline is the caller's rule.  ``ts`` is the pageable host grid the entry read: a caller
    whose entry copies it asynchronously keeps it until it has synchronised the stream."""
    lib = _lib.load()
    dev = _lib.require_gpu()
    Wp, bp, dims, keep = m.hip_params(dev)
    tables = (Wp, bp)
    if second is not None:
        Wb, bb, _, keep_b = second.hip_params(dev)
        tables += (Wb, bb)
    n = len(dims) - 1
    xd = _lib.to_dev_f32(x, dev)
    B, d = xd.shape
    ts, tsp, n_t = _lib.t_span_f32(t_span)
    traj = torch.empty((n_t, B, d), dtype=torch.float32, device=dev)
    ws = _lib.workspace(_lib.OP_ODE, B, max(dims[1:n]) if n > 1 else 1, d, dev)
    args = [*tables, dims, n, ptr(xd), B, tsp, n_t]
    if probe is not None:
        ed = _lib.to_dev_f32(probe[0], dev) if probe[0] is not None else None
        args += [0 if ed is None else 1, ptr(ed)]
    nfe = ctypes.c_int(0)
    steps = ctypes.c_int(0)
    if solver in _lib.ODE_SCHEME:
        what = f"cfm_ode_fixed_{kind}_f32"
        steps.value = n_t - 1
        args += [_lib.ODE_SCHEME[solver], ptr(traj), ctypes.byref(nfe), ptr(ws), stream_ptr()]
    else:
        what = f"cfm_ode_adaptive_{kind}_f32"
        args += [_lib.ODE_TABLEAU[solver], atol, rtol, ptr(traj), ctypes.byref(steps), ctypes.byref(nfe), ptr(ws), stream_ptr()]
    if fused is False:
        lib.cfm_ode_set_fused(0)
    try:
        rc = getattr(lib, what)(*args)
    finally:
        if fused is False:
            lib.cfm_ode_set_fused(1)
    return rc, what, traj, nfe.value, steps.value, ts


class NeuralODE(torch.nn.Module):
    def __init__(self, vector_field, solver="dopri5", order=1, atol=1e-3, rtol=1e-3,
                 sensitivity="autograd", return_t_eval=True, **kwargs):
        super().__init__()
        if solver not in SOLVERS:
            raise NotImplementedError(f"solver {solver!r}: one of {SOLVERS}")
        self.vf = vector_field
        self.solver, self.atol, self.rtol = solver, float(atol), float(rtol)
        self.sensitivity = sensitivity          # inert without autograd through the solve
        self.return_t_eval = return_t_eval
        self.nfe = 0
        self.n_steps = 0
        self.last_path = None     # "hip" / "generic": which path the last trajectory() took

    # ---- dispatch ----
    def _hip_mlp(self):
        return time_mlp(self.vf)

    def _hip_grad(self, x):
        """The action MLP of torch_wrapper(GradModel(mlp)) when the gradient-field drivers take the solve, else None."""
        vf = self.vf
        if (isinstance(vf, torch_wrapper) and isinstance(vf.model, GradModel) and x.dim() == 2
                and x.dtype == torch.float32 and torch.cuda.is_available()):
            return vf.model.hip_action(x.shape[1])
        return None

    @torch.no_grad()
    def trajectory(self, x, t_span):
        _check_t_span(torch.as_tensor(t_span, dtype=torch.float32).cpu())
        from .cnf import CNF
        if isinstance(self.vf, CNF):
            return self._trajectory_cnf(self.vf, x, t_span)
        m = self._hip_mlp()
        if m is not None and x.dim() == 2:
            self.last_path = "hip"
            return self._trajectory_hip(m, x, t_span)
        a = self._hip_grad(x)
        if a is not None:
            traj = self._trajectory_hip(a, x, t_span, grad=True)
            if traj is not None:
                self.last_path = "hip"
                return traj
        self.last_path = "generic"
        return self._trajectory_generic(x, t_span)

    def _trajectory_cnf(self, cnf, x, t_span):
        # one probe for the whole solve (cnf.noise, else a fresh draw exposed as cnf.last_noise)
        eps = None
        if cnf.estimator != "exact":
            eps = cnf.checked_noise(x[:, 1:]) if cnf.noise is not None else cnf.draw_noise(x[:, 1:])
        cnf._solve_noise = eps
        try:
            if x.dim() == 2 and x.dtype == torch.float32 and torch.cuda.is_available():
                m = cnf.hip_mlp(x.shape[1] - 1)
                if m is not None and all(p.dtype == torch.float32 for p in m.parameters()):
                    traj = self._trajectory_cnf_hip(m, x, t_span, eps)
                    if traj is not None:
                        self.last_path = "hip"
                        return traj
                a = cnf.hip_grad(x.shape[1] - 1)     # exact trace of a gradient field: the fixed-step schemes only
                if a is not None and self.solver in _lib.ODE_SCHEME:
                    traj = self._trajectory_cnf_hip(a, x, t_span, None, grad=True)
                    if traj is not None:
                        self.last_path = "hip"
                        return traj
            self.last_path = "generic"
            return self._trajectory_generic(x, t_span)
        finally:
            cnf._solve_noise = None

    def _trajectory_cnf_hip(self, m, x, t_span, eps, grad=False):
        """Augmented solve in cfm_ode_{fixed,adaptive}_cnf_mlp_f32 (grad: m is the action net of a GradModel, fixed
        steps, cfm_ode_fixed_cnf_gradmlp_f32); None when the library declines it (CFM_EINVAL: the fused small-field
        path is switched off) so the caller steps it generically."""
        B, D = x.shape
        if eps is not None and tuple(eps.shape) != (B, D - 1):
            raise ValueError(f"probe of shape {tuple(eps.shape)} for a state of {B} rows and {D - 1} columns")
        rc, what, traj, nfe, steps, _ = _solve_hip("cnf_gradmlp" if grad else "cnf_mlp", m, x, t_span, self.solver,
                                                   self.atol, self.rtol, probe=(eps,))
        if rc == -1:
            return None
        check(rc, what)
        self.nfe, self.n_steps = nfe, steps
        return traj.to(x.device)

    def forward(self, x, t_span):
        sol = self.trajectory(x, t_span)
        return (t_span, sol) if self.return_t_eval else sol

    # ---- HIP drivers ----
    def _trajectory_hip(self, m, x, t_span, grad=False):
        """grad: m is the action net of a GradModel and the solve runs in the cfm_ode_*_gradmlp_f32 drivers; these have
        no layer-per-kernel form, so None comes back when the library declines (CFM_EINVAL: the fused small-field path
        is switched off, or t_span has more points than the workspace holds) and the caller steps it generically."""
        rc, what, traj, nfe, steps, _ = _solve_hip("gradmlp" if grad else "mlp", m, x, t_span, self.solver, self.atol, self.rtol)
        if grad and rc == -1:
            return None
        check(rc, what)
        self.nfe, self.n_steps = nfe, steps
        return traj.to(x.device)

    # ---- generic vector fields: same algorithm at tensor level ----
    def _trajectory_generic(self, x, t_span, record=None, max_steps=None):
        """record (adaptive solvers): a list that receives (t, dt, t_k1, out) of every accepted step, the step log of
        AdaptiveDifferentiableNeuralODE; more than max_steps of them raise."""
        f = self.vf
        ts = torch.as_tensor(t_span, dtype=torch.float32)
        sol = [x]
        self.nfe = 0
        # a decreasing grid: the adaptive solvers integrate g(s, y) = -f(-s, y) on s = -t_span (the fixed-step ones
        # step dt < 0 as it is: the same numbers in fp32)
        adaptive = self.solver in ADAPTIVE_TABLEAUS
        sign = -1.0 if (adaptive and len(ts) > 1 and float(ts[1]) < float(ts[0])) else 1.0
        if sign < 0:
            ts = -ts

        def ev(t, y):
            self.nfe += 1
            if sign < 0:
                return -f(torch.as_tensor(-np.float32(t), dtype=torch.float32, device=y.device), y)
            return f(torch.as_tensor(t, dtype=torch.float32, device=y.device), y)

        if self.solver == "euler":
            for k in range(len(ts) - 1):
                dt = float(ts[k + 1] - ts[k])
                x = x + dt * ev(float(ts[k]), x)
                sol.append(x)
            self.n_steps = len(ts) - 1
            return torch.stack(sol)
        if not adaptive:
            tab = FIXED_TABLEAUS[self.solver]
            for k in range(len(ts) - 1):
                t, dt = np.float32(ts[k]), np.float32(ts[k + 1] - ts[k])
                ks = [ev(float(t), x)]
                for c, row in zip(tab["c"], tab["a"]):
                    y = x + float(dt) * sum(float(a) * kq for a, kq in zip(row, ks))
                    ks.append(ev(float(t + np.float32(c) * dt), y))
                x = x + float(dt) * sum(float(b) * kq for b, kq in zip(tab["b"], ks))
                sol.append(x)
            self.n_steps = len(ts) - 1
            return torch.stack(sol)
        tab = ADAPTIVE_TABLEAUS[self.solver]
        tab_a, tab_c, tab_e = tab["a"], tab["c"], tab["e"]
        order = np.float32(tab["order"])
        atol, rtol = self.atol, self.rtol
        f32 = np.float32
        t, T = f32(ts[0]), f32(ts[-1])
        k1 = ev(t, x)
        scale = atol + x.abs() * rtol
        d0, d1 = f32(float(_hairer_norm(x / scale))), f32(float(_hairer_norm(k1 / scale)))
        h0 = f32(1e-6) if (d0 < 1e-5 or d1 < 1e-5) else f32(0.01) * d0 / d1
        f1 = ev(t + h0, x + h0 * k1)
        d2 = f32(float(_hairer_norm((f1 - k1) / scale))) / h0
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = max(f32(1e-6), h0 * f32(1e-3))
        else:
            h1 = f32(f32(0.01) / max(d1, d2)) ** (f32(1.0) / (order + f32(1.0)))
        dt = f32(min(f32(100) * h0, h1))
        ckpt, steps = 1, 0
        tk1 = t                     # where k1 was evaluated (FSAL: the accepted step's last stage time, not t after a landing)
        while t < T:
            if record is not None and len(record) >= max_steps:
                raise RuntimeError(f"the step log is full: max_steps = {max_steps} accepted steps did not reach the end "
                                   f"of t_span (t = {float(sign * t)}); raise max_steps")
            if t + dt > T:
                dt = f32(T - t)
            dt_old, flag = dt, False
            if ckpt < len(ts) and t + dt > f32(ts[ckpt]):
                dt_old, flag, dt = dt, True, f32(f32(ts[ckpt]) - t)
            lands = ckpt < len(ts) and (flag or t + dt == f32(ts[ckpt]))
            ks = [k1]
            for s in range(6):
                y = x + float(dt) * sum(float(a) * k for a, k in zip(tab_a[s], ks))
                ks.append(ev(t + f32(tab_c[s]) * dt, y))
            x_new = y
            err = float(dt) * sum(float(e) * k for e, k in zip(tab_e, ks))
            ratio = f32(float(_hairer_norm(err / (atol + rtol * torch.max(x.abs(), x_new.abs())))))
            steps += 1
            if ratio <= 1:
                if record is not None:
                    record.append((float(t), float(dt), float(tk1), ckpt if lands else -1))
                    tk1 = f32(t + f32(tab_c[5]) * dt)
                if lands:
                    t = f32(ts[ckpt]); sol.append(x_new); ckpt += 1
                else:
                    t = f32(t + dt)
                x, k1 = x_new, ks[6]
            if flag:
                dt = f32(dt_old - dt)
            if ratio == 0:
                factor = f32(10)
            else:
                minf = f32(1.0) if ratio < 1 else f32(0.2)
                factor = min(f32(10), max(f32(0.9) / ratio ** (f32(1.0) / order), minf))
            dt = f32(dt * factor)
            if not dt > 1e-12:
                dt = f32(1e-12)
        self.n_steps = steps
        return torch.stack(sol)


class _Declined(Exception):
    """A fused entry answered CFM_EINVAL inside its envelope: the fused small-field path is switched off, or (the solves)
    the grid has more points than the solve's workspace holds (n_t > 3 B width).  The caller runs its generic path."""


def _solve_forward(ctx, what, x, ts, dims, params, mid, after=(), declines=False, tail=None):
    """The forward of a differentiable solve of a 4-layer net: one call of the entry ``what`` with ``mid``
    between the grid and the trajectory and ``after`` behind it.  params: the flat (W_0, b_0, W_1, ...) inputs of the
    Function; ts: the float32 host grid.  Saves the trajectory [n_t, B, width] and the parameters on ctx for
    ``_solve_backward`` and returns the trajectory.  declines: CFM_EINVAL raises ``_Declined`` instead of an error.
    tail: a recording solve's ``(alloc, done)``: ``alloc(B, width, dev)`` gives the entry's arguments between nfe and the
    workspace, ``done(rc, nfe)`` looks at the return code before it is checked and gives the tensors that are saved in
    the trajectory's place."""
    lib = _lib.load()
    dev = x.device
    Ws, bs, Wp, bp = _lib.param_tables(params, dev)
    cdims = (ctypes.c_int * 5)(*dims)
    xd = _lib.to_dev_f32(x, dev)
    B, width = xd.shape
    n_t = ts.shape[0]
    traj = torch.empty((n_t, B, width), dtype=torch.float32, device=dev)
    ws = _lib.workspace(_lib.OP_ODE, B, max(dims[1:4]), width, dev)
    nfe = ctypes.c_int(0)
    rc = getattr(lib, what)(Wp, bp, cdims, 4, ptr(xd), B, ts.ctypes.data_as(ctypes.c_void_p), n_t, *mid, ptr(traj), *after,
                            ctypes.byref(nfe), *(tail[0](B, width, dev) if tail else ()), ptr(ws), stream_ptr())
    if declines and rc == -1:
        raise _Declined()
    state = tail[1](rc, nfe.value) if tail else (traj,)
    check(rc, what)
    ctx.ts, ctx.dims, ctx.n_state = ts, dims, len(state)
    ctx.save_for_backward(*state, *params)
    return traj


def _solve_backward(ctx, what, op, g, mid, n_other, head=None):
    """The backward of ``_solve_forward``: one call of the entry ``what`` over the saved trajectory, with ``mid`` between
    the grid and the upstream gradient g; ``op`` sizes its workspace.  Returns the Function's gradients: the state's (if
    needed), None for its ``n_other`` further non-parameter inputs, then (dW_0, db_0, dW_1, ...).
    head: a recording solve's ``head(state, B, n_t)``: the entry's arguments between the layer count and ``mid``, from the
    tensors its forward saved (the first of them [., B, width]), in place of (trajectory, B, grid, n_t)."""
    lib = _lib.load()
    state, params = ctx.saved_tensors[:ctx.n_state], ctx.saved_tensors[ctx.n_state:]
    dev = state[0].device
    Ws, bs, Wp, bp = _lib.param_tables(params, dev)
    dWs, dbs, dWp, dbp = _lib.grad_tables(Ws, bs)
    cdims = (ctypes.c_int * 5)(*ctx.dims)
    n_t, (B, width) = ctx.ts.shape[0], state[0].shape[1:]
    gd = _lib.to_dev_f32(g, dev)
    g0 = torch.empty((B, width), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
    ws = _lib.workspace(op, B, n_t, 0, dev)
    first = head(state, B, n_t) if head else (ptr(state[0]), B, ctx.ts.ctypes.data_as(ctypes.c_void_p), n_t)
    check(getattr(lib, what)(Wp, bp, cdims, 4, *first, *mid, ptr(gd), dWp, dbp, ptr(g0), ptr(ws), stream_ptr()), what)
    grads = [None] * len(params)
    grads[0::2] = dWs
    grads[1::2] = dbs
    return (g0, *[None] * n_other, *grads)


class _FixedStepODEFunction(torch.autograd.Function):
    """The trajectory [n_t, B, d] of a fixed-step solve (cfm_ode_fixed_mlp_f32); backward: cfm_ode_fixed_grad_f32."""

    @staticmethod
    def forward(ctx, x, ts, scheme, dims, *params):
        ctx.scheme = scheme
        return _solve_forward(ctx, "cfm_ode_fixed_mlp_f32", x, ts, dims, params, (scheme,))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _solve_backward(ctx, "cfm_ode_fixed_grad_f32", _lib.OP_ODE_GRAD, g, (ctx.scheme,), 3)


class DifferentiableNeuralODE(NeuralODE):
    """``NeuralODE`` whose trajectory carries a gradient: a loss can be put on ``node(x, t_span)`` (what the reference's
    ``sensitivity="adjoint"`` is for: examples/images/cifar10/utils_cifar.py:63).

    ``solver``: ``euler``, ``midpoint`` or ``rk4``.  ``trajectory(x, t_span)`` returns ``[n_t, B, d]``, differentiable
    with respect to ``x`` and the field's parameters (not ``t_span``); the grid may be decreasing.  The gradient is that
    of the Runge-Kutta recurrence the forward ran (discretise-then-optimise); torchdyn's ``"adjoint"``
    integrates the continuous adjoint with the same solver, which differs from it by the scheme's truncation error and is
    unpinned, as the forward solvers are.

    ``last_path == "hip"``: the field is ``torch_wrapper(MLP(time_varying=True))`` of the small-kernel envelope (4 layers,
    widths <= 64), the state is 2-D fp32 CUDA, every parameter is fp32 on its device and the library takes the solve
    (``cfm_ode_fixed_grad_available``).  The forward is ``cfm_ode_fixed_mlp_f32``, bit-equal to
    ``NeuralODE(vf, solver=s).trajectory(x, t_span)``; the backward is one call of ``cfm_ode_fixed_grad_f32`` over the saved
    trajectory, once differentiable.  ``"generic"``: everything else (CPU, float64, wider nets, other fields, the fused
    path switched off) runs the parent's recurrence in differentiable torch ops.  Nothing is printed."""

    def __init__(self, vector_field, solver="euler", **kwargs):
        super().__init__(vector_field, solver=solver, **kwargs)
        if solver not in _lib.ODE_SCHEME:
            raise NotImplementedError(f"solver {solver!r}: the gradient is that of a fixed-step recurrence; "
                                      f"one of {tuple(_lib.ODE_SCHEME)}")

    def _hip_grad_mlp(self, x):
        """The MLP when cfm_ode_fixed_grad_f32 takes the solve of this state, else None."""
        from .cnf import _small_envelope
        m = self._hip_mlp()
        if m is None or x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32 or not _small_envelope(m, x.shape[1]):
            return None
        lins = m._linears()
        if lins[3].bias is None or not all(p.dtype == torch.float32 and p.device == x.device for p in m.parameters()):
            return None
        if _lib.load().cfm_ode_fixed_grad_available((ctypes.c_int * 5)(*m.dims()), 4) != 0:
            return None
        return m

    def trajectory(self, x, t_span):
        ts = torch.as_tensor(t_span).detach().to(dtype=torch.float32).cpu()
        _check_t_span(ts)
        m = self._hip_grad_mlp(x)
        if m is None:
            self.last_path = "generic"
            return self._trajectory_generic(x, ts)
        lins = m._linears()
        params = [p for l in lins for p in (l.weight, l.bias)]
        dims = m.dims()
        scheme = _lib.ODE_SCHEME[self.solver]
        self.last_path = "hip"
        self.n_steps = ts.numel() - 1
        self.nfe = len(FIXED_TABLEAUS[self.solver]["b"]) * self.n_steps
        return _FixedStepODEFunction.apply(x, np.ascontiguousarray(ts.numpy()), scheme, dims, *params)


class _AdaptiveODEFunction(torch.autograd.Function):
    """The trajectory [n_t, B, d] of an adaptive solve that records its accepted steps (cfm_ode_adaptive_rec_mlp_f32);
    backward: cfm_ode_adaptive_grad_f32 over ysteps[:n_accepted] and the log.  ``out`` (a dict) receives nfe, n_steps,
    n_accepted and step_log."""

    @staticmethod
    def forward(ctx, x, ts, tab, atol, rtol, max_steps, out, dims, *params):
        steps, n_acc = ctypes.c_int(0), ctypes.c_int(0)
        bufs = []

        def alloc(B, width, dev):
            bufs.append(torch.empty((max_steps, 4), dtype=torch.float32, device=dev))            # 16-byte records
            bufs.append(torch.empty((max_steps, B, width), dtype=torch.float32, device=dev))
            return max_steps, ptr(bufs[0]), ptr(bufs[1]), ctypes.byref(n_acc)

        def done(rc, nfe):
            if rc == -3 and n_acc.value >= max_steps:
                raise RuntimeError(f"cfm_ode_adaptive_rec_mlp_f32: the step log is full: max_steps = {max_steps} accepted "
                                   "steps did not reach the end of t_span; raise max_steps")
            n = n_acc.value
            log = bufs[0][:n].clone()
            host = log.cpu()
            out.update(nfe=nfe, n_steps=steps.value, n_accepted=n, step_log=torch.cat(
                [host[:, :3].double(), host.view(torch.int32)[:, 3:].double()], 1))
            return bufs[1][:n].clone(), log          # (copies: the max_steps buffers go back to the allocator)

        ctx.tab, ctx.tsign = tab, (-1.0 if ts[1] < ts[0] else 1.0)
        return _solve_forward(ctx, "cfm_ode_adaptive_rec_mlp_f32", x, ts, dims, params, (tab, atol, rtol),
                              (ctypes.byref(steps),), declines=True, tail=(alloc, done))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        def head(state, B, n_t):
            return ptr(state[0]), ptr(state[1]), state[0].shape[0], B, n_t
        return _solve_backward(ctx, "cfm_ode_adaptive_grad_f32", _lib.OP_ODE_GRAD, g, (ctx.tab, ctx.tsign), 7, head=head)


class AdaptiveDifferentiableNeuralODE(NeuralODE):
    """``NeuralODE`` on ``dopri5`` / ``tsit5`` whose trajectory carries a gradient: the reference's standard sampler call
    ``NeuralODE(torch_wrapper(model), solver="dopri5", sensitivity="adjoint", atol, rtol)`` with a loss on it.

    ``trajectory(x, t_span)`` returns ``[n_t, B, d]`` (n_t >= 2, either direction), differentiable with respect to ``x`` and
    the field's parameters.  The gradient is that of the recurrence of ACCEPTED steps the forward ran, the step sequence
    taken as a constant (discretise-then-optimise): rejected attempts contribute nothing and nothing flows
    through the controller, ``t_span``, ``atol`` or ``rtol``.  It is autograd through ``NeuralODE._trajectory_generic``,
    whose controller reads Python floats only.

    After a call: ``last_path``, ``nfe``, ``n_steps`` (attempts), ``n_accepted`` and ``step_log``, a ``[n_accepted, 4]``
    float64 CPU tensor of ``t, dt, t_k1, out`` per accepted step: solver-space (sign * t) start and size, the time its
    first slope was evaluated at, the ``t_span`` index its end lands on or -1.  More than ``max_steps`` accepted steps
    raise a ``RuntimeError``; there is no second solve.

    ``last_path == "hip"``: the envelope of ``DifferentiableNeuralODE`` and the one-launch adaptive kernel takes the solve
    (``B d >= n_t``).  Forward ``cfm_ode_adaptive_rec_mlp_f32``, bit-equal to ``NeuralODE(vf, solver).trajectory``; backward
    one call of ``cfm_ode_adaptive_grad_f32``, once differentiable.  ``"generic"``: everything else, the parent's loop in
    differentiable torch ops."""

    def __init__(self, vector_field, solver="dopri5", atol=1e-3, rtol=1e-3, max_steps=512, **kwargs):
        if solver not in ADAPTIVE_TABLEAUS:
            raise NotImplementedError(f"solver {solver!r}: the adaptive pairs, one of {tuple(ADAPTIVE_TABLEAUS)} "
                                      "(DifferentiableNeuralODE has the fixed-step schemes)")
        super().__init__(vector_field, solver=solver, atol=atol, rtol=rtol, **kwargs)
        if int(max_steps) < 1:
            raise ValueError("max_steps must be at least 1")
        self.max_steps = int(max_steps)
        self.n_accepted = 0
        self.step_log = None

    def _hip_grad_mlp(self, x):
        """The MLP when cfm_ode_adaptive_grad_f32 takes the solve of this state, else None: the envelope test of
        DifferentiableNeuralODE._hip_grad_mlp (borrowed, not restated), then the adaptive entry's own answer."""
        m = DifferentiableNeuralODE._hip_grad_mlp(self, x)
        if m is None or _lib.load().cfm_ode_adaptive_grad_available((ctypes.c_int * 5)(*m.dims()), 4) != 0:
            return None
        return m

    def trajectory(self, x, t_span):
        ts = torch.as_tensor(t_span).detach().to(dtype=torch.float32).cpu()
        _check_t_span(ts)
        if ts.numel() < 2:
            raise ValueError("an adaptive solve needs at least two t_span points")
        m = self._hip_grad_mlp(x)
        if m is not None:
            params = [p for l in m._linears() for p in (l.weight, l.bias)]
            out = {}
            try:
                traj = _AdaptiveODEFunction.apply(x, np.ascontiguousarray(ts.numpy()), _lib.ODE_TABLEAU[self.solver], self.atol,
                                                  self.rtol, self.max_steps, out, m.dims(), *params)
            except _Declined:             # B d < n_t, or the fused path was switched off after the envelope test: the entry
                                          # declines before any GPU work; whatever fails later is an error, not a decline
                traj = None
            if traj is not None:
                self.last_path = "hip"
                self.nfe, self.n_steps, self.n_accepted, self.step_log = out["nfe"], out["n_steps"], out["n_accepted"], out["step_log"]
                return traj
        self.last_path = "generic"
        record = []
        traj = self._trajectory_generic(x, ts, record=record, max_steps=self.max_steps)
        self.n_accepted = len(record)
        self.step_log = torch.tensor(record, dtype=torch.float64).reshape(-1, 4)
        return traj
