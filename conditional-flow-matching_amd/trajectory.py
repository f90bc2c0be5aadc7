"""Multi-marginal flow matching on time-series snapshots ``X [B, T, d]`` — the ``is_trajectory`` branch of the
reference's runner (cited as ``run:LINE`` into ``runner/src/models/cfm_module.py``): ``preprocess_batch`` run:142-199,
``calc_loc_and_target`` run:225-242 and ``SplineCFMLitModule`` run:1352-1409, without the ``HAS_JOINT_PLANS`` branch.

One call draws an interval per row, couples the consecutive slices (the couplings of a call go to the solver together), and
evaluates location and target of every row in ONE fused HIP launch (``cfm_traj_xt_ut_f32``): the kernel reads each
row's interval, gathers its operands from ``X`` through the device-resident index pairs (linear) or the chain of draws
(spline), evaluates the interpolant, adds the noise and applies the leave-out rule.  The indices never visit the host.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .conditional_flow_matching import (ConditionalFlowMatcher, ExactOptimalTransportConditionalFlowMatcher,
                                        ScheduledBridgeConditionalFlowMatcher,
                                        SchrodingerBridgeConditionalFlowMatcher, pad_t_like_x)

MAX_FUSED_KNOTS = 32        # TRAJ_MAX_KNOTS of csrc/traj.hip: more knots take the eager path
_ACCEPTED = (ConditionalFlowMatcher, ExactOptimalTransportConditionalFlowMatcher, SchrodingerBridgeConditionalFlowMatcher,
             ScheduledBridgeConditionalFlowMatcher)
_BRIDGES = (_lib.VARIANT_SB, _lib.VARIANT_SCHED)      # Brownian-bridge paths: linear interpolant only
_ONE_WORKGROUP_ROWS = 256   # batches up to this size are solved by one workgroup (optimal_transport._solve_many)
_S_CACHE = {}


def natural_spline_map(knots):
    """The map S (float64 [n, n]) from knot values to the second derivatives at the knots of the natural cubic spline
    through them: ``S @ y``.  Rows 0 and n - 1 are zero (the natural end conditions); every row sums to zero.  Solved
    once per knot vector from the usual tridiagonal system and cached."""
    key = tuple(float(x) for x in knots)
    S = _S_CACHE.get(key)
    if S is None:
        tau = np.asarray(key, dtype=np.float64)
        n = tau.size
        if n < 2 or not np.all(np.diff(tau) > 0):
            raise ValueError("natural_spline_map needs at least two strictly increasing knots")
        A, R = np.zeros((n, n)), np.zeros((n, n))
        A[0, 0] = A[n - 1, n - 1] = 1.0
        for k in range(1, n - 1):
            h0, h1 = tau[k] - tau[k - 1], tau[k + 1] - tau[k]
            A[k, k - 1], A[k, k], A[k, k + 1] = h0, 2.0 * (h0 + h1), h1
            R[k, k - 1], R[k, k], R[k, k + 1] = 6.0 / h0, -6.0 / h0 - 6.0 / h1, 6.0 / h1
        S = np.linalg.solve(A, R)
        S.setflags(write=False)
        if len(_S_CACHE) >= 64:
            _S_CACHE.pop(next(iter(_S_CACHE)))
        _S_CACHE[key] = S
    return S


class TrajectoryFlowMatcher:
    """Flow matching across ``T`` snapshots with one of this package's matchers as the conditional path.

    ``FM`` fixes coupling and path: ``ConditionalFlowMatcher(sigma)`` — no coupling;
    ``ExactOptimalTransportConditionalFlowMatcher(sigma)`` — consecutive slices coupled by its ``ot_sampler``;
    ``SchrodingerBridgeConditionalFlowMatcher(sigma, ...)`` — its coupling and the Brownian-bridge path (linear
    interpolant only); ``ScheduledBridgeConditionalFlowMatcher(schedule, ...)`` — the same with a noise schedule, read at
    the row's local time (linear interpolant only).  (An ``FM`` whose ``ot_sampler`` attribute is ``None`` does not couple, like ``self.ot_sampler
    is None`` at run:158.)  ``leaveout_timepoint`` ``L`` holds slice ``L`` out of TRAINING calls (run:152-160, :167-170):
    ``-1`` for none, else ``1 <= L <= T - 2`` (checked against every ``X``).

    ``interpolant="linear"`` (run:142-199, :225-242) — per interval ``k`` the pair is ``(X[:, k], X[:, k + 1])``, or
    ``(X[:, k], X[:, k + 2])`` when training and ``k + 1 == L``; when training and ``FM`` couples, every pair but
    interval ``L`` (never selected) is resampled from its plan.  Row ``b`` takes row ``b`` of the pair of its interval
    ``t_select[b]``; ``xt`` / ``ut`` are ``FM``'s closed forms at the local time ``t``; rows with
    ``t_select + 1 == L`` get ``ut / 2`` and ``t * 2``; ``t_net = t + t_select``.

    ``interpolant="spline"`` (run:1355-1409) — when training with ``L > 0`` slice ``L`` is dropped; the knots are the
    remaining slice numbers ``tau``.  The trajectories are ``ot_sampler.sample_trajectory``'s chain over the remaining
    slices (the identity chain without a coupling); ``t_select`` picks a knot interval ``i``, ``u = rand``,
    ``t_net = tau_i + u (tau_{i+1} - tau_i)``, and ``mu`` / ``ut`` are value and time derivative at ``t_net`` of the
    natural cubic spline through ``(tau_k, traj[b, k])``; ``xt = mu + sigma * eps``.

    Order of the draws: (1) the plan draws, interval by interval — ``np.random`` is consumed as a loop of
    ``sample_plan`` calls (linear) or as ``sample_trajectory`` (spline) consumes it; (2) ``t_select = torch.randint(T - 2
    if leave-out else T - 1, (B,))`` on the CPU generator, entries ``>= L`` then incremented (spline: ``randint(T' -
    1)``, no increment: it indexes knot intervals); (3) ``t = torch.rand(B)`` on the CPU generator; (4) ``eps =
    randn_like`` on ``X``'s device.

    Deviations from the reference, on purpose:

    * the reference draws ``t_select`` on ``X.device`` in the leave-out case only (run:169) and on the CPU otherwise
      (run:172); here it always comes from the CPU generator, like ``t``;
    * the reference draws ``t_select`` before the OT chain in the spline module (run:1366-1371) and, there, applies
      ``t *= 2`` to ``u + t_select`` and ``ut /= 2`` on the interval across the gap under a "TODO handle leaveout case"
      (run:1363, :1402-1404) although its spline already runs on the true knot times.  Here the interval across the gap
      simply has width 2: ``t_net`` and ``ut`` are the spline's own time and derivative, with no further rescaling;
    * ``L = 0`` and ``L >= T - 1`` are refused (the reference indexes out of range at ``L = T - 1`` and ``L = 0``
      switches its own rule off).

    ``last_path`` is ``"hip"`` when the last call ran the fused kernel and ``"eager"`` when it ran the same
    composition in differentiable torch ops: CPU tensors, non-fp32 inputs, inputs that require grad, a subclassed
    ``FM`` that overrides a closed form, or more than 32 knots.
    """

    def __init__(self, FM, interpolant="linear", leaveout_timepoint=-1):
        if type(FM) not in _ACCEPTED and not (isinstance(FM, _ACCEPTED) and
                                              FM._variant in (_lib.VARIANT_ICFM,) + _BRIDGES):
            raise ValueError("TrajectoryFlowMatcher takes a ConditionalFlowMatcher, an "
                             "ExactOptimalTransportConditionalFlowMatcher, a SchrodingerBridgeConditionalFlowMatcher or a "
                             f"ScheduledBridgeConditionalFlowMatcher; got {type(FM).__name__}")
        if interpolant not in ("linear", "spline"):
            raise ValueError(f"interpolant must be 'linear' or 'spline', got {interpolant!r}")
        if interpolant == "spline" and FM._variant in _BRIDGES:
            raise ValueError("interpolant='spline' has no Schrodinger-bridge path: use interpolant='linear' with a "
                             f"{type(FM).__name__}")
        L = int(leaveout_timepoint)
        if L != -1 and L < 1:
            raise ValueError(f"leaveout_timepoint must be -1 or 1 <= L <= T - 2, got {leaveout_timepoint}")
        self.FM = FM
        self.interpolant = interpolant
        self.leaveout_timepoint = L
        self.last_path = None

    # ------------------------------------------------------------------------------------------------ helpers
    def _couples(self):
        return getattr(self.FM, "ot_sampler", None) is not None

    @staticmethod
    def _override(z, B, name):
        if z is not None and (not isinstance(z, torch.Tensor) or z.dim() < 1 or z.shape[0] != B):
            raise ValueError(f"{name} must be a tensor with the batch size {B} of X in front, got "
                             f"{tuple(z.shape) if isinstance(z, torch.Tensor) else type(z).__name__}")
        return z

    def _draws(self, Xf, n_intervals, shift_from, t_select, t, eps):
        """Steps 2-4 of the draw order.  shift_from: entries >= it are incremented (linear leave-out), or None."""
        B, _, d = Xf.shape
        t_select = self._override(t_select, B, "t_select")
        t = self._override(t, B, "t")
        eps = self._override(eps, B, "eps")
        if t_select is None:
            t_select = torch.randint(n_intervals, size=(B,))
            if shift_from is not None:
                t_select[t_select >= shift_from] += 1
        else:
            if t_select.dim() != 1 or t_select.dtype.is_floating_point:
                raise ValueError("t_select must be an integer vector [B]")
            hi = n_intervals + (1 if shift_from is not None else 0)
            bad = (t_select < 0) | (t_select >= hi)
            if shift_from is not None:
                bad = bad | (t_select == shift_from)
            if bool(bad.any()):
                raise ValueError(f"t_select out of range: intervals 0 .. {hi - 1}"
                                 + (f" without {shift_from}" if shift_from is not None else ""))
        t_select = t_select.to(device=Xf.device, dtype=torch.int64)
        if t is None:
            t = torch.rand(B)
        elif t.numel() != B:
            raise ValueError(f"t must have {B} entries, got {tuple(t.shape)}")
        t = t.reshape(B).to(device=Xf.device, dtype=Xf.dtype)
        if eps is None:
            eps = torch.randn((B, d), dtype=Xf.dtype, device=Xf.device)
        elif eps.numel() != B * d:
            raise ValueError(f"eps must have the shape of one slice of X, [{B}, {d}]; got {tuple(eps.shape)}")
        eps = eps.reshape(B, d).to(device=Xf.device, dtype=Xf.dtype)
        return t_select, t, eps

    def _fused(self, Xf, t, eps, knots=None):
        if not Xf.is_cuda or self.FM._customised() or self.FM._needs_eager(Xf, t, eps):
            return False
        return knots is None or knots <= MAX_FUSED_KNOTS

    def _launch(self, mode, Xf, idx, t_select, t, eps, sigma_t, leave, S):
        lib = _lib.load()
        B, T, d = Xf.shape
        Xc, tc, ec = Xf.detach().contiguous(), t.contiguous(), eps.contiguous()      # (held until the launch is queued)
        xt = torch.empty((B, d), dtype=torch.float32, device=Xf.device)
        ut = torch.empty((B, d), dtype=torch.float32, device=Xf.device)
        t_net = torch.empty(B, dtype=torch.float32, device=Xf.device)
        sigma = 0.0 if self.FM._variant == _lib.VARIANT_SCHED else float(self.FM.sigma)      # (the schedule is in the table)
        with torch.cuda.device(Xf.device):
            check(lib.cfm_traj_xt_ut_f32(mode, self.FM._variant, ptr(Xc), B, T, d, ptr(idx), ptr(t_select),
                                         ptr(tc), ptr(ec), sigma, ptr(sigma_t),
                                         leave, ptr(S), ptr(xt), ptr(ut), ptr(t_net), stream_ptr()), "cfm_traj_xt_ut_f32")
        return t_net, xt, ut

    # ------------------------------------------------------------------------------------------------ linear
    def _linear(self, Xf, training, t_select, t, eps):
        B, T, d = Xf.shape
        L = self.leaveout_timepoint
        leave = L if (training and L > 0) else 0
        pairs = [(k, k + 2 if (leave and k + 1 == leave) else k + 1) for k in range(T - 1)]
        # (1) the couplings, solved together; their draws in interval order (run:151-163)
        idx = None
        if training and self._couples():
            sampler = self.FM.ot_sampler
            coupled = [k for k in range(T - 1) if k != L]
            batches = [(Xf[:, pairs[k][0]], Xf[:, pairs[k][1]]) for k in coupled]
            # Batches beyond the one-workgroup solver share ONE chain of launches (or one worker stream each); up to 256
            # rows a coupling is a launch or two on the caller's stream, and the worker threads cost more than they
            # overlap (measured: DESIGN.md 4.14), so those are issued back to back
            sols = sampler._solve_many(batches, workers=3 if B > _ONE_WORKGROUP_ROWS else 1, throughput=True)
            ident = None
            rows = []
            for k in range(T - 1):
                if k in coupled:
                    q = coupled.index(k)
                    i, j = sampler._indices_from_solution(batches[q][0], batches[q][1], sols[q])
                else:
                    if ident is None:
                        ident = torch.arange(B, dtype=torch.int64, device=sols[0].M.device)
                    i = j = ident
                rows += [i, j]
            idx = torch.stack(rows).reshape(T - 1, 2, B)
        # (2)-(4)
        t_select, t, eps = self._draws(Xf, T - 2 if leave else T - 1, leave if leave else None, t_select, t, eps)
        fused = self._fused(Xf, t, eps)
        self.last_path = "hip" if fused else "eager"
        if fused:
            sigma_t = None
            if self.FM._variant == _lib.VARIANT_SB:
                sigma_t = (self.FM.sigma * torch.sqrt(t * (1 - t))).contiguous()      # ref:446, eager, on t's device
            elif self.FM._variant == _lib.VARIANT_SCHED:
                sigma_t = torch.stack(self.FM._coefs(t), dim=1).contiguous()          # [B, 4] at the local times, on t's device
            t_net, xt, ut = self._launch(0, Xf, None if idx is None else idx.to(Xf.device), t_select, t, eps, sigma_t,
                                         leave, None)
            return t_net, xt, ut, eps, t, t_select
        # the reference's composition through FM's (possibly overridden) methods; the pairing is a differentiable gather
        k1 = t_select + 1
        halved = torch.zeros_like(t_select, dtype=torch.bool)
        if leave:
            halved = k1 == leave
            k1 = k1 + halved.to(k1.dtype)
        rb = torch.arange(B, device=Xf.device)
        r0 = r1 = rb
        if idx is not None:
            idx = idx.to(Xf.device)
            r0, r1 = idx[t_select, 0, rb], idx[t_select, 1, rb]
        x0, x1 = Xf[r0, t_select], Xf[r1, k1]
        xt = self.FM._impl("sample_xt")(x0, x1, t, eps)
        ut = self.FM._impl("compute_conditional_flow")(x0, x1, t, xt)
        t_net = t
        if leave:                                             # run:235-237
            ut = torch.where(pad_t_like_x(halved, ut), ut / 2, ut)
            t_net = torch.where(halved, t * 2, t)
        t_net = t_net + t_select                              # run:241
        return t_net, xt, ut, eps, t, t_select

    # ------------------------------------------------------------------------------------------------ spline
    def _spline(self, Xf, training, t_select, t, eps):
        B, T, d = Xf.shape
        L = self.leaveout_timepoint
        leave = L if (training and L > 0) else 0
        keep = [k for k in range(T) if k != leave] if leave else list(range(T))
        Tp = len(keep)
        # (1) the OT chain over the remaining slices (run:1367-1371)
        chain = None
        if self._couples():
            chain = self.FM.ot_sampler._trajectory_indices(Xf[:, keep] if leave else Xf)
        t_select, u, eps = self._draws(Xf, Tp - 1, None, t_select, t, eps)
        S64 = natural_spline_map(keep)
        fused = self._fused(Xf, u, eps, knots=Tp)
        self.last_path = "hip" if fused else "eager"
        if fused:
            S = torch.from_numpy(S64.astype(np.float32)).to(Xf.device)
            t_net, xt, ut = self._launch(1, Xf, None if chain is None else chain.to(Xf.device).contiguous(), t_select, u,
                                         eps, None, leave, S)
            return t_net, xt, ut, eps, u, t_select
        tau = torch.tensor(keep, dtype=Xf.dtype, device=Xf.device)
        S = torch.from_numpy(S64.copy()).to(device=Xf.device, dtype=Xf.dtype)
        rb = torch.arange(B, device=Xf.device)
        Xk = Xf[:, keep] if leave else Xf
        if chain is not None:
            Xk = Xk[chain.to(Xf.device).t(), torch.arange(Tp, device=Xf.device)[None, :]]     # traj [B, Tp, d]
        y0, y1 = Xk[rb, t_select], Xk[rb, t_select + 1]
        dy = Xk - y0[:, None, :]
        m0 = torch.einsum("bk,bkd->bd", S[t_select], dy)
        m1 = torch.einsum("bk,bkd->bd", S[t_select + 1], dy)
        h = (tau[t_select + 1] - tau[t_select])
        t_net = tau[t_select] + u * h
        h, uu = h[:, None], u[:, None]
        a = 1 - uu
        mu = a * y0 + uu * y1 + (h * h / 6) * ((a * a * a - a) * m0 + (uu * uu * uu - uu) * m1)
        ut = (y1 - y0) / h + (h / 6) * ((3 * uu * uu - 1) * m1 - (3 * a * a - 1) * m0)
        xt = mu + self.FM.sigma * eps
        return t_net, xt, ut, eps, u, t_select

    # ------------------------------------------------------------------------------------------------ public
    def sample_location_and_conditional_flow(self, X, training=True, return_noise=False, return_interval=False,
                                             t_select=None, t=None, eps=None):
        """``(t_net, xt, ut[, eps][, (t_local, t_select)])`` for trajectories ``X [B, T, *dim]``, ``T >= 2``.

        ``t_net [B]`` is the time the network sees, ``xt`` / ``ut`` ``[B, *dim]`` location and target, all on ``X``'s
        device and dtype — what ``RegressionStep`` takes, and with ``eps`` and ``FM.compute_lambda(t_local)`` what
        ``SF2MStep`` takes.  ``t_local`` is the time inside the interval (before the leave-out rule doubles it) and
        ``t_select [B]`` (int64) the interval of each row; for the spline, the knot interval among the remaining knots.
        ``t_select=``, ``t=``, ``eps=`` replace the corresponding draws (tests, reproducible loops)."""
        if not isinstance(X, torch.Tensor) or X.dim() < 3:
            raise ValueError("X must be a tensor [B, T, *dim]")
        B, T = X.shape[0], X.shape[1]
        if T < 2:
            raise ValueError(f"X needs at least two time slices, got T = {T}")
        L = self.leaveout_timepoint
        if L != -1 and not (1 <= L <= T - 2):
            raise ValueError(f"leaveout_timepoint must be -1 or 1 <= L <= T - 2 = {T - 2}, got {L}")
        Xf = X.reshape(B, T, -1)
        run = self._linear if self.interpolant == "linear" else self._spline
        t_net, xt, ut, eps, t_local, t_sel = run(Xf, bool(training), t_select, t, eps)
        shape = (B,) + tuple(X.shape[2:])
        fin = lambda z: z.reshape(shape).to(dtype=X.dtype)
        out = (t_net.to(dtype=X.dtype), fin(xt), fin(ut))
        if return_noise:
            out = out + (fin(eps),)
        if return_interval:
            out = out + ((t_local, t_sel),)
        return out
