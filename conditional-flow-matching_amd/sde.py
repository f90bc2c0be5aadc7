"""SDE sampling for SF2M — counterpart of how the reference draws stochastic trajectories:
``torchsde.sdeint(SDE(model, score_model, sigma), x0, ts)`` (examples/2D_tutorials/SF2M_tutorial.ipynb cell 5,
single-cell_example.ipynb, mnist_example.ipynb, conditional_mnist.ipynb) and ``FlowSolver.sdeint`` /
``forward_sde_drift`` / ``backward_sde_drift`` (runner/src/models/components/solver.py:129-139,157-182).

The notebooks name no method (the tutorial's ``solver="euler"`` is a keyword torchsde ignores with a warning), so for
their ``noise_type = "diagonal"``, ``sde_type = "ito"`` classes torchsde runs its default ``srk`` (Roessler's SRI2W1,
strong order 1.5); the runner passes ``method=self.sde_solver``.  Both are built here: ``method="euler"`` (this
package's default) is fixed-step Euler-Maruyama on the ``ts`` grid refined to steps of at most ``dt`` (torchsde's
Euler scheme), ``method="srk"`` is SRI2W1 for the constant diagonal noise all of the reference's SDE classes have.
A script that relied on torchsde's default passes ``method="srk"`` explicitly.  When the drift and the score are
``cfm_amd.MLP`` fields the network evaluations run on the HIP inference kernels and the state update is one fused HIP
kernel per step (``cfm_sde_em_step_f32``) or stage (``cfm_sde_srk_step_f32``); any other callable pair is stepped by
the same scheme in eager torch.
``sigma`` may be a noise schedule (``cfm_amd.schedule``, or any callable of the time with a scalar value): the same
kernels run it — g is evaluated once per refined step on the host, at the SOLVER's time t_k at the start of the step,
also for ``reverse=True`` (what the reference's SDE classes and the eager scheme here do); a user who wants g(1 - t) on
the way back passes ``lambda t: schedule(1 - t)``.  ``srk`` with a schedule is not built.
The Brownian increments come from ``torch.randn`` on the state's device (torchsde's BrownianInterval
stream is not reproducible without torchsde: the noise stream is NOT bit-compatible, the scheme is).
Under ``noise="philox"`` the one-launch kernels draw them themselves: Philox4x32-10 keyed by one ``torch.randint(0, 2**62)``
draw of the generator per ``sdeint`` call, counter (element, refined step, stream), 24-bit uniforms and Box-Muller
(include/cfm_gfx950.h has the layout) — a stream of its own, pinned element by element to the host restatement
``tests/philox_ref.py`` (``tests/test_gpu_sde_philox.py``), in which a row's noise depends on its position in the batch
and the seed, not on the batch size.

``logqp=True`` (``sdeint``, ``FlowSolver.sdeint``, ``DSBMFlowSolver.sdeint``: the validation loop of the runner's SF2M and
DSBM modules, cfm_module.py:911-983) returns ``(ys, log_ratio_increments)`` as ``torchsde.sdeint`` does.  Recalled, not read
(torchsde is not installed here): its ``SDELogqp`` for diagonal noise adds one state column with drift
``0.5 * (u ** 2).sum(1)``, ``u = stable_division(f - h, g)`` (every ``|g| <= 1e-7`` replaced by ``1e-7 * sign(g)``), zero
diffusion and zero start, and ``sdeint`` returns the column's INCREASE over each interval of ``ts`` (``[len(ts) - 1, B]``,
not cumulative) next to the state without it.  Here the column is one more drift-only component of the scheme that runs
the state, on the refined grid: ``euler`` adds ``h_k * q(t_k, y_k)`` with f and g of the state update of step k; ``srk``
adds ``(h / 6) ((q1 + q2) + 4 q3)`` on the three stage drifts (the column's own stage values enter nothing).  The
Brownian increments keep their shapes (torchsde would draw one more column, which multiplies zero).  The one-launch
kernels accumulate it from the drift tile they hold (``h = 0``: csrc/sde_small.h, LOGQP), the launch-per-step path in a
few torch ops per step, the eager path from ``sde.h`` where the object has one; the trajectory is the same bits with
and without it.
"""
import math

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .models import MLP, time_mlp
from .schedule import ConstantNoiseScheduler, CosineNoiseScheduler, LinearDecreasingNoiseScheduler

_BUILTIN_SCHEDULES = (ConstantNoiseScheduler, LinearDecreasingNoiseScheduler, CosineNoiseScheduler)


class FlowScoreSDE(torch.nn.Module):
    """dy = (drift([y, t]) + score([y, t])) dt + sigma dW — the ``SDE`` class of the SF2M tutorial
    (``reverse=True``: backward drift -drift + score evaluated at 1 - t, solver.py:129-139,32-35)."""
    noise_type = "diagonal"
    sde_type = "ito"
    negate_reverse = True      # reverse=True flips the sign of the drift net (DriftSDE does not)

    def __init__(self, drift, score, sigma=1.0, reverse=False):
        super().__init__()
        self.drift, self.score, self.sigma, self.reverse = drift, score, sigma, reverse
        self.last_path = None      # "hip" / "eager": what the last sdeint call on this object ran

    def _cat(self, t, y):
        tt = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        tt = tt.repeat(y.shape[0])[:, None] if tt.dim() == 0 else tt.reshape(-1, 1)
        return torch.cat([y, tt], 1)

    def f(self, t, y):
        if self.reverse:
            x = self._cat(1 - t, y)
            return -self.drift(x) + self.score(x)
        x = self._cat(t, y)
        return self.drift(x) + self.score(x)

    def g(self, t, y):
        s = self.sigma(t) if callable(self.sigma) else self.sigma
        return torch.ones_like(y) * s

    def h(self, t, y):
        """The prior drift of ``sdeint(..., logqp=True)``: zero (runner/src/models/components/solver.py:43-44)."""
        return torch.zeros_like(y)


class DriftSDE(torch.nn.Module):
    """dy = drift([y, t]) dt + sigma dW — ONE drift net, as DSBM trains them (runner/src/models/components/solver.py:249-257
    behind the SDE class of :35-41).  ``reverse=True``: the drift is evaluated at 1 - t and enters with a PLUS sign (the
    backward net IS the drift of the time-reversed process); ``sigma`` is read at the solver's time, as for
    ``FlowScoreSDE``."""
    noise_type = "diagonal"
    sde_type = "ito"
    score = None               # (sdeint's HIP paths: no second field)
    negate_reverse = False     # (and no sign flip on the way back)

    def __init__(self, drift, sigma=1.0, reverse=False):
        super().__init__()
        self.drift, self.sigma, self.reverse = drift, sigma, reverse
        self.last_path = None      # "hip" / "eager": what the last sdeint call on this object ran

    _cat = FlowScoreSDE._cat
    g = FlowScoreSDE.g
    h = FlowScoreSDE.h

    def f(self, t, y):
        return self.drift(self._cat(1 - t if self.reverse else t, y))


_SDE_CLASSES = (FlowScoreSDE, DriftSDE)      # what sdeint's HIP paths know how to take apart


def _grid(ts, dt):
    """The ts grid refined so that no step exceeds dt; returns [(t, h, is_output)]."""
    pts = [float(x) for x in ts]
    steps = []
    for a, b in zip(pts[:-1], pts[1:]):
        n = max(1, int(math.ceil(abs(b - a) / dt * (1.0 - 1e-6))))      # (ts usually arrives as float32: 0.05 is 0.0500000007)
        for k in range(n):
            steps.append((a + (b - a) * k / n, (b - a) / n, k == n - 1))
    return steps


def _fused_fields(sde):
    """(drift, score) as two 4-layer time-varying MLPs of widths <= 64 with identical layer sizes, or None.  A DriftSDE:
    (drift, None), the kernel's single-field mode."""
    f, s = sde.drift, sde.score
    if s is None:
        s = f
    if not (isinstance(f, MLP) and isinstance(s, MLP) and f.time_varying and s.time_varying):
        return None
    df, ds = f.dims(), s.dims()
    if len(df) != 5 or df != ds or max(df[1:]) > 64 or df[0] != df[4] + 1:
        return None
    return f, sde.score, df


_G_CACHE = {}         # (schedule type, parameters, grid) -> g(t_k): _schedule_values


def _schedule_values(sigma, steps):
    """g(t_k) of a callable ``sigma`` for every step of the refined grid, as Python floats: evaluated on the host at the
    solver's time at the start of the step, in float32.  None when a value is not a scalar (state-dependent noise)."""
    # the built-in schedules are pure functions of their numeric parameters: a loop that samples again and again on one
    # grid pays the per-step host evaluations (about 9 us each) once
    key = None
    if type(sigma) in _BUILTIN_SCHEDULES and all(isinstance(p, (int, float)) for p in vars(sigma).values()):
        key = (type(sigma), tuple(sorted(vars(sigma).items())), tuple(t for t, _, _ in steps))
        if key in _G_CACHE:
            return list(_G_CACHE[key])
    vals = []
    for t, _, _ in steps:
        v = sigma(torch.as_tensor(t, dtype=torch.float32))
        if isinstance(v, torch.Tensor) and v.numel() != 1:
            return None
        try:
            vals.append(float(v))
        except (TypeError, ValueError):
            return None
    if key is not None:
        if len(_G_CACHE) >= 16:
            _G_CACHE.pop(next(iter(_G_CACHE)))
        _G_CACHE[key] = tuple(vals)
    return vals


def _em_records(steps, g, reverse):
    """The EmStep records of cfm_sde_em_mlp_f32 (csrc/sde_small.h), 16 bytes per step: field time, step, g(t_k) sqrt|h_k|,
    output flag — with the casts of the launch-per-step path: float32 time, float32 step, float32 (g sqrt|h|)."""
    import struct
    return b"".join(struct.pack("<fffi", (1.0 - t) if reverse else t, h, gk * math.sqrt(abs(h)), 1 if is_out else 0)
                    for (t, h, is_out), gk in zip(steps, g))


def _srk_records(steps, sigma, reverse):
    """The SrkStep records of cfm_sde_srk_mlp_f32 (csrc/sde_small.h), 32 bytes per step: the field times of the three stages
    (t, t + h, t + h / 2), step, sigma sqrt|h|, 3/4 sigma sqrt|h|, output flag, padding — with the casts of the
    launch-per-step path, as ``_em_records``."""
    import struct
    recs = []
    for t, h, is_out in steps:
        gs = sigma * math.sqrt(abs(h))
        te = [(1.0 - u) if reverse else u for u in (t, t + h, t + 0.5 * h)]
        recs.append(struct.pack("<ffffffii", te[0], te[1], te[2], h, gs, 0.75 * sigma * math.sqrt(abs(h)),
                                1 if is_out else 0, 0))
    return b"".join(recs)


_LOGQP_EPS = 1e-7        # torchsde's stable_division


def _stable_division(a, b, eps=_LOGQP_EPS):
    """torchsde's ``misc.stable_division``: every ``b`` with ``|b| <= eps`` becomes ``eps * sign(b)`` (so 0 stays 0)."""
    b = torch.where(b.abs() > eps, b, torch.full_like(b, eps) * b.sign())
    return a / b


def _logqp_weights(steps, g, srk):
    """qw_k of the HIP paths under ``logqp``, as float32 values: the per-step factor of the row sum of squared drifts,
    ``h_k / (2 g_k^2)`` for ``euler`` and ``h / (12 sigma^2)`` for ``srk`` (whose sum is (k1^2 + k2^2) + 4 k3^2), formed
    in float64 and rounded once.  ``0 < |g_k| <= 1e-7`` enters as ``1e-7 sign(g_k)`` (stable_division; for qw alone);
    ``g_k == 0`` raises."""
    import struct
    qw = []
    for (t, h, _), gk in zip(steps, g):
        if gk == 0.0:
            raise ValueError(f"sdeint(logqp=True): g = 0 at t = {t}: the log-ratio integrand (f / g)^2 is infinite there "
                             "(torchsde would return inf or nan)")
        if abs(gk) <= _LOGQP_EPS:
            gk = math.copysign(_LOGQP_EPS, gk)
        qw.append(0.5 * h / ((6.0 if srk else 1.0) * gk * gk))
    return list(struct.unpack(f"<{len(qw)}f", struct.pack(f"<{len(qw)}f", *qw)))


def _packed_steps(steps, g_steps, srk, reverse, qw=None):
    """(blob, workspace bytes) of a one-launch call: the step records (``_srk_records`` / ``_em_records``), and with ``qw``
    (``_logqp_weights``) the records followed by the n_steps float32 weights, for a workspace of (record + 4) n_steps
    bytes (include/cfm_gfx950.h, the entries' flag bit 1)."""
    import struct
    if srk:
        blob = _srk_records(steps, g_steps[0] if steps else 0.0, reverse)          # (srk: sigma is constant)
    else:
        blob = _em_records(steps, g_steps, reverse)
    if qw is not None:
        blob += struct.pack(f"<{len(qw)}f", *qw)
    return blob, len(blob)


def _kernel_reverse_flag(sde):
    """The ``reverse`` bit (bit 0 of the flag word) of the one-launch kernels: it NEGATES the first field, which is
    FlowScoreSDE's way back; a DriftSDE's reverse lives in the records' te = 1 - t alone (0 in both directions)."""
    return 1 if (sde.reverse and sde.negate_reverse) else 0


_SRK_SCOPE = ("sdeint method 'srk' is built for FlowScoreSDE with a constant (non-callable) sigma: for constant diagonal "
              "noise every diffusion-derivative term of the SRI2W1 tableau vanishes; a state- or time-dependent g needs "
              "the full tableau, which is not built")


def _noise_arg(noise, method, n_steps, y0):
    """None for the named modes, else the caller's standard normals checked against the refined grid."""
    if isinstance(noise, str):
        if noise not in ("philox", "torch"):
            raise ValueError("noise must be 'philox', 'torch' or a tensor of standard normals")
        return None
    if not torch.is_tensor(noise):
        raise ValueError("noise must be 'philox', 'torch' or a tensor of standard normals")
    want = (n_steps, 2) + tuple(y0.shape) if method == "srk" else (n_steps,) + tuple(y0.shape)
    if tuple(noise.shape) != want:
        raise ValueError(f"sdeint(method={method!r}): the noise tensor must have shape {list(want)} "
                         f"([n_steps{', 2' if method == 'srk' else ''}, B, d] on the grid refined to dt), got {list(noise.shape)}")
    return noise


def _run_one_launch(sde, fields, y0, y, steps, g_steps, srk, given, noise, generator, qw=None):
    """The whole trajectory in one launch of cfm_sde_em_mlp_f32 / cfm_sde_srk_mlp_f32.  fields: ``_fused_fields(sde)``; y:
    the fp32 device copy of y0; given: the caller's normals on the device, or None for ``noise`` "torch" / "philox".
    qw (``_logqp_weights``): the call's logqp form, ``(trajectory, log-ratio increments [n_out, B])``."""
    import ctypes
    lib = _lib.load()
    dev = y.device
    f, s, dims = fields
    B, d = y.shape
    n_out = sum(1 for st in steps if st[2])
    blob, ws_bytes = _packed_steps(steps, g_steps, srk, sde.reverse, qw)
    host = (ctypes.c_char * ws_bytes).from_buffer_copy(blob)
    xi = given
    seed = 0
    if xi is None and noise == "torch":
        shape = (2, B, d) if srk else (B, d)
        xi = torch.stack([torch.randn(shape, device=dev, dtype=torch.float32, generator=generator) for _ in steps])
    elif xi is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), device=dev, generator=generator).item())
    Wf, bf, _, keep_f = f.hip_params(dev)
    Ws, bs, _, keep_s = s.hip_params(dev) if s is not None else (None, None, None, None)      # one field: Ws = bs = NULL
    cd = (ctypes.c_int * 5)(*dims)
    flags = _kernel_reverse_flag(sde)
    if qw is None:
        traj = out = torch.empty((n_out, B, d), dtype=torch.float32, device=dev)
    else:
        # one buffer: the trajectory followed by the log-ratio increments
        flags |= 2
        out = torch.empty(n_out * B * d + n_out * B, dtype=torch.float32, device=dev)
        traj, lr = out[:n_out * B * d].view(n_out, B, d), out[n_out * B * d:].view(n_out, B)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
    name = "cfm_sde_srk_mlp_f32" if srk else "cfm_sde_em_mlp_f32"
    check(getattr(lib, name)(Wf, bf, Ws, bs, cd, 4, ptr(y), B, host, len(steps), flags,
                             ptr(xi), seed, ptr(out), ptr(ws), stream_ptr()), name)
    # (no synchronisation: a host array may be dropped as soon as the call returns, include/cfm_gfx950.h)
    traj = torch.cat([y0.to(torch.float32)[None].to(y0.device), traj.to(y0.device)])
    return traj if qw is None else (traj, lr.to(y0.device))


def _run_stepped(sde, y0, y, steps, g_steps, srk, given, generator, qw=None):
    """A launch per step: the fields through ``MLP.forward_hip``, the state update in cfm_sde_em_step_f32 (``euler``) or
    one cfm_sde_srk_step_f32 per stage (``srk``).  y: the fp32 device copy of y0, updated in place; the increments are
    drawn inside the loop unless ``given``.  qw (``_logqp_weights``): the log-ratio column too, a few torch ops per step on
    the field values the step kernel gets (no kernel of its own: the runner's nets take the one-launch path)."""
    lib = _lib.load()
    dev = y.device
    out = [y0]
    sign = 1.0
    lr = torch.zeros(y.shape[0], dtype=torch.float32, device=dev) if qw is not None else None
    lrs = []
    if srk:
        sigma = g_steps[0] if steps else 0.0          # (srk: constant)

        def pair(yy, u):
            te = (1.0 - u) if sde.reverse else u
            v = sde.drift.forward_hip(yy, te)
            return (-v if sde.reverse else v), sde.score.forward_hip(yy, te)
        ys = torch.empty_like(y)
    for k, (t, h, is_out) in enumerate(steps):
        if srk:
            xi = given[k] if given is not None else torch.randn((2,) + tuple(y.shape), device=dev, dtype=torch.float32,
                                                                generator=generator)
            xi1, xi2 = xi[0], xi[1]
            v1, s1 = pair(y, t)
            v2 = s2 = v3 = s3 = None
            for stage in (1, 2, 3):
                check(lib.cfm_sde_srk_step_f32(stage, ptr(y), ptr(ys), ptr(v1), ptr(s1), ptr(v2), ptr(s2), ptr(v3),
                                               ptr(s3), ptr(xi1), ptr(xi2), float(h), sigma, sign, y.numel(),
                                               stream_ptr()), "cfm_sde_srk_step_f32")
                if stage == 1:
                    v2, s2 = pair(ys, t + h)
                elif stage == 2:
                    v3, s3 = pair(ys, t + 0.5 * h)
            if lr is not None:
                k1, k2, k3 = v1 + s1, v2 + s2, v3 + s3
                lr = lr + qw[k] * ((k1 * k1 + k2 * k2) + 4.0 * (k3 * k3)).sum(1)
        else:
            te = (1.0 - t) if sde.reverse else t
            v = sde.drift.forward_hip(y, te)
            s = sde.score.forward_hip(y, te) if sde.score is not None else None
            if sde.reverse and sde.negate_reverse:
                v = -v
            xi = given[k] if given is not None else torch.randn(y.shape, device=dev, dtype=torch.float32, generator=generator)
            if lr is not None:
                f = v + s if s is not None else v
                lr = lr + qw[k] * (f * f).sum(1)
            check(lib.cfm_sde_em_step_f32(ptr(y), ptr(v), ptr(s), ptr(xi), float(h), g_steps[k], sign,
                                          y.numel(), stream_ptr()), "cfm_sde_em_step_f32")
        if is_out:
            out.append(y.clone().to(y0.device))
            if lr is not None:
                lrs.append(lr.to(y0.device))
                lr = torch.zeros_like(lr)
    traj = torch.stack([o.to(torch.float32) for o in out])
    if qw is None:
        return traj
    return traj, (torch.stack(lrs) if lrs else torch.zeros((0, y.shape[0]), dtype=torch.float32, device=y0.device))


def _run_eager(sde, y0, steps, srk, given, generator, logqp=False):
    """The same schemes in eager torch ops on ``sde.f`` / ``sde.g``, in the caller's dtype and on its device.  logqp: also
    the log-ratio column lr' = 1/2 sum_j u_j^2, u = stable_division(f - h, g), as one more drift-only component of the
    scheme (``sde.h(t, y)`` when the object has one, else 0), returned as its increase over every interval of ``ts``."""
    out = [y0]
    y = y0
    if given is not None:
        given = given.to(device=y.device, dtype=y.dtype)
    prior = getattr(sde, "h", None)

    def q(tt, yy, f, g):
        u = _stable_division(f - prior(tt, yy) if prior is not None else f, g)
        return 0.5 * (u * u).flatten(1).sum(1)
    lr = torch.zeros(y.shape[0], dtype=y.dtype, device=y.device) if logqp else None
    lrs = []
    for k, (t, h, is_out) in enumerate(steps):
        tt = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        if srk:
            # the scheme of csrc/sde_srk.h in the caller's dtype
            xi = given[k] if given is not None else torch.randn((2,) + tuple(y.shape), device=y.device, dtype=y.dtype,
                                                                generator=generator)
            gs = float(sde.sigma) * math.sqrt(abs(h))
            k1 = sde.f(tt, y)
            y2 = y + h * k1
            k2 = sde.f(tt + h, y2)
            y3 = y + (0.25 * h) * (k1 + k2) + (0.75 * gs) * (xi[0] + xi[1] / math.sqrt(3.0))
            k3 = sde.f(tt + 0.5 * h, y3)
            if logqp:
                g = torch.full_like(y, float(sde.sigma))
                lr = lr + (h / 6.0) * ((q(tt, y, k1, g) + q(tt + h, y2, k2, g)) + 4.0 * q(tt + 0.5 * h, y3, k3, g))
            y = y + (h / 6.0) * ((k1 + k2) + 4.0 * k3) + gs * xi[0]
        else:
            xi = given[k] if given is not None else torch.randn(y.shape, device=y.device, dtype=y.dtype, generator=generator)
            f, g = sde.f(tt, y), sde.g(tt, y)
            if logqp:
                lr = lr + h * q(tt, y, f, g)
            y = y + h * f + g * math.sqrt(abs(h)) * xi
        if is_out:
            out.append(y)
            if logqp:
                lrs.append(lr)
                lr = torch.zeros_like(lr)
    if not logqp:
        return torch.stack(out)
    return torch.stack(out), (torch.stack(lrs) if lrs else y.new_zeros((0, y.shape[0])))


@torch.no_grad()
def sdeint(sde, y0, ts, method="euler", dt=1e-3, generator=None, noise="philox", fused=None, logqp=False, **unused):
    """Trajectory [len(ts), B, d] of ``sde`` (an object with f(t, y), g(t, y)) from y0 on the ``ts`` grid refined to
    steps of at most ``dt``.  ``method="euler"`` (default): Euler-Maruyama.  ``method="srk"``: torchsde's default
    scheme for diagonal Ito noise (SRI2W1, strong order 1.5), built for ``FlowScoreSDE`` with a constant ``sigma`` and
    strictly increasing ``ts`` (backward integration is ``reverse=True``); three drift evaluations per step.

    Two small ``cfm_amd.MLP`` fields (4 layers, widths <= 64: the SF2M tutorial's and the single-cell models) run the
    WHOLE trajectory in one launch (``cfm_sde_em_mlp_f32`` / ``cfm_sde_srk_mlp_f32``: weights of both fields in LDS,
    state in registers).  A ``DriftSDE`` (one drift net: DSBM's forward or backward SDE) takes the same ``euler`` paths
    with one field, the one-launch kernel in its single-field mode.
    ``noise="philox"`` (default): N(0, 1) from Philox4x32-10 inside the kernel, seeded from ``generator`` (or torch's
    default CUDA generator), so ``torch.manual_seed`` makes runs repeatable; ``noise="torch"``: the increments are
    drawn with ``torch.randn`` step by step exactly as the launch-per-step scheme draws them (``(B, d)`` per step for
    ``euler``, ``(2, B, d)`` = (xi1, xi2) for ``srk``) — same trajectory, bit for bit, as that scheme; a tensor: the
    caller's standard normals, ``[n_steps, B, d]`` for ``euler`` and ``[n_steps, 2, B, d]`` for ``srk`` with
    ``n_steps`` the length of the refined grid.  ``fused=False`` forces the launch-per-step scheme (measurement /
    test switch).  A callable ``sde.sigma`` with a scalar value (a noise schedule) runs on the same ``euler`` kernels,
    evaluated per refined step at the solver's time t_k (module docstring); a non-scalar value keeps the eager scheme.

    ``logqp=True`` (torchsde's keyword): returns ``(ys, log_ratio_increments)``, the second ``[len(ts) - 1, B]``: the
    increase over each interval of ``ts`` (not cumulative) of the column with drift ``0.5 * (u ** 2).sum(1)``,
    ``u = stable_division(f - h, g)``, zero diffusion and zero start, integrated by the scheme that runs the state
    (module docstring).  The trajectory is the one ``logqp=False`` gives on the same noise, bit for bit, on every path:
    the one-launch kernels reduce the drift tile they hold (``h = 0``), the launch-per-step path adds a few torch ops
    per step, the eager path evaluates ``sde.h`` when the object has one.  On the HIP paths a step with ``g == 0``
    raises ``ValueError`` before any launch."""
    if method not in ("euler", "srk"):
        raise NotImplementedError(f"sdeint method {method!r}: 'euler' (Euler-Maruyama) and 'srk' (SRI2W1) are built")
    srk = method == "srk"
    if srk:
        if not isinstance(sde, FlowScoreSDE) or callable(sde.sigma):
            raise NotImplementedError(_SRK_SCOPE)
        pts = [float(x) for x in ts]
        if any(b <= a for a, b in zip(pts[:-1], pts[1:])):
            raise ValueError("sdeint(method='srk'): ts must be strictly increasing (integrate backwards with "
                             "FlowScoreSDE(..., reverse=True))")
    steps = _grid(ts, float(dt))
    given = _noise_arg(noise, method, len(steps), y0)
    known = isinstance(sde, _SDE_CLASSES)
    fast = (known and isinstance(sde.drift, MLP) and (sde.score is None or isinstance(sde.score, MLP))
            and y0.dim() == 2 and torch.cuda.is_available())
    g_steps = None
    if known and callable(sde.sigma) and (fast or fused is True):
        # a schedule: one scalar per step (srk with a callable sigma was refused above)
        g_steps = _schedule_values(sde.sigma, steps)
        if g_steps is None:
            if fused is True:
                raise ValueError("sdeint(fused=True): sigma(t) must be a scalar (a noise schedule); state-dependent noise "
                                 "is stepped in eager torch")
            fast = False
    qw = None
    if fast and logqp:
        # (before any launch and before last_path: g = 0 raises here)
        qw = _logqp_weights(steps, g_steps if g_steps is not None else [float(sde.sigma)] * len(steps), srk)
    if known:
        sde.last_path = "hip" if fast else "eager"
    if not fast:
        return _run_eager(sde, y0, steps, srk, given, generator, logqp)
    _lib.load()
    dev = _lib.require_gpu()
    y = _lib.to_dev_f32(y0, dev).clone()
    if given is not None:
        given = _lib.to_dev_f32(given, dev).contiguous()
    fields = _fused_fields(sde) if (y.shape[1] <= 64 and fused is not False) else None
    if fields is not None and y.shape[1] != fields[2][4]:
        # the one-launch kernel reads y0 with the fields' output width as its pitch: a state of another width
        # must not reach it (the stepping path raises the layer's shape error instead)
        if fused is True:
            raise ValueError(f"sdeint(fused=True): y0 has {y.shape[1]} columns, the fields map {fields[2][4]}")
        fields = None
    if fused is True and fields is None:
        raise ValueError("sdeint(fused=True): needs two 4-layer time-varying cfm_amd.MLP fields of widths <= 64 "
                         "(FlowScoreSDE; one for a DriftSDE)")
    if g_steps is None:
        g_steps = [float(sde.sigma)] * len(steps)
    if fields is not None:
        return _run_one_launch(sde, fields, y0, y, steps, g_steps, srk, given, noise, generator, qw)
    return _run_stepped(sde, y0, y, steps, g_steps, srk, given, generator, qw)


def _mlp_pair(first, second):
    """(MLP, MLP) when both fields are, or wrap, time-varying MLPs that the HIP paths take (``models.time_mlp``), else None."""
    pair = (time_mlp(first, bare=True), time_mlp(second, bare=True))
    return None if None in pair else pair


def _refuse_srk(who):
    raise NotImplementedError(f"{who}(sde_solver='srk'): sigma is a schedule sigma(t) here, and 'srk' is built "
                              "for constant diagonal noise only (the full SRI2W1 tableau is not built)")


def _refuse_adaptive(adaptive):
    if adaptive:
        raise NotImplementedError("sdeint(adaptive=True): the samplers here step the refined t_span grid with fixed steps "
                                  "(Euler-Maruyama, srk); torchsde's adaptive step-size control with its Brownian-interval "
                                  "queries is not built")


class _SolverSDE:
    """The eager SDE of a FlowSolver for ``sdeint``: f(t, y) from the solver's drift methods (so ``nfe`` counts), g from
    its schedule."""

    def __init__(self, solver, reverse):
        self.solver, self.reverse = solver, reverse

    def f(self, t, y):
        return self.solver.backward_sde_drift(1 - t, y) if self.reverse else self.solver.forward_sde_drift(t, y)

    def g(self, t, y):
        return self.solver.sigma(t) * torch.ones_like(y)

    def h(self, t, y):
        return torch.zeros_like(y)


class FlowSolver(torch.nn.Module):
    """Subset of runner/src/models/components/solver.py:44-230 on this backend: a flow field and an
    optional score field (separate networks, or one network whose output is [flow, score]) behind
    ``odeint`` (NeuralODE) and ``sdeint`` (Euler-Maruyama; ``srk`` needs a constant sigma: ``sde.sdeint``).  vector_field / score_field are called as
    f(t, x) like torchdyn vector fields.  ``sdeint`` with ``sde_solver="euler"`` and two separate fields that unwrap to
    time-varying ``cfm_amd.MLP``s (a ``torch_wrapper`` around one, or a bare one) runs ``sde.sdeint``'s HIP paths with the
    schedule ``sigma``; ``last_path`` says ``"hip"`` or ``"eager"`` after a call."""

    def __init__(self, vector_field, dim, score_field=None, sigma=None, ode_solver="euler", sde_solver="euler",
                 dt=0.01, atol=1e-5, rtol=1e-5, augmentations=None, **kwargs):
        super().__init__()
        self.net, self.dim, self.score_net = vector_field, dim, score_field
        self.separate_score = score_field is not None
        self.sigma, self.ode_solver, self.sde_solver = sigma, ode_solver, sde_solver
        self.dt, self.atol, self.rtol, self.nfe = dt, atol, rtol, 0
        self.augmentations = augmentations          # a cnf.AugmentationModule or None; may be assigned later (solver.py:201)
        self.last_path = None

    def forward_flow_and_score(self, t, x, only_flow=False):       # solver.py:103-121
        if self.separate_score:
            vt, st = self.net(t, x), self.score_net(t, x)
        else:
            vtst = self.net(t, x)
            if vtst.shape[1] == x.shape[1]:
                return vtst
            k = vtst.shape[1] // 2
            vt, st = vtst[:, :k], vtst[:, k:]
        return vt if only_flow else (vt, st)

    def forward_sde_drift(self, t, x):                              # solver.py:123-127
        self.nfe += 1
        vt, st = self.forward_flow_and_score(t, x)
        return vt + st

    def backward_sde_drift(self, t, x):                             # solver.py:129-133
        self.nfe += 1
        vt, st = self.forward_flow_and_score(t, x)
        return -vt + st

    def forward_ode_drift(self, t, x):                              # solver.py:135-138
        self.nfe += 1
        return self.forward_flow_and_score(t, x, only_flow=True)

    def odeint(self, x0, t_span):
        """The ODE trajectory [n_t, B, d]; with ``augmentations`` set, ``(traj, aug [n_t, B, aug_dims])`` as solver.py:201-216:
        the path integrals of the ``AugmentationModule`` from zero initial columns.  ``ode_solver="euler"`` on an fp32 CUDA
        state of a small-envelope time-varying ``cfm_amd.MLP`` flow net runs one launch of ``cfm_ode_euler_cnf_reg_mlp_f32``
        (``last_path == "hip"``, ``nfe == n_t - 1``); everything else steps the augmented field in torch ops
        (``"eager"``)."""
        from .ode import NeuralODE
        self.nfe = 0
        if self.augmentations is None:
            node = NeuralODE(self.forward_ode_drift, solver=self.ode_solver, atol=self.atol, rtol=self.rtol,
                             return_t_eval=False)
            return node(x0, t_span)
        return self._odeint_augmented(x0, t_span, self._hip_flow(x0))

    def _hip_flow(self, x0):
        """The flow MLP when the augmented Euler kernel takes ``forward_ode_drift`` on x0 (cnf._small_envelope), else None."""
        from .cnf import _small_envelope
        m = time_mlp(self.net, bare=True)
        if (m is None or self.ode_solver != "euler" or x0.dim() != 2 or not x0.is_cuda or x0.dtype != torch.float32
                or not _small_envelope(m, x0.shape[1])):
            return None
        ok = all(p.dtype == torch.float32 and p.device == x0.device for p in m.parameters())
        return m if ok else None

    def _odeint_augmented(self, x0, t_span, m):
        """``(traj, aug)`` under ``self.augmentations``: one HIP launch on the MLP ``m`` where there is one and the entry
        takes the call, else the augmented field ``[augs, dx]`` stepped by ``NeuralODE``'s generic path."""
        from .cnf import TRACE_EXACT, TRACE_NONE, augmented_euler_hip
        from .ode import NeuralODE, _check_t_span
        am = self.augmentations
        a = am.aug_dims
        if a == 0:
            node = NeuralODE(self.forward_ode_drift, solver=self.ode_solver, atol=self.atol, rtol=self.rtol,
                             return_t_eval=False)
            traj = node(x0, t_span)
            return traj, traj.new_zeros((*traj.shape[:2], 0))
        if m is not None and am.reg_mask:
            _check_t_span(torch.as_tensor(t_span, dtype=torch.float32).cpu())
            with torch.no_grad():
                got = augmented_euler_hip(m, x0, t_span, TRACE_EXACT if am.cnf_estimator == "exact" else TRACE_NONE, am.reg_mask)
            if got is not None:
                self.last_path, self.nfe = "hip", got[1]
                return got[0][:, :, a:], got[0][:, :, :a]
        self.last_path = "eager"

        def field(t, state):
            augs, dx = am.integrands(self.forward_ode_drift, t, state[:, a:])
            return torch.cat([augs, dx], 1)
        node = NeuralODE(field, solver=self.ode_solver, atol=self.atol, rtol=self.rtol, return_t_eval=False)
        x = x0.reshape(x0.shape[0], -1)
        sol = node(torch.cat([x.new_zeros((x.shape[0], a)), x], 1), t_span)
        return sol[:, :, a:], sol[:, :, :a]

    def _hip_fields(self):
        """(flow MLP, score MLP) when sdeint's HIP paths can take the pair (the rule of NeuralODE._hip_mlp), else None."""
        if self.sde_solver != "euler" or not self.separate_score or self.sigma is None:
            return None
        return _mlp_pair(self.net, self.score_net)

    def sdeint(self, x0, t_span, reverse=False, generator=None, *, logqp=False, adaptive=False):
        """solver.py:157-182.  ``logqp=True``: ``(traj, kldiv)`` as ``sde.sdeint`` returns them, ``kldiv [n_t - 1, B]`` per
        interval of ``t_span`` (cfm_module.py:911-983 logs ``mean(kldiv[-1])``).  ``adaptive=True`` is not built."""
        _refuse_adaptive(adaptive)
        if self.sde_solver == "srk":
            _refuse_srk("FlowSolver")
        self.nfe = 0
        fields = self._hip_fields()
        if fields is not None:
            sde = FlowScoreSDE(fields[0], fields[1], sigma=self.sigma, reverse=reverse)
            out = sdeint(sde, x0, t_span, method="euler", dt=self.dt, generator=generator, logqp=logqp)
            self.last_path = sde.last_path
            self.nfe = len(_grid(t_span, float(self.dt)))          # one evaluation of the field pair per refined step
            return out
        self.last_path = "eager"
        return sdeint(_SolverSDE(self, reverse), x0, t_span, method=self.sde_solver, dt=self.dt, generator=generator,
                      logqp=logqp)


class DSBMFlowSolver(FlowSolver):
    """runner/src/models/components/solver.py:225-269 on this backend: ``vector_field`` is the FORWARD SDE drift net and
    ``score_field`` the BACKWARD one (two separate nets, called as f(t, x); the single-net split output is not built).
    ``sigma``: a noise schedule (``cfm_amd.schedule``) or a number for a constant one.

    ``sdeint``: forward ``dy = f(t, y) dt + g(t) dW``; ``reverse=True`` has drift ``+b(1 - t, y)`` with g read at the
    solver's time (solver.py:249-257, :35-41).  Time-varying ``cfm_amd.MLP`` nets run ``sde.sdeint``'s HIP paths on a
    ``DriftSDE``: 4 layers of widths <= 64 the one-launch kernel in its single-field mode (``cfm_sde_em_mlp_f32`` with
    ``Ws = NULL``), wider ones a launch per step; anything else the eager scheme.  ``sde_solver="srk"`` is refused.

    ``odeint``: ``dx/dt = (f(t, x) - b(t, x)) / 2`` (solver.py:259-263).  MLP pairs of equal sizes under ``euler``,
    ``midpoint`` or ``rk4`` run ``cfm_ode_fixed_pair_mlp_f32`` (one launch for 4 layers of widths <= 64;
    ``fused=False`` forces its launch-per-stage form: two forward passes, the halved difference, the stage combine —
    the same bits); ``dopri5`` / ``tsit5`` and every other field run ``NeuralODE``'s generic path on the combined
    callable.  ``nfe`` counts one evaluation of the pair per stage.  ``last_path``: ``"hip"`` or ``"eager"``.  With
    ``augmentations`` set, ``odeint`` returns ``(traj, aug)`` from the generic path alone (the pair kernel has no augmented
    form)."""

    def __init__(self, vector_field, dim, score_field=None, sigma=None, ode_solver="euler", sde_solver="euler", dt=0.01,
                 **kwargs):
        if score_field is None:
            raise TypeError("DSBMFlowSolver needs the backward drift net as score_field (one net with a split "
                            "[forward, backward] output is not built)")
        if isinstance(sigma, (int, float)) and not isinstance(sigma, bool):
            sigma = ConstantNoiseScheduler(sigma)
        super().__init__(vector_field, dim, score_field=score_field, sigma=sigma, ode_solver=ode_solver,
                         sde_solver=sde_solver, dt=dt, **kwargs)

    def forward_sde_drift(self, t, x):                              # solver.py:249-252
        self.nfe += 1
        return self.net(t, x)

    def backward_sde_drift(self, t, x):                             # solver.py:254-257
        self.nfe += 1
        return self.score_net(t, x)

    def forward_ode_drift(self, t, x):                              # solver.py:259-263
        self.nfe += 1
        return (self.net(t, x) - self.score_net(t, x)) / 2

    def _hip_pair(self):
        """(forward MLP, backward MLP) when the HIP paths can take them (the rule of NeuralODE._hip_mlp), else None."""
        return _mlp_pair(self.net, self.score_net)

    def sdeint(self, x0, t_span, reverse=False, generator=None, noise="philox", fused=None, *, logqp=False, adaptive=False):
        _refuse_adaptive(adaptive)
        if self.sde_solver == "srk":
            _refuse_srk("DSBMFlowSolver")
        if self.sigma is None:
            raise ValueError("DSBMFlowSolver.sdeint needs sigma (a noise schedule or a number)")
        self.nfe = 0
        pair = self._hip_pair()
        if pair is not None:
            sde = DriftSDE(pair[1] if reverse else pair[0], sigma=self.sigma, reverse=reverse)
            out = sdeint(sde, x0, t_span, method="euler", dt=self.dt, generator=generator, noise=noise, fused=fused,
                         logqp=logqp)
            self.last_path = sde.last_path
            self.nfe = len(_grid(t_span, float(self.dt)))          # one drift evaluation per refined step
            return out
        self.last_path = "eager"
        return sdeint(_SolverSDE(self, reverse), x0, t_span, method="euler", dt=self.dt, generator=generator, noise=noise,
                      logqp=logqp)

    @torch.no_grad()
    def odeint(self, x0, t_span, fused=None):
        from .ode import NeuralODE, _check_t_span
        self.nfe = 0
        if self.augmentations is not None:      # the pair kernel has no augmented form: the combined callable, stepped in torch ops
            return self._odeint_augmented(x0, t_span, None)
        pair = self._hip_pair()
        if (pair is not None and self.ode_solver in _lib.ODE_SCHEME and x0.dim() == 2 and x0.dtype == torch.float32
                and torch.cuda.is_available()):
            dims = [m.dims() for m in pair]
            if dims[0] == dims[1] and x0.shape[1] == dims[0][-1]:
                _check_t_span(torch.as_tensor(t_span, dtype=torch.float32).cpu())
                self.last_path = "hip"
                return self._odeint_hip(pair, x0, t_span, fused)
        self.last_path = "eager"
        node = NeuralODE(self.forward_ode_drift, solver=self.ode_solver, atol=self.atol, rtol=self.rtol, return_t_eval=False)
        return node(x0, t_span)

    def _odeint_hip(self, pair, x0, t_span, fused):
        from .ode import _solve_hip
        rc, what, traj, nfe, _, ts = _solve_hip("pair_mlp", pair[0], x0, t_span, self.ode_solver, second=pair[1], fused=fused)
        check(rc, what)          # (`ts` may go when the call has returned: include/cfm_gfx950.h, host arrays)
        self.nfe = nfe
        return traj.to(x0.device)

    @torch.no_grad()
    def resample_pairs(self, x0, x1, generator=None, noise="philox"):
        """The outer-loop refresh of DSBM / iterative Markovian fitting (runner/src/models/cfm_module.py:1018-1033): the
        forward SDE from ``x0[:B // 2]`` and the reverse SDE from ``x1[B // 2:]`` over ``t_span = (0, 1)``, the latter
        flipped in time; returns ``[B, 2, *dim]`` with ``[:, 0]`` the time-0 end and ``[:, 1]`` the time-1 end of every
        pair.  ``noise``: as ``sdeint``; a tensor ``[n_steps, B, *dim]`` is split by rows between the two solves.  A pure
        composition of ``sdeint``."""
        half = x0.shape[0] // 2
        t_span = torch.linspace(0, 1, 2)
        nf, nb = (noise[:, :half], noise[:, half:]) if torch.is_tensor(noise) else (noise, noise)
        forward_traj = self.sdeint(x0[:half], t_span, generator=generator, noise=nf)
        backward_traj = torch.flip(self.sdeint(x1[half:], t_span, reverse=True, generator=generator, noise=nb), (0,))
        return torch.cat([forward_traj, backward_traj], dim=1).transpose(0, 1)
