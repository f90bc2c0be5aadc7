"""The action-matching objective (Neklyudov et al. 2022) with a gradient: training of ``GradModel`` fields.

Counterpart of ``ActionMatchingLitModule.step`` (runner/src/models/cfm_module.py:670-694).  For a scalar action net
``s([x, t])`` the loss is, per row,

    l = s(x0, 0) - s(x1, 1) + 1/2 |grad_x s(xt, t)|^2 + d/dt s(xt, t),        loss = mean l.

It contains a gradient already, so its parameter gradient is a double backward.  For an
``MLP(dim, out_dim=1, time_varying=True)`` of the small-kernel envelope (``models.hip_action``) on fp32 CUDA inputs,
the loss and all eight parameter gradients come from ONE call of ``cfm_action_matching_grad_f32`` (csrc/action_grad.h,
DESIGN.md 4.11): the forward of an ``autograd.Function`` makes it and keeps the gradients, the backward scales them by
the upstream scalar.  Everything else (CPU, float64, wider or deeper nets, other modules, the fused small-field path
switched off) is the reference's formulation in differentiable torch ops through the module graph.
``action_matching_loss.last_path`` says which of the two ran (``"hip"`` / ``"generic"``); nothing is printed.
"""
import ctypes

import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .models import MLP, GradModel, hip_action
from .ode import _Declined


class _ActionMatchingFunction(torch.autograd.Function):
    """loss of one cfm_action_matching_grad_f32 call; backward: the gradients that call left, times the upstream scalar.
    The eight gradients share one buffer, so that scaling them is one multiplication.  xt None: the kernel interpolates."""

    @staticmethod
    def forward(ctx, x0, x1, xt, t, dims, *params):
        lib = _lib.load()
        dev = x0.device
        ps = [p if p.is_contiguous() else p.contiguous() for p in params]
        x0d, x1d, td, xtd = (v if v is None or v.is_contiguous() else v.contiguous() for v in (x0, x1, t, xt))
        B = x0d.shape[0]
        sizes = [p.numel() for p in ps]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        base, offs = flat.data_ptr(), [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        Wp = (ctypes.c_void_p * 4)(*[p.data_ptr() for p in ps[0::2]])
        bp = (ctypes.c_void_p * 4)(*[p.data_ptr() for p in ps[1::2]])
        dWp = (ctypes.c_void_p * 4)(*[base + 4 * o for o in offs[0:8:2]])
        dbp = (ctypes.c_void_p * 4)(*[base + 4 * o for o in offs[1:8:2]])
        cdims = (ctypes.c_int * 5)(*dims)
        ws = _lib.workspace(_lib.OP_ACTION_GRAD, B, 0, 0, dev)
        rc = lib.cfm_action_matching_grad_f32(Wp, bp, cdims, 4, ptr(x0d), ptr(x1d), ptr(xtd), ptr(td), B, ptr(loss), dWp,
                                              dbp, ptr(ws), stream_ptr())
        if rc == -1:
            raise _Declined()
        _lib.check(rc, "cfm_action_matching_grad_f32")
        ctx.flat, ctx.sizes, ctx.shapes = flat, sizes, [p.shape for p in ps]
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        parts = (ctx.flat * g).split(ctx.sizes)
        return (None, None, None, None, None, *[q.view(sh) for q, sh in zip(parts, ctx.shapes)])


def _generic(net, x0, x1, t, xt):
    """The reference's lines in differentiable torch ops, with the parameters cast to the inputs' dtype and device."""
    params = {k: p.to(device=x0.device, dtype=x0.dtype) for k, p in net.named_parameters()}
    buffers = {k: b.to(device=x0.device) for k, b in net.named_buffers()}

    def energy(inp):
        return torch.func.functional_call(net, (params, buffers), (inp,))

    outer = torch.is_grad_enabled()
    with torch.enable_grad():
        xg = xt.detach().requires_grad_(True)
        tg = t.detach().requires_grad_(True)
        st = torch.sum(energy(torch.cat([xg, tg], dim=-1)))
        dsdx, dsdt = torch.autograd.grad(st, (xg, tg), create_graph=outer)
    a0 = energy(torch.cat([x0, torch.zeros_like(x0[:, :1])], dim=-1))
    a1 = energy(torch.cat([x1, torch.ones_like(x1[:, :1])], dim=-1))
    loss = a0 - a1 + 0.5 * (dsdx ** 2).sum(1, keepdim=True) + dsdt
    return loss.mean()


def action_matching_loss(action, x0, x1, t, xt=None):
    """The action-matching loss of ``action`` (a scalar ``MLP(dim, out_dim=1, time_varying=True)``, a ``GradModel``
    around one, or any module mapping [B, d + 1] to [B, 1]) on the pairs (x0, x1) [B, d] at the times t ([B] or [B, 1]).

    ``xt`` defaults to the reference's interpolant ``t * x1 + (1 - t) * x0``; a caller whose net sees an offset time (the
    reference's ``t_select``) passes the ``xt`` it interpolated with the plain time, and as ``t`` the time column the
    net is to see.  Returns a scalar tensor for ``loss.backward()``: the parameters receive gradients, the inputs do
    not (in the reference they carry no graph).  The HIP path is once differentiable.
    """
    a = action.action if isinstance(action, GradModel) else action
    if x0.dim() != 2 or x1.shape != x0.shape:
        raise ValueError(f"x0 and x1 are [B, d] of one shape; got {tuple(x0.shape)} and {tuple(x1.shape)}")
    B, d = x0.shape
    t = torch.as_tensor(t, dtype=x0.dtype, device=x0.device)
    if t.numel() != B:
        raise ValueError(f"t holds one time per row: {B}; got shape {tuple(t.shape)}")
    t = t.reshape(B, 1)
    if xt is not None and xt.shape != x0.shape:
        raise ValueError(f"xt has shape {tuple(xt.shape)}; x0 has {tuple(x0.shape)}")
    m = hip_action(a, d) if B >= 1 and x0.is_cuda else None
    if m is not None:
        lins = m._linears()
        params = [p for l in lins for p in (l.weight, l.bias)]
        given = (x0, x1, t) if xt is None else (x0, x1, t, xt)
        if (all(v.dtype == torch.float32 and v.device == x0.device for v in given)
                and all(p.device == x0.device for p in params)):
            try:
                loss = _ActionMatchingFunction.apply(x0, x1, xt, t, m.dims(), *params)
                action_matching_loss.last_path = "hip"
                return loss
            except _Declined:
                pass
    action_matching_loss.last_path = "generic"
    if xt is None:
        xt = t * x1 + (1 - t) * x0
    return _generic(a.net if isinstance(a, MLP) else a, x0, x1, t, xt)


action_matching_loss.last_path = None
