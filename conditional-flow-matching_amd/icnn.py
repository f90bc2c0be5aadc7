"""Input-convex networks for optimal transport (Makkuva et al. 2020): the runner's ICNN baseline.

Counterpart of ``runner/src/models/components/icnn_model.py`` (the net) and of ``ICNNLitModule`` with ``compute_w2``
(``runner/src/models/icnn_module.py:98-135, 229-245``: the two losses of the minimax objective and the W2 estimate).

The net has a convex-in-x structure: a z-path of bias-free linears between Softplus activations, and a skip connection
from x into every layer,

    a_1 = Wz_0 x + bz_0,   h_l = softplus(a_l),   a_{l+1} = Wz_l h_l + Wx_{l-1} x + bx_{l-1},   out = Wz_L h_L + Wx_{L-1} x.

Its transport map is the input gradient of that scalar, and the g-objective contains such a gradient already, so its
parameter gradient is a double backward: three ``autograd.grad(create_graph=True)`` graphs per step in the reference.
For two nets of one shape in the envelope of ``cfm_icnn_f32`` (2 <= L <= 4, dimh <= 64, d <= ``HIP_MAX_DIM``) on fp32 CUDA
inputs, each of the four operations is one call of that entry (csrc/icnn.hip): one launch for the
transport map, three for the W2 means and the f-step, four for the g-step, whatever B and d.  Everything else (CPU,
float64, other shapes, the fused small-field path switched off) is the reference's formulation in differentiable torch
ops.  Every function carries ``last_path`` (``"hip"`` / ``"generic"``); nothing is printed.
"""
import ctypes

import torch
from torch import nn

from . import _lib
from ._lib import stream_ptr
from .ode import _Declined

HIP_MAX_DIM = _lib.ICNN_MAX_DIM      # CFM_ICNN_MAX_DIM of include/cfm_gfx950.h


class ICNN(nn.Module):
    """``ICNN(dim, dimh, num_hidden_layers)`` with the reference's parameter names: ``Wzs`` (L + 1 linears: [dimh, dim] with
    bias, L - 1 of [dimh, dimh] and one [1, dimh] without) and ``Wxs`` (L linears: L - 1 of [dimh, dim] with bias and one
    [1, dim] without), so that a reference ``state_dict()`` loads with ``strict=True``."""

    def __init__(self, dim=2, dimh=64, num_hidden_layers=4):
        super().__init__()
        L = num_hidden_layers
        self.Wzs = nn.ModuleList([nn.Linear(dim, dimh)] + [nn.Linear(dimh, dimh, bias=False) for _ in range(L - 1)]
                                 + [nn.Linear(dimh, 1, bias=False)])
        self.Wxs = nn.ModuleList([nn.Linear(dim, dimh) for _ in range(L - 1)] + [nn.Linear(dim, 1, bias=False)])
        self.act = nn.Softplus()
        self.dim, self.dimh, self.num_hidden_layers = dim, dimh, L

    def forward(self, x):
        """[B, dim] -> [B, 1] in differentiable torch ops (the generic path: CPU, float64 and double backward work)."""
        L = self.num_hidden_layers
        h = self.act(self.Wzs[0](x))
        for l in range(1, L):
            h = self.act(self.Wzs[l](h) + self.Wxs[l - 1](x))
        return self.Wzs[L](h) + self.Wxs[L - 1](x)

    def transport(self, x):
        """grad_x of the net's output at the rows of x [B, dim]: the transport map.  Values only (no graph)."""
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"x is [B, {self.dim}]; got {tuple(x.shape)}")
        if _hip_ok((self,), (x,)):
            try:
                p = torch.empty_like(x, memory_format=torch.contiguous_format)
                _call(_lib.ICNN_TRANSPORT, self, None, x, None, 0.0, p)
                ICNN.transport.last_path = "hip"
                return p
            except _Declined:
                pass
        ICNN.transport.last_path = "generic"
        return _grad_map(self, _cast(self, x), x, False).detach()


ICNN.transport.last_path = None


def _hip_ok(nets, inputs):
    """nets of one shape inside the envelope, fp32 CUDA inputs of one device with at least a row, parameters with them"""
    n0, x0 = nets[0], inputs[0]
    if not all(isinstance(n, ICNN) for n in nets) or not x0.is_cuda or x0.shape[0] < 1:
        return False
    if any((n.dim, n.dimh, n.num_hidden_layers) != (n0.dim, n0.dimh, n0.num_hidden_layers) for n in nets):
        return False
    if not (2 <= n0.num_hidden_layers <= 4 and 1 <= n0.dimh <= 64 and 1 <= n0.dim <= HIP_MAX_DIM):
        return False
    if any(v.dtype != torch.float32 or v.device != x0.device or v.dim() != 2 or v.shape[1] != n0.dim for v in inputs):
        return False
    return all(p.dtype == torch.float32 and p.device == x0.device for n in nets for p in n.parameters())


def _fill(desc, net, keep, grads=None):
    """the weight tables of one net into its half of the descriptor, and (grads: a flat buffer in parameters() order)
    the gradient tables.  keep collects what the raw addresses point into."""
    L = net.num_hidden_layers

    def dev(t):
        t = t.detach()
        t = t if t.is_contiguous() else t.contiguous()
        keep.append(t)
        return t.data_ptr()

    for l in range(L + 1):
        desc.Wz[l] = dev(net.Wzs[l].weight)
    desc.bz0 = dev(net.Wzs[0].bias)
    for l in range(L):
        desc.Wx[l] = dev(net.Wxs[l].weight)
    for l in range(L - 1):
        desc.bx[l] = dev(net.Wxs[l].bias)
    if grads is not None:
        at = {}
        off = 0
        for name, p in net.named_parameters():
            at[name] = grads.data_ptr() + 4 * off
            off += p.numel()
        for l in range(L + 1):
            desc.dWz[l] = at[f"Wzs.{l}.weight"]
        desc.dbz0 = at["Wzs.0.bias"]
        for l in range(L):
            desc.dWx[l] = at[f"Wxs.{l}.weight"]
        for l in range(L - 1):
            desc.dbx[l] = at[f"Wxs.{l}.bias"]


def _call(op, f, g, x, y, reg, p, w=None, losses=None, grads=None):
    """One cfm_icnn_f32 call on the current stream; _Declined when the entry refuses (the fused path switched off)."""
    lib = _lib.load()
    keep = []
    c = _lib.IcnnCall()
    c.size = ctypes.sizeof(_lib.IcnnCall)
    c.op, c.d, c.dimh, c.L, c.reg = op, f.dim, f.dimh, f.num_hidden_layers, float(reg)
    data = x if x is not None else y
    c.B = data.shape[0]
    for v in (x, y, p, w):                      # the kernels index every one of them as [B, d]
        if v is not None and tuple(v.shape) != (c.B, c.d):
            raise ValueError(f"cfm_icnn_f32 takes [B, d] = [{c.B}, {c.d}] buffers; got {tuple(v.shape)}")
    _fill(c.f, f, keep, grads if op == _lib.ICNN_F_STEP else None)
    if g is not None:
        _fill(c.g, g, keep, grads if op == _lib.ICNN_G_STEP else None)
    for name, v in (("x", x), ("y", y)):
        if v is not None:
            v = v.detach()
            v = v if v.is_contiguous() else v.contiguous()
            keep.append(v)
            setattr(c, name, v.data_ptr())
    c.p = p.data_ptr()
    if w is not None:
        c.w = w.data_ptr()
    if losses is not None:
        c.losses = losses.data_ptr()
    if op != _lib.ICNN_TRANSPORT:
        ws = _lib.workspace(_lib.OP_ICNN, c.B, 0, 0, data.device)
        c.ws = ws.data_ptr()
    c.stream = stream_ptr().value
    rc = lib.cfm_icnn_f32(ctypes.byref(c))
    if rc == -1:
        raise _Declined()
    _lib.check(rc, "cfm_icnn_f32")


class _IcnnStepFunction(torch.autograd.Function):
    """loss of one F_STEP / G_STEP call; backward: the gradients that call left, times the upstream scalar.  params are the
    trained net's parameters() (the graph's leaves); the gradients share one buffer in their order."""

    @staticmethod
    def forward(ctx, op, f, g, x, y, reg, *params):
        sizes = [q.numel() for q in params]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=y.device)
        losses = torch.empty(3, dtype=torch.float32, device=y.device)
        p = torch.empty(y.shape, dtype=torch.float32, device=y.device)
        w = torch.empty_like(p) if op == _lib.ICNN_G_STEP else None
        _call(op, f, g, x if op == _lib.ICNN_F_STEP else None, y, reg, p, w, losses, flat)
        ctx.flat, ctx.sizes, ctx.shapes = flat, sizes, [q.shape for q in params]
        return losses[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        parts = (ctx.flat * gout).split(ctx.sizes)
        return (None, None, None, None, None, None, *[q.view(sh) for q, sh in zip(parts, ctx.shapes)])


def _cast(net, like, detach=False):
    """the net's parameters in like's dtype and on its device (detach: as constants)"""
    return {k: (p.detach() if detach else p).to(device=like.device, dtype=like.dtype) for k, p in net.named_parameters()}


def _apply(net, params, x):
    return torch.func.functional_call(net, params, (x,))


def _grad_map(net, params, y, create_graph):
    with torch.enable_grad():
        yg = y.detach().requires_grad_(True)
        return torch.autograd.grad(torch.sum(_apply(net, params, yg)), yg, create_graph=create_graph)[0]


def _penalty(params, reg):
    return reg * sum(torch.sum(torch.relu(-w) ** 2) / 2 for k, w in params.items() if k.startswith("Wzs.") and k.endswith(".weight"))


def _check(f, g, x, y):
    if x.dim() != 2 or y.shape != x.shape:
        raise ValueError(f"x and y are [B, d] of one shape; got {tuple(x.shape)} and {tuple(y.shape)}")
    for name, net in (("f", f), ("g", g)):
        if isinstance(net, ICNN) and net.dim != x.shape[1]:
            raise ValueError(f"{name} takes {net.dim} columns; x and y have {x.shape[1]}")


def icnn_g_loss(f, g, x, y, reg=0.1):
    """The g-objective of the minimax ICNN formulation (icnn_module.py:102-115):

        mean(f(grad g(y)) - y . grad g(y)) + reg sum_{W in g.Wzs} |relu(-W)|^2 / 2     (the penalty only when reg > 0).

    A scalar tensor whose ``.backward()`` leaves gradients on g's parameters ONLY: f is a constant here, as it is under
    Lightning's optimizer toggling, which switches f's ``requires_grad`` off while g's optimizer steps.  x takes no part in
    the value (the reference evaluates f(x) and drops it).  The HIP path is once differentiable."""
    _check(f, g, x, y)
    if _hip_ok((f, g), (x, y)):
        try:
            loss = _IcnnStepFunction.apply(_lib.ICNN_G_STEP, f, g, x, y, reg, *g.parameters())
            icnn_g_loss.last_path = "hip"
            return loss
        except _Declined:
            pass
    icnn_g_loss.last_path = "generic"
    fp, gp = _cast(f, y, detach=True), _cast(g, y)
    p = _grad_map(g, gp, y, torch.is_grad_enabled())
    loss = torch.mean(_apply(f, fp, p) - torch.sum(y * p, dim=1, keepdim=True))
    return loss + _penalty(gp, reg) if reg > 0 else loss


def icnn_f_loss(f, g, x, y, reg=0.1):
    """The f-objective (icnn_module.py:116-126): mean(f(x) - f(grad g(y))) + reg sum_{W in f.Wzs} |relu(-W)|^2 / 2.
    A scalar tensor whose ``.backward()`` leaves gradients on f's parameters only: grad g(y) is a constant of this step.
    The HIP path is once differentiable."""
    _check(f, g, x, y)
    if _hip_ok((f, g), (x, y)):
        try:
            loss = _IcnnStepFunction.apply(_lib.ICNN_F_STEP, f, g, x, y, reg, *f.parameters())
            icnn_f_loss.last_path = "hip"
            return loss
        except _Declined:
            pass
    icnn_f_loss.last_path = "generic"
    fp = _cast(f, x)
    p = _grad_map(g, _cast(g, y, detach=True), y, False).detach()
    loss = torch.mean(_apply(f, fp, x) - _apply(f, fp, p))
    return loss + _penalty(fp, reg) if reg > 0 else loss


def icnn_w2(f, g, x, y, return_loss=False):
    """``compute_w2`` (icnn_module.py:229-245): mean(f(grad g(y)) - f(x) - y . grad g(y) + |x|^2 / 2 + |y|^2 / 2), and with
    ``return_loss`` also (f_loss, g_loss) = (mean(f(x) - f(grad g(y))), mean(f(grad g(y)) - y . grad g(y))) without the
    penalty terms, exactly as the reference.  Values only: 0-dim tensors without a graph."""
    _check(f, g, x, y)
    if _hip_ok((f, g), (x, y)):
        try:
            losses = torch.empty(3, dtype=torch.float32, device=y.device)
            _call(_lib.ICNN_W2, f, g, x, y, 0.0, torch.empty_like(y, memory_format=torch.contiguous_format), None, losses)
            icnn_w2.last_path = "hip"
            return (losses[0], losses[1], losses[2]) if return_loss else losses[0]
        except _Declined:
            pass
    icnn_w2.last_path = "generic"
    with torch.no_grad():
        fp = _cast(f, x)
        p = _grad_map(g, _cast(g, y), y, False)
        fx, fgy = _apply(f, fp, x), _apply(f, fp, p)
        ydp = torch.sum(y * p, dim=1, keepdim=True)
        w2 = torch.mean(fgy - fx - ydp + 0.5 * torch.sum(x ** 2, dim=1, keepdim=True) + 0.5 * torch.sum(y ** 2, dim=1, keepdim=True))
        return (w2, torch.mean(fx - fgy), torch.mean(fgy - ydp)) if return_loss else w2


icnn_g_loss.last_path = None
icnn_f_loss.last_path = None
icnn_w2.last_path = None
