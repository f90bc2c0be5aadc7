"""The regression step of the reference's training loops as ONE call into the HIP library.

Every loop of the reference ends the same way (examples/images/cifar10/train_cifar10.py:141-151, the 2-D
tutorials, single-cell_example.ipynb cell 6):

    optimizer.zero_grad()
    t, xt, ut = FM.sample_location_and_conditional_flow(x0, x1)
    vt = model(torch.cat([xt, t[:, None]], dim=-1))
    loss = torch.mean((vt - ut) ** 2)
    loss.backward()
    optimizer.step()

``RegressionStep(model, optimizer)(t, xt, ut)`` is the last four lines for a ``cfm_amd.MLP`` field and a
``cfm_amd.FusedAdam``: ``cfm_mlp_regression_step_f32`` (forward with the time column fused into the first layer's
epilogue, MSE + its gradient seed, dgrad / wgrad, one fixed-order reduction) followed by ``cfm_adam_step_f32`` — 14
launches of this library's kernels and no eager PyTorch op in between (the eager form spends ~10 extra
``at::native`` launches on cat / sub / pow / mean / fill per step).  Same arithmetic as the autograd path
(same kernels); gradients land in persistent ``.grad`` buffers, so the optimizer's pointer table is built once.
With ``torch.distributed`` initialised (one process per GPU, rank-local coupling) the gradients are averaged the way
the reference's DDP wrapper does it (train_cifar10_ddp.py:92,167-180): one bucket per layer, all-reduced on a
communication stream as soon as that layer's gradient is final (``layer_done`` events recorded by the C call between
its launches) while the remaining layers' products still run; the compute stream waits for the buckets, and the
``1 / world`` of the mean is a factor inside the Adam launch (``grad_scale``) — no eager op in the step for N > 1 either.

``SF2MStep(model, score_model, optimizer)(t, xt, ut, eps, lambda_t)`` is the same for the [SF]2M loops
(examples/2D_tutorials/SF2M_tutorial.ipynb cell 3, single-cell_example.ipynb, runner/src/models/cfm_module.py:896-909):
a flow net and a score net of equal layer sizes under one optimizer, ``cfm_mlp_sf2m_step_f32`` — every launch of the
regression step serving both nets — followed by one ``cfm_adam_step_f32`` over all parameters of both.

``DSBMStep(forward_model, backward_model, optimizer)(t, xt, forward_target, backward_target, forward_scaling,
backward_scaling)`` is the same driver for DSBM (runner/src/models/cfm_module.py:1215-1227): a forward and a backward drift
net, each under a row-weighted MSE, ``cfm_mlp_dsbm_step_f32``.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .models import MLP


class _FusedStep:
    """What the fused steps share, for one net or two of equal layer sizes: the flat gradient buffer with every ``.grad``
    a view of it, the activation buffers and workspaces per batch size, the pointer tables, the batch checks."""

    def _setup(self, nets):
        """nets: one or two checked MLPs (fp32, biased, on one GPU, equal layer sizes); the first one's layers come first
        in ``lins`` and in every table."""
        self.net, self.n_nets = nets[0], len(nets)
        self.dims = nets[0].dims()
        self.n = len(self.dims) - 1
        self.lins = [l for net in nets for l in net._linears()]
        self.dev = self.lins[0].weight.device
        # ONE flat gradient buffer; every parameter's .grad is a view of it (one all-reduce for data parallel runs)
        self.flat_grad = torch.zeros(sum(l.weight.numel() + l.bias.numel() for l in self.lins), dtype=torch.float32, device=self.dev)
        self._gviews, off = [], 0
        for l in self.lins:
            for p in (l.weight, l.bias):
                v = self.flat_grad[off:off + p.numel()].view_as(p); off += p.numel()
                p.grad = v
                self._gviews.append(v)
        self._B = None

    def _buffers(self, B):
        """hidden / preact (the first net's layers first), one loss-gradient seed g and one workspace per net, and their
        host tables; rebuilt only when the batch size changes."""
        if self._B != B:
            d, n, dev, nets = self.dims, self.n, self.dev, range(self.n_nets)
            self.hidden = [torch.empty((B, d[l + 1]), dtype=torch.float32, device=dev) for _ in nets for l in range(n - 1)]
            self.preact = [torch.empty((B, d[l + 1]), dtype=torch.float32, device=dev) for _ in nets for l in range(n - 1)]
            self.g = [torch.empty((B, d[n]), dtype=torch.float32, device=dev) for _ in nets]      # own allocations: aligned alike
            one = _lib.load().cfm_workspace_bytes(_lib.OP_MLP_TRAIN, B, max(d), max(d[l] * d[l + 1] for l in range(n)))
            self.ws = torch.empty(self.n_nets * one, dtype=torch.uint8, device=dev)      # the nets' workspaces back to back
            m = max(1, self.n_nets * (n - 1))
            self.hp = (ctypes.c_void_p * m)(*([h.data_ptr() for h in self.hidden] or [0]))
            self.zp = (ctypes.c_void_p * m)(*([z.data_ptr() for z in self.preact] or [0]))
            self.cd = (ctypes.c_int * (n + 1))(*d)
            self._B = B

    def _tables(self):
        """(W, b, dW, db): host tables of n_nets * n device pointers, the first net's layers first.  The parameters' storage
        may have moved (load_state_dict keeps it, .to() does not), so the pointers are taken per call; a replaced .grad is
        put back."""
        for v, p in zip(self._gviews, (q for l in self.lins for q in (l.weight, l.bias))):
            if p.grad is not v:
                p.grad = v
        N = len(self.lins)
        return ((ctypes.c_void_p * N)(*[l.weight.data_ptr() for l in self.lins]),
                (ctypes.c_void_p * N)(*[l.bias.data_ptr() for l in self.lins]),
                (ctypes.c_void_p * N)(*[self._gviews[2 * l].data_ptr() for l in range(N)]),
                (ctypes.c_void_p * N)(*[self._gviews[2 * l + 1].data_ptr() for l in range(N)]))

    def _in_width(self):
        """columns of xt: the first layer's input without the time column"""
        return self.dims[0] - int(bool(self.net.time_varying))

    def _xt_ut(self, who, xt, ut, same_rows):
        """(xt, ut, B) with xt and ut detached and reshaped to [B, -1], their columns checked against the layer sizes
        (same_rows: and ut's rows against xt's)."""
        xt = xt.detach().reshape(xt.shape[0], -1)
        ut = ut.detach().reshape(ut.shape[0], -1)
        B = xt.shape[0]
        if xt.shape[1] != self._in_width() or ut.shape[1] != self.dims[self.n] or (same_rows and ut.shape[0] != B):
            raise RuntimeError(f"{who}: xt has {xt.shape[1]} / ut has {ut.shape[1]} columns, the "
                               f"{'net maps' if self.n_nets == 1 else 'nets map'} {self._in_width()} (+ time) -> {self.dims[self.n]}")
        return xt, ut, B

    def _times(self, who, t, B):
        """t as a device vector with one time per row, or None for a net without a time column"""
        if not self.net.time_varying:
            return None
        tt = _lib.to_dev_f32(t.detach().reshape(-1), self.dev)
        if tt.numel() != B:
            raise RuntimeError(f"{who}: one time per row is required")
        return tt


class RegressionStep(_FusedStep):
    def __init__(self, model, optimizer, data_parallel=None):
        """data_parallel: None — the bucketed gradient all-reduce runs iff torch.distributed is initialised with more than
        one rank; True — whenever a process group exists, also with ONE rank (the N > 1 composition — communication
        stream, per-layer events, grad_scale — on the real backend of a one-GPU box); False — never."""
        self.data_parallel = data_parallel
        net = model.module if hasattr(model, "module") and isinstance(model.module, MLP) else model
        if not isinstance(net, MLP):
            raise TypeError("RegressionStep drives a cfm_amd.MLP vector field")
        self.opt = optimizer
        from .optim import FusedAdam
        self._fused_opt = isinstance(optimizer, FusedAdam)           # its step() takes the 1 / world of the mean (grad_scale)
        lins = net._linears()
        if lins[0].weight.device.type != "cuda" or any(l.weight.dtype != torch.float32 or l.bias is None for l in lins):
            raise TypeError("RegressionStep needs an fp32 MLP with biases on the GPU")
        self._setup([net])
        # per-layer buckets of the flat buffer ([W_l, b_l] are adjacent) + one event per layer for the data-parallel form
        self._buckets, off = [], 0
        for l in self.lins:
            nl = l.weight.numel() + l.bias.numel()
            self._buckets.append(self.flat_grad[off:off + nl]); off += nl
        self._events = self._comm = self._evp = None
        self.loss = torch.zeros((), dtype=torch.float32, device=self.dev)

    def _dp_setup(self):
        """events (created by a first record: torch makes the HIP event lazily) and the communication stream"""
        if self._events is None:
            cur = torch.cuda.current_stream(self.dev)
            self._events = [torch.cuda.Event() for _ in range(self.n)]
            for e in self._events:
                e.record(cur)
            self._evp = (ctypes.c_void_p * self.n)(*[e.cuda_event for e in self._events])
            self._comm = torch.cuda.Stream(device=self.dev)
        return self._evp

    def backward_only(self, t, xt, ut, layer_events=None):
        """forward + loss + backward; returns the loss (0-dim device tensor, overwritten by the next call).
        layer_events: ctypes array of n hipEvent_t (see ``cfm_mlp_regression_step_f32``: ``layer_done``) or None."""
        lib = _lib.load()
        xt, ut, B = self._xt_ut("RegressionStep", xt, ut, same_rows=False)
        xt = _lib.to_dev_f32(xt, self.dev); ut = _lib.to_dev_f32(ut, self.dev)
        tt = self._times("RegressionStep", t, B)
        self._buffers(B)
        Wp, bp, dWp, dbp = self._tables()
        check(lib.cfm_mlp_regression_step_f32(ptr(xt), ptr(tt), ptr(ut), Wp, bp, self.cd, self.n, B, self.hp, self.zp,
                                              ptr(self.g[0]), dWp, dbp, ptr(self.loss), layer_events, ptr(self.ws),
                                              stream_ptr()),
              "cfm_mlp_regression_step_f32")
        return self.loss

    def __call__(self, t, xt, ut):
        import torch.distributed as dist
        have_pg = dist.is_available() and dist.is_initialized()
        world = dist.get_world_size() if have_pg else 1
        if self.data_parallel is False or not have_pg or (world <= 1 and not self.data_parallel):
            loss = self.backward_only(t, xt, ut)
            self.opt.step()
            return loss
        evp = self._dp_setup()
        loss = self.backward_only(t, xt, ut, layer_events=evp)       # asynchronous: the backward is still running
        works = []
        with torch.cuda.stream(self._comm):
            for l in range(self.n - 1, -1, -1):                      # the order the gradients become final in
                self._comm.wait_event(self._events[l])
                works.append(dist.all_reduce(self._buckets[l], async_op=True))
        for w in works:
            w.wait()                                                 # the compute stream waits for the buckets
        if self._fused_opt:
            self.opt.step(grad_scale=1.0 / world)                    # sum -> mean inside the Adam launch
        else:                                                        # any other optimizer: scale the buckets, then its own step
            self.flat_grad.mul_(1.0 / world)
            self.opt.step()
        return loss


def _as_mlp(net, who, what):
    net = net.module if hasattr(net, "module") and isinstance(net.module, MLP) else net
    if not isinstance(net, MLP):
        raise TypeError(f"{who}: {what} is a {type(net).__name__}, not a cfm_amd.MLP")
    return net


def _need_fp32_gpu(who, nets):
    """nets: (Linear layers, what to call them) per net; biases first, then the dtype, then the device"""
    for lins, what in nets:
        if any(l.bias is None for l in lins):
            raise TypeError(f"{who}: {what} has a Linear layer without bias")
    for lins, what in nets:
        if any(l.weight.dtype != torch.float32 or l.bias.dtype != torch.float32 for l in lins):
            raise TypeError(f"{who}: {what} is not fp32")
    for lins, what in nets:
        if any(l.weight.device.type != "cuda" or l.bias.device != l.weight.device for l in lins):
            raise TypeError(f"{who}: {what} is not on the GPU")


class SF2MStep(_FusedStep):
    """The [SF]2M training step for a flow ``MLP`` and a score ``MLP`` of equal layer sizes:

        vt = model(torch.cat([xt, t[:, None]], dim=-1)); st = score_model(torch.cat([xt, t[:, None]], dim=-1))
        flow_loss = torch.mean((vt - ut) ** 2); score_loss = torch.mean((lambda_t[:, None] * st + eps) ** 2)
        (flow_loss + score_weight * score_loss).backward(); optimizer.step()

    ``step(t, xt, ut, eps, lambda_t)`` returns the device tensor ``[flow_loss, score_loss]`` (both unweighted, overwritten
    by the next call); ``lambda_t`` is the caller's ``FM.compute_lambda(...)``, one value per row."""

    MAX_LAYERS = 7      # cfm_mlp_sf2m_step_f32: the one final reduction holds the jobs of two 7-layer nets

    _WHO, _FIRST, _SECOND = "SF2MStep", "flow", "score"      # how the refusals name the step and its two nets

    def __init__(self, model, score_model, optimizer, score_weight=1.0):
        who, first, second = self._WHO, self._FIRST, self._SECOND
        net, self.score_net = _as_mlp(model, who, f"the {first} model"), _as_mlp(score_model, who, f"the {second} model")
        flins, slins = net._linears(), self.score_net._linears()
        dims, sdims = net.dims(), self.score_net.dims()
        if dims != sdims or bool(net.time_varying) != bool(self.score_net.time_varying):
            raise TypeError(f"{who}: the nets' layer sizes differ ({first} {dims}, {second} {sdims}): one launch serves both "
                            "nets only when their layers have equal sizes")
        _need_fp32_gpu(who, ((flins, f"the {first} model"), (slins, f"the {second} model")))
        if slins[0].weight.device != flins[0].weight.device:
            raise TypeError(f"{who}: the {second} model is not on the GPU of the {first} model")
        if net is self.score_net:
            raise TypeError(f"{who}: the {first} and the {second} model are the same module")
        self.opt, self.score_weight = optimizer, float(score_weight)
        self._setup([net, self.score_net])                            # flow first, score second: the order of every table
        self.losses = torch.zeros(2, dtype=torch.float32, device=self.dev)

    def backward_only(self, t, xt, ut, eps, lambda_t):
        """forward + both losses + backward of both nets; returns ``[flow_loss, score_loss]`` (device tensor)"""
        if self.n > self.MAX_LAYERS:
            raise RuntimeError(f"SF2MStep: the nets have {self.n} Linear layers; the fused step takes at most "
                               f"{self.MAX_LAYERS} (two nets' reduction jobs fill its one table)")
        lib = _lib.load()
        xt, ut, B = self._xt_ut("SF2MStep", xt, ut, same_rows=True)
        if eps.numel() != ut.numel() or eps.shape[0] != B:
            raise RuntimeError(f"SF2MStep: eps has shape {tuple(eps.shape)}, ut {tuple(ut.shape)}")
        if lambda_t.numel() != B:
            raise RuntimeError(f"SF2MStep: lambda_t has {lambda_t.numel()} values for {B} rows (one per row is required)")
        xt = _lib.to_dev_f32(xt, self.dev); ut = _lib.to_dev_f32(ut, self.dev)
        eps = _lib.to_dev_f32(eps.reshape(B, -1), self.dev); lam = _lib.to_dev_f32(lambda_t.reshape(-1), self.dev)
        tt = self._times("SF2MStep", t, B)
        self._buffers(B)
        Wp, bp, dWp, dbp = self._tables()
        check(lib.cfm_mlp_sf2m_step_f32(ptr(xt), ptr(tt), ptr(ut), ptr(eps), ptr(lam), Wp, bp, self.hp, self.zp, dWp, dbp,
                                        self.cd, self.n, B, ptr(self.g[0]), ptr(self.g[1]), ptr(self.losses),
                                        self.score_weight, ptr(self.ws), stream_ptr()),
              "cfm_mlp_sf2m_step_f32")
        return self.losses

    def loss(self):
        """``flow_loss + score_weight * score_loss`` of the last call (logging: not part of the step)"""
        return self.losses[0] + self.score_weight * self.losses[1]

    def __call__(self, t, xt, ut, eps, lambda_t):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("SF2MStep is not built for data parallel runs (its gradients would be stepped on "
                                      "unreduced); use one process, or RegressionStep for the flow net alone")
        losses = self.backward_only(t, xt, ut, eps, lambda_t)
        self.opt.step()
        return losses


class DSBMStep(SF2MStep):
    """The DSBM (diffusion Schrodinger bridge matching) training step for a forward and a backward drift ``MLP`` of equal
    layer sizes (runner/src/models/cfm_module.py:1215-1227; the batch is ``DSBMConditionalFlowMatcher``'s):

        f = forward_model(torch.cat([xt, t[:, None]], dim=-1)); b = backward_model(torch.cat([xt, t[:, None]], dim=-1))
        forward_loss = torch.mean(forward_scaling[:, None] * (f - forward_target) ** 2)
        backward_loss = torch.mean(backward_scaling[:, None] * (b - backward_target) ** 2)
        (forward_loss + backward_loss).backward(); optimizer.step()

    ``step(t, xt, forward_target, backward_target, forward_scaling, backward_scaling)`` returns the device tensor
    ``[forward_loss, backward_loss]`` (overwritten by the next call).  One ``cfm_mlp_dsbm_step_f32``: the two-net driver of
    ``SF2MStep`` with a row-weighted loss in the last layer's epilogue, the launch count of one regression step.  The
    reference raises "Loss Not Finite" on a non-finite loss (run:1224-1225); that check reads the loss on the host, a
    synchronisation the step does not make: it stays with the caller (``torch.isfinite(losses).all()`` when wanted)."""

    _WHO, _FIRST, _SECOND = "DSBMStep", "forward", "backward"

    def __init__(self, forward_model, backward_model, optimizer):
        n = len(_as_mlp(forward_model, self._WHO, "the forward model")._linears())
        if n > self.MAX_LAYERS:      # (refused here, not at the first step: nothing about it depends on the batch)
            raise TypeError(f"DSBMStep: the nets have {n} Linear layers; the fused step takes at most "
                            f"{self.MAX_LAYERS} (two nets' reduction jobs fill its one table)")
        super().__init__(forward_model, backward_model, optimizer, score_weight=1.0)
        self.backward_net = self.score_net

    def backward_only(self, t, xt, forward_target, backward_target, forward_scaling, backward_scaling):
        """forward + both losses + backward of both nets; returns ``[forward_loss, backward_loss]`` (device tensor)"""
        lib = _lib.load()
        xt = xt.detach().reshape(xt.shape[0], -1)
        B, n = xt.shape[0], self.n
        ft = forward_target.detach().reshape(forward_target.shape[0], -1)
        bt = backward_target.detach().reshape(backward_target.shape[0], -1)
        if xt.shape[1] != self._in_width() or ft.shape != (B, self.dims[n]) or bt.shape != ft.shape:
            raise RuntimeError(f"DSBMStep: xt has shape {tuple(xt.shape)}, the targets {tuple(ft.shape)} and {tuple(bt.shape)}; "
                               f"the nets map {self._in_width()} (+ time) -> {self.dims[n]}")
        if forward_scaling.numel() != B or backward_scaling.numel() != B:
            raise RuntimeError(f"DSBMStep: the scalings have {forward_scaling.numel()} and {backward_scaling.numel()} values "
                               f"for {B} rows (one per row is required)")
        xt = _lib.to_dev_f32(xt, self.dev); ft = _lib.to_dev_f32(ft, self.dev); bt = _lib.to_dev_f32(bt, self.dev)
        wf = _lib.to_dev_f32(forward_scaling.detach().reshape(-1), self.dev)
        wb = _lib.to_dev_f32(backward_scaling.detach().reshape(-1), self.dev)
        tt = self._times("DSBMStep", t, B)
        self._buffers(B)
        Wp, bp, dWp, dbp = self._tables()
        check(lib.cfm_mlp_dsbm_step_f32(ptr(xt), ptr(tt), ptr(ft), ptr(bt), ptr(wf), ptr(wb), Wp, bp, self.hp, self.zp, dWp, dbp,
                                        self.cd, n, B, ptr(self.g[0]), ptr(self.g[1]), ptr(self.losses), ptr(self.ws),
                                        stream_ptr()),
              "cfm_mlp_dsbm_step_f32")
        return self.losses

    def __call__(self, t, xt, forward_target, backward_target, forward_scaling, backward_scaling):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("DSBMStep is not built for data parallel runs (its gradients would be stepped on "
                                      "unreduced); use one process")
        losses = self.backward_only(t, xt, forward_target, backward_target, forward_scaling, backward_scaling)
        self.opt.step()
        return losses
