"""A guarded, poisoned allocation harness: WHERE an entry writes, and what it reads before it has written it.

    with guarded("ff") as g:          # or guarded("00"), or guarded("stale").stale_from(previous_run)
        outs = op(inputs)             # every torch.empty / empty_like / zeros / zeros_like on g.device is served here
    bad = g.check()                   # [] or [(ordinal, shape, dtype, side, first bad offset, count), ...]

While the context is active torch.empty, torch.empty_like, torch.zeros and torch.zeros_like are replaced (and restored in
every case).  An allocation on the target device comes from a private uint8 arena of nbytes + 2 * GUARD bytes; the tensor
handed out is a view of arena[GUARD : GUARD + nbytes] in the requested dtype and shape, so the back guard begins at the
FIRST byte past the request (torch's own allocator rounds a request up to 512 bytes: a store a few elements past a buffer
lands in slack nobody looks at).  Both guards hold GUARD_BYTE.  GUARD is a multiple of 512: the view keeps the alignment
torch would give.  Everything else passes through unchanged: other devices, pinned memory, out=, zero-sized requests,
non-strided layouts.

The `empty` kinds are filled, on the current stream, with
  "00"     byte 0x00;
  "ff"     byte 0xFF: a negative NaN in fp32 / fp64, -1 in the integer types;
  "stale"  the bytes a PREVIOUS guarded run (of another problem with the same allocation sequence) left in the allocation
           of the same ordinal: stale_from(previous) replays them and raises when sizes or dtypes differ, ordinal by ordinal.
The `zeros` kinds stay zero; copy_of(t) hands out a guarded copy of an existing tensor (a working copy of an input).  Both constant fills are needed: each equals a pattern some driver memsets for itself (zeros;
the all-ones sentinels), so a missing initialisation hides behind one and shows under the other; the stale fill is the
production situation, plausible values of another solve.

A workspace cache between the caller and the allocator (cfm_amd._lib._ws_tls.cache) is cleared by the CALLER before a
guarded run, so that the workspace is carved afresh inside the harness, and after it, so that no guarded view outlives the
run's bookkeeping (clear_workspace_cache).  The harness keeps every arena alive until it is dropped itself.

Two things the harness CANNOT see: a store further than GUARD bytes from a buffer (it lands in another allocation or in
unmapped memory), and any out-of-bounds READ (only its effect on a result, if the fills differ there).

Importing this module needs no device: it is tested on CPU tensors (tests/test_footprint_util_host.py)."""
import torch

GUARD = 4096
GUARD_BYTE = 0xA5
FILLS = ("00", "ff", "stale")

_PATCHED = ("empty", "empty_like", "zeros", "zeros_like")


class _Rec:
    __slots__ = ("arena", "nbytes", "shape", "dtype", "kind")

    def __init__(self, arena, nbytes, shape, dtype, kind):
        self.arena, self.nbytes, self.shape, self.dtype, self.kind = arena, nbytes, shape, dtype, kind

    @property
    def body(self):
        return self.arena[GUARD:GUARD + self.nbytes]


def _dense(t):
    """The elements of t fill numel() consecutive slots in some order of the dimensions (contiguous, channels-last, ...)."""
    run = 1
    for stride, size in sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz > 1):
        if stride != run:
            return False
        run *= size
    return True


def clear_workspace_cache():
    """Drop the calling thread's cached workspaces of cfm_amd._lib (the only cache of device buffers in the package: the
    results of cfm_amd.optimal_transport own their buffers)."""
    from cfm_amd import _lib
    _lib._ws_tls.cache = {}


class guarded:
    def __init__(self, fill, device=None):
        assert fill in FILLS, fill
        self.fill = fill
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = self._norm(torch.device(device))
        self.records = []
        self._prev = None
        self._orig = None

    # ------------------------------------------------------------------------------------------------ set-up
    @staticmethod
    def _norm(dev):
        if dev.type == "cuda" and dev.index is None:
            return torch.device("cuda", torch.cuda.current_device())
        return dev

    def stale_from(self, previous):
        """The finished guarded run whose buffers' last contents fill this run's allocations.  Returns self."""
        assert self.fill == "stale" and isinstance(previous, guarded) and previous._orig is None
        self._prev = previous
        return self

    def __enter__(self):
        assert self._orig is None and not self.records, "one run per harness object"
        if self.fill == "stale":
            assert self._prev is not None, 'guarded("stale") needs stale_from(previous)'
        self._orig = {n: getattr(torch, n) for n in _PATCHED}
        try:
            for n in _PATCHED:
                setattr(torch, n, self._wrap(n))
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, et, ev, tb):
        self._restore()
        if et is None and self._prev is not None and len(self.records) != len(self._prev.records):
            raise AssertionError(f"stale_from: this run made {len(self.records)} allocations, the previous one "
                                 f"{len(self._prev.records)}")
        return False

    def _restore(self):
        if self._orig is not None:
            for n, f in self._orig.items():
                setattr(torch, n, f)
            self._orig = None

    # ------------------------------------------------------------------------------------------------ allocation
    def _wrap(self, name):
        orig = self._orig[name]
        like = name.endswith("_like")
        kind = "zeros" if name.startswith("zeros") else "empty"

        def alloc(*args, **kw):
            if kw.get("out") is not None or kw.get("pin_memory"):
                return orig(*args, **kw)
            dev = kw.get("device")
            if dev is None:
                dev = args[0].device if like else self._orig["empty"](0).device      # torch's default device
            if self._norm(torch.device(dev)) != self.device:
                return orig(*args, **kw)
            meta = orig(*args, **{**kw, "device": "meta"})       # shape, dtype and strides as torch would choose them
            if meta.numel() == 0 or meta.layout != torch.strided or not _dense(meta):
                return orig(*args, **kw)
            return self._serve(kind, meta, bool(kw.get("requires_grad")))
        alloc.__name__ = name
        return alloc

    def _serve(self, kind, meta, requires_grad):
        empty = self._orig["empty"]
        nbytes = meta.numel() * meta.element_size()
        arena = empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=self.device)
        arena[:GUARD].fill_(GUARD_BYTE)
        arena[GUARD + nbytes:].fill_(GUARD_BYTE)
        rec = _Rec(arena, nbytes, tuple(meta.shape), meta.dtype, kind)
        k = len(self.records)
        if self._prev is not None:
            if k >= len(self._prev.records):
                raise AssertionError(f"stale_from: allocation {k} has no counterpart in the previous run")
            p = self._prev.records[k]
            if (p.nbytes, p.dtype, p.kind) != (rec.nbytes, rec.dtype, rec.kind):
                raise AssertionError(f"stale_from: allocation {k} is {rec.kind} {rec.shape} {rec.dtype}, the previous run's "
                                     f"was {p.kind} {p.shape} {p.dtype}")
        if kind == "copy":
            pass                                  # copy_of fills it
        elif kind == "zeros":
            rec.body.zero_()
        elif self.fill == "00":
            rec.body.zero_()
        elif self.fill == "ff":
            rec.body.fill_(0xFF)
        else:
            rec.body.copy_(self._prev.records[k].body)
        self.records.append(rec)
        t = rec.body.view(meta.dtype).as_strided(meta.shape, meta.stride())
        return t.requires_grad_() if requires_grad else t

    def copy_of(self, t):
        """A guarded copy of a tensor on the target device (a working copy of an INPUT: an in-place entry's only buffer gets
        its guards this way).  Inside the context only; counted as an allocation of kind "copy", which no fill touches."""
        assert self._orig is not None and t.device == self.device and t.numel() > 0 and _dense(t)
        c = self._serve("copy", self._orig["empty_like"](t, device="meta"), False)
        c.copy_(t)
        return c

    # ------------------------------------------------------------------------------------------------ verdicts
    def check(self):
        """The violated guards: (ordinal, shape, dtype, side, first bad offset, count).  The offset is in bytes relative to
        the buffer: negative in front of its first byte, 0 = the first byte past its end."""
        if not self.records:
            return []
        # one reduction for the common case: nothing touched
        dirty = torch.stack([(r.arena[:GUARD] != GUARD_BYTE).any() | (r.arena[GUARD + r.nbytes:] != GUARD_BYTE).any()
                             for r in self.records])
        bad = []
        for k in dirty.nonzero().flatten().tolist():
            r = self.records[k]
            for side, g, base in (("front", r.arena[:GUARD], -GUARD), ("back", r.arena[GUARD + r.nbytes:], 0)):
                hit = (g != GUARD_BYTE).nonzero().flatten()
                if hit.numel():
                    bad.append((k, r.shape, r.dtype, side, base + int(hit[0]), int(hit.numel())))
        return bad

    def untouched(self):
        """True when every buffer still holds exactly what the harness put there (a call that declines writes nothing).
        Under the stale fill that is the previous run's buffer as it is NOW: keep the previous run's buffers unchanged."""
        for k, r in enumerate(self.records):
            if r.kind == "copy":
                continue
            if r.kind == "zeros" or self.fill == "00":
                same = not bool(r.body.any())
            elif self.fill == "ff":
                same = bool((r.body == 0xFF).all())
            else:
                same = torch.equal(r.body, self._prev.records[k].body)
            if not same:
                return False
        return True
