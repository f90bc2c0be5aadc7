"""The harness of tests/footprint_util.py on itself, on CPU tensors: plain torch ops stand in for kernels.  It must catch
each fault it exists for (a store behind or in front of a buffer, an output element never written, scratch read before it
is written) and stay quiet on a correct op."""
import pytest
import torch

import footprint_util as fu
from footprint_util import GUARD, guarded

CPU = torch.device("cpu")
_ORIG = [getattr(torch, n) for n in fu._PATCHED]
N = 37          # odd, and 37 * 4 bytes is no multiple of any allocator rounding


def _raw(t, n):
    """The n elements of t's storage from t's first element on, bounds ignored (what a kernel's pointer arithmetic sees)."""
    return t.as_strided((n,), (1,))


def _x():
    return torch.arange(1, N + 1, dtype=torch.float32)


def op_correct(x):
    out = torch.empty_like(x)
    scratch = torch.empty(N, dtype=torch.float64)
    scratch.copy_(x)                    # written before it is read
    out.copy_(scratch * 2)
    return out


def op_past_the_end(x):
    out = torch.empty(N, dtype=torch.float32)
    _raw(out, N + 1).copy_(torch.cat([x * 2, torch.ones(1)]))
    return out


def op_before_the_start(x):
    out = torch.empty(N, dtype=torch.float32)
    out.copy_(x * 2)
    out.as_strided((1,), (1,), out.storage_offset() - 1).fill_(3.0)
    return out


def op_skips_last(x):
    out = torch.empty_like(x)
    out[:-1].copy_(x[:-1] * 2)
    return out


def op_reads_scratch_first(x):
    scratch = torch.empty(N, dtype=torch.float32)
    out = torch.empty_like(x)
    out.copy_(x * 2 + scratch)          # the partial sums were never zeroed
    return out


def _run(op, fill, prev=None):
    g = guarded(fill, CPU)
    if prev is not None:
        g.stale_from(prev)
    with g:
        out = op(_x())
    return g, out


def _bits(t):
    return t.contiguous().view(torch.uint8)


def test_view_sits_between_two_guards():
    with guarded("ff", CPU) as g:
        t = torch.empty((3, 5), dtype=torch.float64)
        z = torch.zeros(7, dtype=torch.int32)
    assert GUARD % 512 == 0
    assert t.shape == (3, 5) and t.dtype == torch.float64 and t.is_contiguous() and bool(torch.isnan(t).all())
    assert z.dtype == torch.int32 and not bool(z.any())
    r = g.records[0]
    assert r.arena.numel() == 3 * 5 * 8 + 2 * GUARD and t.data_ptr() == r.arena.data_ptr() + GUARD
    assert bool((r.arena[:GUARD] == fu.GUARD_BYTE).all()) and bool((r.arena[GUARD + 120:] == fu.GUARD_BYTE).all())
    assert t.data_ptr() % 64 == 0
    assert g.check() == [] and g.untouched()
    with guarded("00", CPU) as g0:
        i = torch.empty(4, dtype=torch.int64)
    assert not bool(i.any())
    with guarded("ff", CPU):
        i = torch.empty(4, dtype=torch.int64)
    assert bool((i == -1).all())


def test_a_store_one_element_past_the_output_is_reported():
    g, _ = _run(op_past_the_end, "00")
    assert g.check() == [(0, (N,), torch.float32, "back", 0, 4)]       # 1.0f = 00 00 80 3f: four bytes off the pattern


def test_a_store_one_element_before_the_output_is_reported():
    g, _ = _run(op_before_the_start, "00")
    bad = g.check()
    assert len(bad) == 1 and bad[0][:4] == (0, (N,), torch.float32, "front") and -4 <= bad[0][4] < 0


def test_an_in_place_op_on_a_guarded_copy_of_its_input():
    x = _x()
    with guarded("ff", CPU) as g:
        c = g.copy_of(x)
        c.mul_(2)
    assert torch.equal(c, x * 2) and g.check() == [] and g.untouched() and g.records[0].kind == "copy"
    with guarded("ff", CPU) as g:
        c = g.copy_of(x)
        _raw(c, N + 1).mul_(2)                 # one element too many
    assert [b[:4] for b in g.check()] == [(0, (N,), torch.float32, "back")]      # (doubling a float leaves its low bytes)


def test_a_skipped_last_element_differs_between_the_fills():
    (_, a), (_, b) = _run(op_skips_last, "00"), _run(op_skips_last, "ff")
    assert not torch.equal(_bits(a), _bits(b))
    assert torch.equal(a[:-1], b[:-1]) and float(a[-1]) == 0.0 and bool(torch.isnan(b[-1]))


def test_scratch_read_before_written_differs_between_the_fills():
    (g0, a), (g1, b) = _run(op_reads_scratch_first, "00"), _run(op_reads_scratch_first, "ff")
    assert g0.check() == [] and g1.check() == []
    assert not torch.equal(_bits(a), _bits(b))
    # ... and under the stale fill: the scratch holds what the previous run's first allocation was left with
    prev, _ = _run(op_reads_scratch_first, "00")
    prev.records[0].body.view(torch.float32).fill_(5.0)
    _, c = _run(op_reads_scratch_first, "stale", prev)
    assert torch.equal(c, _x() * 2 + 5.0)


def test_a_correct_op_passes_all_three_fills():
    ref = op_correct(_x())
    g0, a = _run(op_correct, "00")
    g1, b = _run(op_correct, "ff")
    g2, c = _run(op_correct, "stale", g1)
    for g, t in ((g0, a), (g1, b), (g2, c)):
        assert g.check() == [] and torch.equal(_bits(t), _bits(ref)) and len(g.records) == 2
    assert not g0.untouched() and not g1.untouched()


def test_other_devices_zero_sizes_and_out_pass_through():
    with guarded("ff", CPU) as g:
        m = torch.empty(5, device="meta")
        e = torch.empty(0)
        e2 = torch.zeros((0, 3))
        dst = torch.ones(4)
        r = torch.zeros(4, out=dst)
    assert m.device.type == "meta" and e.numel() == 0 and e2.shape == (0, 3)
    assert r.data_ptr() == dst.data_ptr() and not bool(dst.any())
    assert g.records == []
    with guarded("ff", torch.device("meta")) as g:          # the target is another device: CPU requests are torch's own
        t = torch.empty(8)
        u = torch.empty_like(t)
    assert g.records == [] and t.device.type == "cpu" and u.device.type == "cpu"


def test_patched_functions_are_restored_after_an_exception():
    orig = [getattr(torch, n) for n in fu._PATCHED]
    with pytest.raises(RuntimeError, match="boom"):
        with guarded("00", CPU):
            assert torch.empty is not orig[0]
            raise RuntimeError("boom")
    assert [getattr(torch, n) for n in fu._PATCHED] == orig
    with guarded("00", CPU):
        pass
    assert [getattr(torch, n) for n in fu._PATCHED] == orig


def test_stale_from_refuses_another_allocation_sequence():
    prev, _ = _run(op_correct, "ff")                       # float32 [N], then float64 [N]
    with pytest.raises(AssertionError, match="allocation 1"):
        _run(op_reads_scratch_first, "stale", prev)        # float32 [N], float32 [N]
    with pytest.raises(AssertionError, match="allocations"):
        _run(op_skips_last, "stale", prev)                 # one allocation instead of two
    with pytest.raises(AssertionError):
        with guarded("stale", CPU):
            pass
    assert [getattr(torch, n) for n in fu._PATCHED] == _ORIG      # (restored after each refusal)
