"""GPU (-m gpu): the conventions at the top of include/cfm_gfx950.h for cfm_icnn_f32, whose stream travels in its descriptor
and which the case table of tests/stream_cases.py therefore does not find by itself.

The four operations are stream_cases.Case objects with true (seed 0) and decoy (seed 1) inputs, run through
  * the side-stream-behind-a-delay protocol of tests/test_gpu_stream_contract.py: all work goes on the given stream, and
    the descriptor (a host object that is dropped when the call returns) is consumed during the call;
  * the poisoned, guarded-buffer protocol of tests/test_gpu_memory_contract.py: p, w, losses, the gradient buffer and the
    workspace filled with 0x00, 0xFF and stale bytes between guard zones; outputs written whole, nothing else written;
    a declining call (reg < 0: CFM_EINVAL before any HIP call) writes nothing.
Both modules' helpers are called, none of their tests.  The memory module tallies the fills each case id ran under and
reads back only the ids of its own parametrisation; the ids added here (cfm_icnn_f32-...) are none of them.

The shape (B = 40, d = 3, dimh = 33, L = 3) leaves a partial last tile, three workgroups and no dimension on a multiple of
the tile; every output and the workspace come from torch.empty inside the op, which is what the harness guards."""
import pytest
import torch

import icnn_restate as ir
import stream_cases as sc
import test_gpu_memory_contract as mem
import test_gpu_stream_contract as stc

pytestmark = pytest.mark.gpu

ENTRY = "cfm_icnn_f32"
B, D, H, L = 40, 3, 33, 3
dev = stc.dev
delay = stc.delay


def _make(seed, device):
    inp = {}
    for n, P in (("f", ir.gen_params(40 + seed, D, H, L)), ("g", ir.gen_params(50 + seed, D, H, L))):
        for k, v in P.items():
            inp[n + "." + k] = torch.tensor(v, dtype=torch.float32, device=device)
    x, y = ir.gen_data(60 + seed, B, D)
    inp["x"] = torch.tensor(x, dtype=torch.float32, device=device)
    inp["y"] = torch.tensor(y, dtype=torch.float32, device=device)
    return inp


def _net(inp, n):
    """an ICNN whose parameters ARE the case's buffers (no copy: the entry must read them where the protocol put them)"""
    import cfm_amd
    net = cfm_amd.ICNN(D, H, L)
    for k in ir.names(L):
        mod, idx, attr = k.split(".")
        setattr(getattr(net, mod)[int(idx)], attr, torch.nn.Parameter(inp[n + "." + k]))
    return net


def _op(opcode, reg=0.1):
    def op(inp):
        from cfm_amd import _lib, icnn
        from cfm_amd.ode import _Declined
        f, g = _net(inp, "f"), _net(inp, "g")
        device = inp["x"].device
        p = torch.empty(B, D, dtype=torch.float32, device=device)
        w = torch.empty(B, D, dtype=torch.float32, device=device) if opcode == _lib.ICNN_G_STEP else None
        losses = torch.empty(3, dtype=torch.float32, device=device) if opcode != _lib.ICNN_TRANSPORT else None
        step = opcode in (_lib.ICNN_F_STEP, _lib.ICNN_G_STEP)
        flat = torch.empty(sum(q.numel() for q in f.parameters()), dtype=torch.float32, device=device) if step else None
        x = None if opcode == _lib.ICNN_G_STEP else inp["x"]
        y = None if opcode == _lib.ICNN_TRANSPORT else inp["y"]
        try:
            icnn._call(opcode, f, g if y is not None else None, x, y, reg, p, w, losses, flat)
            rc = 0
        except _Declined:
            rc = -1
        outs = [(n, t, None) for n, t in (("p", p), ("w", w), ("losses", losses), ("grads", flat)) if t is not None]
        return outs, (rc,)
    return op


CASES = [sc.Case(ENTRY, name, _make, _op(code)) for code, name in enumerate(("transport", "w2", "f_step", "g_step"))]
DECLINES = sc.Case(ENTRY, "declines", _make, _op(3, reg=-1.0))
DECLINES.declines = True


def test_the_table_does_not_cover_this_entry_by_itself():
    """when this fails the entry has a `void* stream` parameter or a table case: fold these cases into the table"""
    assert ENTRY not in sc.CASES and ENTRY not in sc.EXEMPT


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_operation_on_a_side_stream_behind_a_delay(dev, delay, case):
    true, decoy = case.make(0, dev), case.make(1, dev)
    ref_outs, ref_host, _k1 = stc._run(case, true)
    dec_outs, _, _k2 = stc._run(case, stc._mix(decoy, true))
    assert stc._differs(dec_outs, ref_outs), (case.id, "the decoy gives the true result: this case tests nothing")
    outs, host, busy, call_ms, calls = stc._side_stream_run(case, true, decoy, delay, case.op)
    print(f"\n[icnn contract] {case.id}: call returned after {call_ms:.2f} ms, stream busy at return: {busy}, entry calls: {calls}")
    assert calls == 1, (case.id, "one call of the C entry per operation")
    assert busy, (case.id, "not tested: the side stream was idle when the call returned", call_ms)
    stc._same(case, outs, host, ref_outs, ref_host, "side stream")


@pytest.mark.parametrize("case", CASES + [DECLINES], ids=[c.id for c in CASES + [DECLINES]])
def test_operation_on_poisoned_guarded_buffers(dev, case):
    try:
        bad = mem._contract(case, dev)
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):        # the device context is gone: nothing after this means anything
            pytest.exit(f"{case.id}: {e}", returncode=3)
        raise
    assert not bad, "\n".join([case.id] + bad)
