"""GPU (-m gpu): the three promises of include/cfm_gfx950.h's conventions, on the case table of tests/stream_cases.py.

1. Side-stream fidelity.  Every entry that takes a `stream` is run on a fresh side stream behind a ~30 ms delay, on working
   buffers that hold DECOY inputs until copies enqueued on that same stream (behind the delay) bring the true ones in.  A
   launch, memset or copy the entry left on the null stream runs at once, reads a decoy (or writes before the solve does)
   and gives another answer; the result must equal the default-stream result bit for bit.  The case only counts when the
   stream was still busy as the call returned (the entries that synchronise the host excepted) and when the decoy's own
   result differs from the true one.  The side stream is one the null stream does not queue behind (_fresh_side_stream:
   about one torch stream in four shares the null stream's hardware queue, where null-stream work would wait for the
   delay and the protocol would see nothing), and the protocol is run once on an op that IS left on the null stream.
2. Host arrays.  A HOST data array (t_span, step records) may be overwritten as soon as the call returns: behind the same
   delay the array is overwritten with the decoy grid right after the call, and the result must be the true grid's.
3. Threads.  Two host threads, each on its own stream and its own problem, get their single-threaded results bit for bit
   (the adaptive drivers' read-back buffer is per thread).

The oracle throughout is the entry's own default-stream result on an idle device."""
import functools
import threading
import time

import numpy as np
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

DELAY_MS = 30.0


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


@pytest.fixture(scope="session")
def delay():
    """enqueue() puts ~DELAY_MS of device work on the current stream and returns at once.  Calibrated once per session with
    events; not a tolerance: the only requirement on it is the query() condition of the tests."""
    torch.cuda.set_device(0)
    if hasattr(torch.cuda, "_sleep"):
        probe = 20_000_000
        torch.cuda._sleep(1000)
        ms = min(_timed_ms(lambda: torch.cuda._sleep(probe)) for _ in range(3))
        cycles = int(probe * DELAY_MS / ms)
        enqueue = lambda: torch.cuda._sleep(cycles)      # noqa: E731
        what = f"torch.cuda._sleep({cycles})"
    else:
        a = torch.randn(4096, 4096, device="cuda:0")
        a @ a
        ms = min(_timed_ms(lambda: a @ a) for _ in range(3))
        reps = max(1, int(round(DELAY_MS / ms)))

        def enqueue():
            for _ in range(reps):
                a @ a
        what = f"{reps} matmuls of 4096^2"
    got = _timed_ms(enqueue)
    print(f"\n[stream contract] delay: {what} = {got:.1f} ms")
    assert got >= 0.5 * DELAY_MS, got
    return enqueue


# --------------------------------------------------------------------------------------------------------- harness
def _clone(inp):
    return {k: (v.clone() if torch.is_tensor(v) else v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def _device_keys(inp):
    return [k for k, v in inp.items() if torch.is_tensor(v) and not k.startswith("_")]


def _mix(device_from, host_from):
    """Device buffers of one set, host arguments (grids, records, scalars) of the other."""
    out = _clone(host_from)
    for k in _device_keys(device_from):
        out[k] = device_from[k].clone()
    return out


def _run(case, inp):
    """One default-stream run on a private copy, synchronised.  Returns (outs, host, the copy that keeps outs' inputs alive)."""
    c = _clone(inp)
    if case.prep:
        case.prep(c)
    outs, host = case.op(c)
    torch.cuda.synchronize()
    if host:
        assert host[0] == 0, (case.id, host)
    for name, t, _ in outs:
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), (case.id, name, "non-finite output: the inputs are not valid")
    return outs, host, c


def _same(case, outs, host, ref_outs, ref_host, what):
    assert host == ref_host, (case.id, what, host, ref_host)
    assert [o[0] for o in outs] == [o[0] for o in ref_outs]
    for (name, a, rtol), (_, b, _) in zip(outs, ref_outs):
        if rtol is None:
            assert torch.equal(a, b), (case.id, what, name, "differs from the default-stream result")
        else:
            assert torch.allclose(a.double(), b.double(), rtol=rtol, atol=0.0), (case.id, what, name, rtol)


def _differs(outs, ref_outs):
    """Beyond run-to-run noise: an exact output with another bit, or a tolerance output 1000 tolerances away."""
    for (_, a, rtol), (_, b, _) in zip(outs, ref_outs):
        if rtol is None:
            if not torch.equal(a, b):
                return True
        elif not torch.allclose(a.double(), b.double(), rtol=1e3 * rtol, atol=0.0):
            return True
    return False


class _Count:
    """Counting wrapper set on the loaded library object in place of the named entry."""

    def __init__(self, name):
        from cfm_amd import _lib
        self.lib, self.name, self.n = _lib.load(), name, 0

    def __enter__(self):
        self.orig = getattr(self.lib, self.name)

        def counted(*a):
            self.n += 1
            return self.orig(*a)
        setattr(self.lib, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.orig)


def _fresh_side_stream(delay):
    """A fresh stream that the NULL stream does not queue behind.  The runtime multiplexes its streams onto a few hardware
    queues (four by default), and packets of one hardware queue run in order: null-stream work that shares the side stream's
    queue starts only after the delay, sees the true inputs, and a launch left on the null stream would go unnoticed.  So
    each candidate is probed: with the delay queued on it, a small null-stream operation must finish within a third of the
    delay (measured on the host: query() of the candidate lags the end of its work) and while the candidate is still busy."""
    null = torch.cuda.default_stream()
    probe = torch.zeros(64, device="cuda")
    probe.add_(1.0)
    for attempt in range(16):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay()
        t0 = time.perf_counter()
        with torch.cuda.stream(null):
            probe.add_(1.0)
        null.synchronize()
        independent = 1e3 * (time.perf_counter() - t0) < DELAY_MS / 3 and not s.query()
        s.synchronize()
        if independent:
            return s, attempt
    pytest.fail("not tested: every candidate side stream shares its hardware queue with the null stream")


def _side_stream_run(case, true, decoy, delay, op):
    """op on working buffers that hold the decoys until the side stream, behind the delay, copies the true inputs in.
    Returns (outs, host, stream busy when the call returned, host time of the call in ms, calls of the C entry)."""
    work = _mix(decoy, true)
    if case.prep:
        case.prep(work)
    side, skipped = _fresh_side_stream(delay)
    print(f"\n[stream contract] side stream {side.cuda_stream:#x} (candidates that shared the null stream's queue: {skipped})")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        delay()
        for k in _device_keys(true):
            work[k].copy_(true[k], non_blocking=True)
        t0 = time.perf_counter()
        with _Count(case.entry) as cnt:
            outs, host = op(work)
        busy = not side.query()
        call_ms = 1e3 * (time.perf_counter() - t0)
        side.synchronize()
    torch.cuda.synchronize()
    return outs, host, busy, call_ms, cnt.n


ALL = sc.all_cases()


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_entry_on_a_side_stream_behind_a_delay(dev, delay, case):
    true, decoy = case.make(0, dev), case.make(1, dev)
    assert _device_keys(true) == _device_keys(decoy)
    for k in _device_keys(true):
        assert true[k].shape == decoy[k].shape and true[k].dtype == decoy[k].dtype, k
    ref_outs, ref_host, _k1 = _run(case, true)
    dec_outs, _, _k2 = _run(case, _mix(decoy, true))
    assert _differs(dec_outs, ref_outs), (case.id, "the decoy gives the true result: this case tests nothing")

    outs, host, busy, call_ms, calls = _side_stream_run(case, true, decoy, delay, case.op)
    print(f"\n[stream contract] {case.id}: call returned after {call_ms:.2f} ms, stream busy at return: {busy}, "
          f"entry calls: {calls}")
    assert calls >= 1, (case.id, "the named C entry was not called")
    if not case.syncs:
        assert busy, (case.id, "not tested: the side stream was idle when the call returned (delay too short, or the "
                               "call waited for the stream)", call_ms)
    _same(case, outs, host, ref_outs, ref_host, "side stream")


def test_the_protocol_catches_work_left_on_the_null_stream(dev, delay):
    """The harness on itself: the same protocol with an op that (wrongly) enqueues on the null stream does not wait for
    the side stream's copies, reads the decoys, and must NOT reproduce the default-stream result."""
    case = sc.CASES["cfm_sqeuclid_cost_f32"][0]
    true, decoy = case.make(0, dev), case.make(1, dev)
    ref_outs, _, _k1 = _run(case, true)
    dec_outs, _, _k2 = _run(case, decoy)

    def on_the_null_stream(inp):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return case.op(inp)
    outs, _, busy, _, calls = _side_stream_run(case, true, decoy, delay, on_the_null_stream)
    assert busy and calls == 1
    assert _differs(outs, ref_outs), "null-stream work waited for the side stream: the protocol cannot see it"
    assert not _differs(outs, dec_outs)


HOST_CASES = [sc.CASES[e][0] for e in sc.HOST_DATA] + [c for e, n in sc.HOST_DATA_EXTRA for c in sc.CASES[e] if c.name == n]


@pytest.mark.parametrize("case", HOST_CASES, ids=[c.id for c in HOST_CASES])
def test_host_array_may_be_overwritten_when_the_call_returns(dev, delay, case):
    true, decoy = case.make(0, dev), case.make(1, dev)
    hk = [k for k in sc.HOST_KEYS if k in true]
    assert len(hk) == 1, hk
    hk = hk[0]
    assert true[hk].shape == decoy[hk].shape and true[hk].dtype == decoy[hk].dtype and not np.array_equal(true[hk], decoy[hk])
    ref_outs, ref_host, _k1 = _run(case, true)
    other = dict(true)
    other[hk] = decoy[hk]
    alt_outs, _, _k2 = _run(case, other)
    assert _differs(alt_outs, ref_outs), (case.id, "the decoy grid gives the true grid's result: this case tests nothing")

    work = _clone(true)
    if case.prep:
        case.prep(work)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay()
        t0 = time.perf_counter()
        outs, host = case.op(work)
        work[hk][...] = decoy[hk]              # the array the entry was given, overwritten in place
        busy = not side.query()
        call_ms = 1e3 * (time.perf_counter() - t0)
        side.synchronize()
    print(f"\n[stream contract] {case.id}: host array overwritten {call_ms:.2f} ms after the call began, stream busy then: {busy}")
    assert busy, (case.id, "not tested: the side stream was idle when the call returned", call_ms)
    _same(case, outs, host, ref_outs, ref_host, "host array overwritten after return")
    assert _differs(outs, alt_outs)


# --------------------------------------------------------------------------------------------------------- threads
def _problem(make, op, dev):
    """(solve, reference): solve() runs the entry on the current stream on this problem's own buffers and returns its outputs
    on the host and its host results; reference is solve() on the default stream, single-threaded."""
    inp = make(0, dev)
    torch.cuda.synchronize()

    def solve():
        outs, host = op(_clone(inp))
        torch.cuda.current_stream().synchronize()
        return [(n, t.cpu()) for n, t, _ in outs], host
    return solve, solve()


def _adaptive(B, d, n_t, tab, tol, salt):
    return sc._mk_ode(B=B, d=d, n_t=n_t, salt=salt), sc._op_adaptive("cfm_ode_adaptive_mlp_f32", tab, tol)


def _sinkhorn_problem():
    def op(inp):
        from cfm_amd import optimal_transport as ot
        r = ot.sinkhorn_log(inp["M"], sc.REG, max_iter=50, stop_thr=0.0)
        return [("f", r.f, None), ("g", r.g, None), ("iters", r.iters, None)], ()
    return sc._mk_cost, op


PAIRS = {
    "persistent-dopri5-vs-tsit5": lambda: (_adaptive(300, 2, 9, 0, 1e-4, 31), _adaptive(300, 5, 12, 1, 1e-5, 32)),
    "layer-path-pair": lambda: (_adaptive(300, 2, 50, 0, 1e-6, 33), _adaptive(257, 2, 47, 1, 1e-6, 34)),
    "cnf-adaptive-vs-recording": lambda: (
        (sc._mk_ode(B=300, aug=1, salt=35), sc._op_cnf_adaptive("cfm_ode_adaptive_cnf_mlp_f32", 0, 1, 1e-5)),
        (sc._mk_ode(B=300, n_t=12, salt=36), functools.partial(sc._op_rec, tol=1e-4))),
    "control-sinkhorn-vs-assign": lambda: (_sinkhorn_problem(), (sc._mk_square(1), sc._op_assign)),
}
LOOPS = 8


@pytest.mark.parametrize("pair", list(PAIRS))
def test_two_threads_on_different_problems(dev, pair):
    """Each thread loops over ITS OWN problem (other x, net seed, tolerance and grid than the other thread's); every
    iteration equals that thread's single-threaded result bit for bit, host results included."""
    from cfm_amd import _lib
    lib = _lib.load()
    layers = pair == "layer-path-pair"
    if layers:
        lib.cfm_ode_set_fused(0)
    try:
        problems = [_problem(mk, op, dev) for mk, op in PAIRS[pair]()]
        for _, (outs, host) in problems:
            print(f"\n[stream contract] {pair}: single-threaded host results {host}")
            if host:
                assert host[0] == 0, host
        if layers:          # hundreds of read-backs per thread
            assert all(ref[1][1] * LOOPS >= 200 for _, ref in problems), [ref[1] for _, ref in problems]
        barrier = threading.Barrier(2)
        got, errs = [[], []], []

        def work(k):
            try:
                torch.cuda.set_device(dev)
                with torch.cuda.stream(torch.cuda.Stream()):
                    barrier.wait(timeout=30)
                    for _ in range(LOOPS):
                        got[k].append(problems[k][0]())
            except Exception as e:       # noqa: BLE001
                errs.append(repr(e))

        th = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(2)]
        [t.start() for t in th]
        [t.join(timeout=60) for t in th]
        assert not any(t.is_alive() for t in th), "a solver thread did not finish within 60 s"
    finally:
        if layers:
            lib.cfm_ode_set_fused(1)
    assert not errs, errs
    for k in range(2):
        ref_outs, ref_host = problems[k][1]
        assert len(got[k]) == LOOPS
        for it, (outs, host) in enumerate(got[k]):
            assert host == ref_host, (pair, k, it, host, ref_host)
            for (name, a), (_, b) in zip(outs, ref_outs):
                assert torch.equal(a, b), (pair, k, it, name)
