"""GPU: the roads through the exact solver's HOST driver that the default configuration does not take — plain launches
instead of replayed hipGraphs, the polled chunk programs as the main road, the dense state machine alone, a cached
program whose identity a setter has changed, the thread's wait mode, and more program combinations than a thread keeps.

Every case must return, on generic costs (unique optimum), the permutation of the default path AND of
`cfm_oracle.exact_perm`, and must leave the process-wide dense-fallback counter of `cfm_assign_debug_fallback` where
it was.  These are the product's own roads on valid inputs.

`python tests/test_gpu_assign_driver.py OUT.npz` is the child of the plain-launch case: CFM_ASG_GRAPH is read once per
process, so that case solves in a fresh process and the parent compares what it saved."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "oracle")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import cfm_oracle as oracle

pytestmark = pytest.mark.gpu

# the defaults of the library's tuning record (the initialiser of g_params in csrc/assign.hip)
DEFAULT_BULK, DEFAULT_BULK_MIN_N, DEFAULT_CHUNK, DEFAULT_MODE = 96, 512, 10, 1
GEO = {512: 8, 1024: 64}          # n -> d of the geometric instances
NB = 4


def _geo_batch(n, d, count, seed, dev):
    """`count` cost matrices of bench.synth_batches-style minibatches: Gaussian source, clamped mixture of ten as target."""
    import cfm_amd.optimal_transport as ot
    g = torch.Generator().manual_seed(seed)
    mu = torch.rand(10, d, generator=g) * 2 - 1
    out = []
    for _ in range(count):
        x0 = torch.randn(n, d, generator=g)
        k = torch.randint(0, 10, (n,), generator=g)
        x1 = torch.clamp(0.35 * torch.randn(n, d, generator=g) + mu[k], -1, 1)
        out.append(ot.cost_matrix(x0.to(dev), x1.to(dev)))
    return out


def _matrices(dev):
    """{512: [4 matrices], 1024: [4 matrices], 4096: [the C3 instance]} — the same in every process."""
    import cfm_amd.optimal_transport as ot
    Ms = {n: _geo_batch(n, d, NB, 100 + n, dev) for n, d in GEO.items()}
    x0, x1 = oracle.config_inputs("C3")
    Ms[4096] = [ot.cost_matrix(x0.to(dev), x1.to(dev))]
    return Ms


def _fallback(lib):
    fb = (ctypes.c_int * 2)()
    lib.cfm_assign_debug_fallback(fb)
    return int(fb[0]), int(fb[1])


def _solve_all(Ms):
    """Single solves of the first matrix of every size and the batch of four at n = 512 and n = 1024."""
    import cfm_amd.optimal_transport as ot
    out = {}
    for n, ms in Ms.items():
        out[f"single_{n}"] = ot.assign_exact(ms[0]).cpu().numpy()
        if len(ms) == NB:
            out[f"batch_{n}"] = ot.assign_exact_batch(ms).cpu().numpy()
    return out


@pytest.fixture(scope="module")
def ctx():
    """The instances, their optimum by SciPy, and the default path's permutations (checked against SciPy here)."""
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    lib = _lib.load()
    Ms = _matrices(dev)
    ref = {n: [oracle.exact_perm(m.cpu().numpy()) for m in ms] for n, ms in Ms.items()}
    fb0 = _fallback(lib)
    want = {n: [ot.assign_exact(m).cpu().numpy() for m in ms] for n, ms in Ms.items()}
    for n in Ms:
        for b in range(len(Ms[n])):
            assert np.array_equal(want[n][b], ref[n][b]), (n, b)
        if len(Ms[n]) == NB:
            pb = ot.assign_exact_batch(Ms[n]).cpu().numpy()
            for b in range(NB):
                assert np.array_equal(pb[b], want[n][b]), (n, b)
    assert _fallback(lib) == fb0
    return {"dev": dev, "lib": lib, "Ms": Ms, "ref": ref, "want": want}


def _check(ctx, n, b, perm, what=""):
    perm = perm.cpu().numpy() if torch.is_tensor(perm) else np.asarray(perm)
    assert np.array_equal(perm, ctx["want"][n][b]), (what, n, b, "differs from the default path")
    assert np.array_equal(perm, ctx["ref"][n][b]), (what, n, b, "differs from the oracle")


def _check_single(ctx, n, what=""):
    import cfm_amd.optimal_transport as ot
    _check(ctx, n, 0, ot.assign_exact(ctx["Ms"][n][0]), what)


def _check_batch(ctx, n, what=""):
    import cfm_amd.optimal_transport as ot
    pb = ot.assign_exact_batch(ctx["Ms"][n])
    for b in range(NB):
        _check(ctx, n, b, pb[b], what)


def _restore(lib, saved_async):
    lib.cfm_assign_set_bulk(DEFAULT_BULK, DEFAULT_BULK_MIN_N)
    lib.cfm_assign_set_params(0, 0, 0, -1, 0, -1, DEFAULT_CHUNK)
    lib.cfm_assign_set_mode(DEFAULT_MODE)
    lib.cfm_assign_set_async(saved_async[0], saved_async[1], saved_async[2])
    now = (ctypes.c_int * 3)(); lib.cfm_assign_get_async(now)
    assert list(now) == list(saved_async)


def _saved_async(lib):
    saved = (ctypes.c_int * 3)(); lib.cfm_assign_get_async(saved)
    return saved


def test_plain_launches_in_a_fresh_process(ctx, tmp_path):
    """CFM_ASG_GRAPH=0: every program is issued launch by launch.  Single solves (512, 1024, C3) and batches of four."""
    out = str(tmp_path / "plain.npz")
    env = dict(os.environ, CFM_ASG_GRAPH="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    got = np.load(out)
    assert int(got["graph_env"]) == 0
    assert list(got["fallback_before"]) == list(got["fallback_after"]), "the dense fallback ran in the child"
    for n, ms in ctx["Ms"].items():
        _check(ctx, n, 0, got[f"single_{n}"], "plain single")
        if len(ms) == NB:
            for b in range(NB):
                _check(ctx, n, b, got[f"batch_{n}"][b], "plain batch")


def test_polled_chunks_as_the_main_road(ctx):
    """cfm_assign_set_bulk(0, 0): no unpolled head, the solve runs on the polled chunk program from its first launch."""
    lib = ctx["lib"]
    saved = _saved_async(lib)
    fb0 = _fallback(lib)
    try:
        lib.cfm_assign_set_bulk(0, 0)
        for n in ctx["Ms"]:
            _check_single(ctx, n, "bulk 0")
        for n in GEO:
            _check_batch(ctx, n, "bulk 0")
    finally:
        _restore(lib, saved)
    assert _fallback(lib) == fb0
    _check_single(ctx, 1024, "defaults restored")


@pytest.mark.parametrize("n", [512, 1024])
def test_dense_machine_only(ctx, n):
    """cfm_assign_set_mode(0): no candidate lists, no one-workgroup list solver — the chip-wide forest phases finish."""
    lib = ctx["lib"]
    saved = _saved_async(lib)
    fb0 = _fallback(lib)
    try:
        lib.cfm_assign_set_mode(0)
        _check_single(ctx, n, "dense only")
        _check_batch(ctx, n, "dense only")
    finally:
        _restore(lib, saved)
    assert _fallback(lib) == fb0
    _check_single(ctx, n, "defaults restored")


@pytest.mark.parametrize("n", [512, 1024, 4096])
def test_a_setter_changes_the_identity_of_a_cached_program(ctx, n):
    """One workspace, one stream: the programs captured by the first solve must not be replayed once `chunk` or the
    asynchronous mode differ — every later solve returns what the first did."""
    lib = ctx["lib"]
    saved = _saved_async(lib)
    fb0 = _fallback(lib)
    try:
        _check_single(ctx, n, "first")
        lib.cfm_assign_set_params(0, 0, 0, -1, 0, -1, 6)
        _check_single(ctx, n, "chunk 6")
        for mode in (0, 1, 2):
            lib.cfm_assign_set_async(mode, -1, -1)
            _check_single(ctx, n, f"chunk 6, async {mode}")
    finally:
        _restore(lib, saved)
    assert _fallback(lib) == fb0
    _check_single(ctx, n, "defaults restored")


@pytest.mark.parametrize("n", [512, 1024, 4096])
def test_wait_mode_of_the_thread_changes_between_solves(ctx, n):
    """cfm_set_blocking_sync: the events of a cached program are re-made when the thread's wait mode changed."""
    lib = ctx["lib"]
    fb0 = _fallback(lib)
    try:
        _check_single(ctx, n, "spin")
        lib.cfm_set_blocking_sync(1)
        _check_single(ctx, n, "yield")
        if n in GEO:
            _check_batch(ctx, n, "yield")
        lib.cfm_set_blocking_sync(0)
        _check_single(ctx, n, "spin again")
    finally:
        lib.cfm_set_blocking_sync(0)
    assert _fallback(lib) == fb0


def test_more_program_combinations_than_a_thread_keeps(ctx):
    """Six (workspace, n, nb, stream) combinations on one thread, cycled twice: the four slots evict and re-capture."""
    lib = ctx["lib"]
    fb0 = _fallback(lib)
    side = torch.cuda.Stream(device=ctx["dev"])
    torch.cuda.synchronize()

    def on_side(fn, *a):
        with torch.cuda.stream(side):
            fn(*a)
            side.synchronize()

    for cycle in range(2):
        for n in GEO:
            _check_single(ctx, n, f"cycle {cycle}")
            _check_batch(ctx, n, f"cycle {cycle}")
            on_side(_check_single, ctx, n, f"cycle {cycle}, side stream")
    assert _fallback(lib) == fb0


def _child(out):
    from cfm_amd import _lib
    dev = _lib.require_gpu()
    lib = _lib.load()
    torch.cuda.set_device(dev)
    Ms = _matrices(dev)
    fb0 = _fallback(lib)
    got = _solve_all(Ms)
    torch.cuda.synchronize()
    np.savez(out, graph_env=np.int64(int(os.environ.get("CFM_ASG_GRAPH", "1"))), fallback_before=np.array(fb0),
             fallback_after=np.array(_fallback(lib)), **got)


if __name__ == "__main__":
    _child(sys.argv[1])
