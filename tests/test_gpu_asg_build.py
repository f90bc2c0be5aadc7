"""GPU: the candidate lists and bounds that asg_build leaves in the workspace, BITWISE against the NumPy restatement of
the rule (tests/asg_build_restate.py) fed the prices the build read (the workspace keeps a copy: the list solver moves
the prices afterwards).  One solve per case through the public entry, the lists through cfm_assign_debug_lists.

The shapes are the smallest at which each path of the kernel can go wrong:
    1024           smallest fast-path size (strip in registers, prices in LDS)
    2048           fast path, padding slots (fewer than 16 float4 per lane)
    4096           the C3 geometry
    576, 1000      slow path (LDS strips), ragged last strip
    64             tau = +inf: every column listed
    1024, tied     integer costs: rows on which the bisection runs out of fp32 thresholds (the non-convergence exit)
    4 x 1024       the batch entry: one carving per problem (blockIdx.y)
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import asg_build_restate as R
import cfm_oracle as oracle

pytestmark = pytest.mark.gpu


def _geo(n, d, seed, dev, count=1):
    """bench-style minibatches: Gaussian source, clamped mixture of ten as target."""
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


def _tied(n, kind, dev):
    """Heavily tied integer costs.  "grid": squared distances of points on the integer grid {0..3}^3 (integers in
    0..27, every column sixteen times); "small": independent integers in 0..3; "binary": 0 / 1."""
    g = torch.Generator().manual_seed(77)
    if kind == "grid":
        x0 = torch.randint(0, 4, (n, 3), generator=g).float()
        x1 = torch.randint(0, 4, (n, 3), generator=g).float()
        M = ((x0[:, None, :] - x1[None, :, :]) ** 2).sum(-1)
    else:
        M = torch.randint(0, 4 if kind == "small" else 2, (n, n), generator=g).float()
    return M.contiguous().to(dev)


def _lists(lib, ws, n, b=0):
    cl = np.zeros((n, R.SP_K, 2), dtype=np.uint32)
    cT = np.zeros(n, dtype=np.float64)
    p = np.zeros(n, dtype=np.float64)
    rc = lib.cfm_assign_debug_lists(ctypes.c_void_p(ws.data_ptr()), n, b, cl.ctypes.data_as(ctypes.c_void_p),
                                    cT.ctypes.data_as(ctypes.c_void_p), p.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return cl, cT, p


def _compare(M, got, what):
    cl, cT, p = got
    assert np.any(p != 0.0), (what, "the solve never reached the list build")
    want_cl, want_cT, tau, cnt = R.build_lists(M.cpu().numpy(), p)
    n = M.shape[0]
    bad_cl = np.nonzero((cl != want_cl).any(axis=(1, 2)))[0]
    bad_cT = np.nonzero(cT.view(np.uint64) != want_cT.view(np.uint64))[0]
    print(f"{what}: n={n} members min/median/max {cnt.min()}/{int(np.median(cnt))}/{cnt.max()}, rows below 32: "
          f"{int((cnt < 32).sum())}, rows with differing lists {bad_cl.size}, bounds {bad_cT.size}")
    assert bad_cl.size == 0, (what, "lists differ in rows", bad_cl[:8].tolist())
    assert bad_cT.size == 0, (what, "bounds differ in rows", bad_cT[:8].tolist())
    return cnt


def _solve_single(M):
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    lib = _lib.load()
    n = M.shape[0]
    ws = _lib.workspace(_lib.OP_ASSIGN, n, n, 0, M.device)
    ws.zero_()
    perm = ot.assign_exact(M)
    torch.cuda.synchronize()
    assert sorted(perm.cpu().tolist()) == list(range(n))
    return _lists(lib, ws, n)


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    return _lib.require_gpu()


@pytest.mark.parametrize("n,d", [(1024, 64), (2048, 64), (576, 16), (1000, 16)])
def test_lists_match_the_restatement(dev, n, d):
    M = _geo(n, d, 500 + n, dev)[0]
    cnt = _compare(M, _solve_single(M), f"geo {n}")
    assert np.all((cnt >= 32) & (cnt <= 64))


def test_c3_geometry(dev):
    import cfm_amd.optimal_transport as ot
    x0, x1 = oracle.config_inputs("C3")
    M = ot.cost_matrix(x0.to(dev), x1.to(dev))
    assert M.shape[0] == 4096
    cnt = _compare(M, _solve_single(M), "C3")
    assert np.all((cnt >= 32) & (cnt <= 64))


DEFAULT_STOP_FRAC, DEFAULT_ARR_CAP = 0.02, 10      # the library's tuning record (the initialiser of g_params in csrc/assign.hip)


def test_every_column_listed_at_64(dev):
    """At n = 64 the auction usually matches every row and the solve goes straight to its certificate: no lists.  The
    epsilon phases are cut early (a quarter of the rows unmatched) so that free rows are left for the list solver; the
    first instance whose solve reached the build is compared."""
    from cfm_amd import _lib
    lib = _lib.load()
    lib.cfm_assign_set_small(0)          # (n <= 256 takes the one-workgroup solver otherwise)
    got = None
    try:
        for arr_cap in (-1, 1):          # (then with a single epsilon = 0 round as well)
            lib.cfm_assign_set_params(0, 0, 0, 0.25, 0, arr_cap, 0)
            for seed in range(6):
                M = _geo(64, 8, 564 + seed, dev)[0]
                got = _solve_single(M)
                if np.any(got[2] != 0.0):
                    break
            if np.any(got[2] != 0.0):
                break
    finally:
        lib.cfm_assign_set_params(0, 0, 0, DEFAULT_STOP_FRAC, 0, DEFAULT_ARR_CAP, 0)
        lib.cfm_assign_set_small(1)
    print(f"n = 64: arr_cap {arr_cap}, seed {seed}")
    cnt = _compare(M, got, "all listed 64")
    assert np.all(cnt == 64) and np.all(got[1] == np.inf)


def test_tied_integer_costs_take_the_exit(dev):
    """Rows on which more than 32 columns share one fp32 r: no threshold keeps 32..64 of them and the bisection ends on
    its `lo < mid < hh` test.  Whether a tied instance leaves such rows depends on the prices its auction ends with, so
    every kind is compared and at least one must have exercised the exit."""
    import time
    took_exit = []
    for kind in ("grid", "small", "binary"):
        M = _tied(1024, kind, dev)
        t0 = time.perf_counter()
        got = _solve_single(M)
        print(f"tied {kind}: solved in {1e3 * (time.perf_counter() - t0):.1f} ms")
        cnt = _compare(M, got, f"tied {kind}")
        took_exit.append(bool(np.any(cnt < 32)))
    assert any(took_exit), "no row took the bisection's non-convergence exit: the instances are not tied enough"


def test_batch_of_four(dev):
    import cfm_amd.optimal_transport as ot
    from cfm_amd import _lib
    lib = _lib.load()
    n, nb = 1024, 4
    Ms = _geo(n, 64, 900, dev, count=nb)
    ws = _lib.workspace(_lib.OP_ASSIGN, n, n, nb, dev)
    ws.zero_()
    perm = ot.assign_exact_batch(Ms)
    torch.cuda.synchronize()
    assert perm.shape == (nb, n)
    for b in range(nb):
        _compare(Ms[b], _lists(lib, ws, n, b), f"batch problem {b}")
