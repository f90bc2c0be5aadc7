"""GPU: every kernel-selection path of the entropic-OT unit at its edge shapes, against the plain float64 oracle.

cfm_sinkhorn_log_f32 picks its row pass from the shape (streaming / one-shot fast / generic with v in LDS or in
global memory, float4 or scalar loads) and its column strips from B0; the points variant stages the other cloud in
chunks of `stage_cap` points.  Each entry of TABLE names the path it selects; cfm_sinkhorn_dispatch_info (the host
helper the entry point itself calls) must report that path.

The sharp test is the SENTINEL solve: M = 40 reg everywhere but one zero per row, placed on the edge columns of every
unit / tile / segment boundary.  In the column pass a column that loses its sentinel (or counts it twice) moves its
potential by about 40 (by log 2); every row carries a sentinel, so every row and strip edge is covered as well.  Its
dual (one zero per column, the edge columns alone in their rows) is as sharp in the row pass, which the first form
cannot see (_row_sentinel_cases).  The bound stays the project's 1e-5 * max(|u|, |v|, 1).  All oracles here are NumPy float64 on the same fp32 matrix."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the one-shot child of test (f) runs this file as a script: no conftest there
    for _p in (ROOT, os.path.join(ROOT, "oracle")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import cfm_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-9            # unbalanced / partial plans on the same fp32 matrix (tests/test_gpu_unbalanced.py)
REG_SENT = 0.5         # sentinel solves: M = 40 * reg = 20.0 exactly in fp32
FIELDS = ("vec", "row_fast", "v_in_lds", "nchunk", "rows_per_chunk", "rows_per_wg", "row_wgs", "stream_nf4",
          "stream_want", "lds_bytes")


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _ot():
    import cfm_amd.optimal_transport as ot
    return ot


# (B0, B1, misaligned) -> (row pass, vec, v_in_lds, nchunk, rows_per_chunk)
#   row pass: "stream" = sk_row_stream<4> (sk_row_pass<true> under CFM_SK_STREAM=0), "generic" = sk_row_pass<false>
TABLE = {
    # stream, ONE workgroup: waves 1..7 have no row; one 1024-column unit per row
    (1, 1024, False): ("stream", 1, 1, 1, 1),
    # stream, two workgroups (rows 0..12 over 16 waves: three waves without a row); single-unit rows
    (13, 1024, False): ("stream", 1, 1, 1, 13),
    # stream, three units per row: the last unit of a row hands over to the prefetch of the wave's next row; 3 strips 23+23+21
    (67, 3072, False): ("stream", 1, 1, 3, 23),
    # stream at the LDS limit (v = 128 KiB), 16 units per row
    (5, 16384, False): ("stream", 1, 1, 1, 5),
    # stream with grid = CU count (257 workgroups wanted): waves walk 2 rows or 1; 64 column strips of 33 rows, the last
    # one empty, the one before it 9 rows (waves without rows); the sampler's row scan crosses 1024 twice
    (2055, 1024, False): ("stream", 1, 1, 64, 33),
    # misaligned M (a view one float into a larger buffer): scalar loads and the generic row pass, although B1 % 1024 == 0
    (40, 1024, True): ("generic", 0, 1, 2, 20),
    # a multiple of 1024 whose v does not fit LDS: generic, v from global memory, float4 loads
    (9, 17408, False): ("generic", 1, 0, 1, 9),
    # v from global memory, float4 loads, B1 % 256 != 0 (a last column tile of one float4); strips of 17 + 16 rows: waves without rows
    (33, 16388, False): ("generic", 1, 0, 2, 17),
    # v from global memory, scalar loads with a ragged last float4 (16390 = 4 * 4097 + 2); one strip of 6 rows: 3 waves without rows
    (6, 16390, False): ("generic", 0, 0, 1, 6),
    # generic, v in LDS just below the 48 KiB threshold of the LDS attribute (49120 B) ...
    (10, 6140, False): ("generic", 1, 1, 1, 10),
    # ... just above it (49184 B) ...
    (10, 6148, False): ("generic", 1, 1, 1, 10),
    # ... and at the top (131040 B)
    (12, 16380, False): ("generic", 1, 1, 1, 12),
    # generic float4 / scalar, two strips (17 + 16 rows)
    (33, 1028, False): ("generic", 1, 1, 2, 17),
    (33, 1027, False): ("generic", 0, 1, 2, 17),
    # generic scalar, a second column tile of ONE column
    (9, 257, False): ("generic", 0, 1, 1, 9),
    # generic float4, one strip of 31 / 32 rows (the last trip of wave 3 is one row short / full)
    (31, 64, False): ("generic", 1, 1, 1, 31),
    (32, 64, False): ("generic", 1, 1, 1, 32),
    # degenerate
    (1, 1, False): ("generic", 0, 1, 1, 1),
    (1, 5, False): ("generic", 0, 1, 1, 1),
    (5, 1, False): ("generic", 0, 1, 1, 5),
    (2, 3, False): ("generic", 0, 1, 1, 2),
}
SHAPES = list(TABLE)
_ids = [f"{b0}x{b1}{'_misaligned' if mis else ''}" for b0, b1, mis in SHAPES]
# one shape per row-pass family (c, d)
CONV_SHAPES = [(13, 1024, False), (67, 3072, False), (5, 16384, False), (2055, 1024, False), (33, 1027, False),
               (6, 16390, False), (40, 1024, True)]
_conv_ids = [_ids[SHAPES.index(s)] for s in CONV_SHAPES]


def _dispatch(B0, B1, aligned):
    from cfm_amd import _lib
    out = (ctypes.c_longlong * 16)()
    _lib.check(_lib.load().cfm_sinkhorn_dispatch_info(B0, B1, int(aligned), out), "cfm_sinkhorn_dispatch_info")
    return dict(zip(FIELDS, out))


def _pts_dispatch(B0, B1, d):
    from cfm_amd import _lib
    out = (ctypes.c_longlong * 8)()
    _lib.check(_lib.load().cfm_sinkhorn_points_dispatch_info(B0, B1, d, out), "cfm_sinkhorn_points_dispatch_info")
    return dict(zip(("stage_cap", "col_grid", "row_grid", "trip_u", "pre", "lds_bytes", "chunks_x0", "chunks_x1"), out))


def _to_dev(Mnp, dev, misaligned=False):
    """The fp32 matrix on the device; misaligned: a contiguous view one float into a larger buffer."""
    B0, B1 = Mnp.shape
    if not misaligned:
        M = torch.from_numpy(np.array(Mnp, dtype=np.float32)).to(dev)     # (a copy: the cached matrices are read-only)
        assert M.data_ptr() % 16 == 0
        return M
    buf = torch.zeros(B0 * B1 + 8, dtype=torch.float32, device=dev)
    M = buf[1:1 + B0 * B1].view(B0, B1)
    M.copy_(torch.from_numpy(np.array(Mnp, dtype=np.float32)))
    assert M.data_ptr() % 16 == 4 and M.is_contiguous()
    return M


def _potentials(r, B0, B1, dev):
    from cfm_amd import _lib
    lib = _lib.load()
    u = torch.empty(B0, dtype=torch.float64, device=dev)
    v = torch.empty(B1, dtype=torch.float64, device=dev)
    _lib.check(lib.cfm_sinkhorn_potentials_f64(_lib.ptr(r.ws), B0, B1, _lib.ptr(u), _lib.ptr(v),
                                               _lib.stream_ptr()), "potentials")
    return u.cpu().numpy(), v.cpu().numpy()


def _precise_word(r):
    """SkState.precise: int32 word 3 of the state block at the head of the workspace."""
    return int(r.ws[:16].cpu().view(torch.int32)[3])


def _dev_uv(u, v, uo, vo):
    """(max |u - uo|, max |v - vo|, potential scale of the project's bound)."""
    return (float(np.abs(u - uo).max()), float(np.abs(v - vo).max()),
            float(max(np.abs(uo).max(), np.abs(vo).max(), 1.0)))


# ------------------------------------------------------------------------------------------- inputs and oracles
@functools.lru_cache(maxsize=None)
def _clouds(B0, B1, d=2):
    """x0 ~ N(0, 1)^d, x1 ~ N(0, 1)^d + 0.5 (fp32), one seed for every shape."""
    rng = np.random.default_rng(0)
    x0 = rng.standard_normal((B0, d)).astype(np.float32)
    x1 = (rng.standard_normal((B1, d)) + 0.5).astype(np.float32)
    return x0, x1


@functools.lru_cache(maxsize=None)
def _cloud_cost(B0, B1):
    """The matrix of the cloud cases, built on the CPU: independent of the cost kernel."""
    M = oracle.sqeuclid_cost_f64(*_clouds(B0, B1)).astype(np.float32)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _oracle_fixed(B0, B1, reg, iters, check_every=10):
    return oracle.sinkhorn_log(_cloud_cost(B0, B1), reg, numItermax=iters, stopThr=0.0, check_every=check_every)


@functools.lru_cache(maxsize=None)
def _oracle_conv(B0, B1, reg, stop_thr):
    """(u, v, it, err at the stopping check, err at the check before it)."""
    M = _cloud_cost(B0, B1)
    u, v, it, err = oracle.sinkhorn_log(M, reg, stopThr=stop_thr)
    assert it < 1000 and it % 10 == 1 and it > 1
    _, _, _, err_before = oracle.sinkhorn_log(M, reg, numItermax=it - 10, stopThr=0.0)
    return u, v, it, err, err_before


def _edge_cols(B1):
    cand = [0, 3, 4, 63, 64, 255, 256, 1023, 1024, 4095, 4096, B1 - 5, B1 - 4, B1 - 1]
    return sorted({c for c in cand if 0 <= c < B1})


def _sentinel_cases(B0, B1):
    """M = 40 reg everywhere, M[i, pi_k(i)] = 0 with pi_k(i) = edge[(i + k) % len(edge)]; shifts k until every edge
    column has been hit (several tiny solves when B0 is small)."""
    edge = _edge_cols(B1)
    hit = set()
    for k in range(0, len(edge), B0):
        M = np.full((B0, B1), 40.0 * REG_SENT, dtype=np.float32)
        cols = [edge[(i + k) % len(edge)] for i in range(B0)]
        M[np.arange(B0), cols] = 0.0
        hit.update(cols)
        yield M
    assert hit == set(edge)


def _row_sentinel_cases(B0, B1):
    """The dual sentinel, sharp in the ROW pass.  With one zero per row and all other entries equal, the balanced
    structure of _sentinel_cases leaves every u within 3e-4 of 0 — the value u starts from — and a row's sentinel is
    one term among ~B1 equal ones: a row pass that loses an element, or never writes a row, stays inside the bound
    (measured: a streaming pass that skipped its last row passed at 2.7e-4 against a bound of 2.8e-4).  Here every
    COLUMN has exactly one zero, so after the column pass all v_j are equal and a row's sum is its zeros alone: each
    edge column is the only zero of a row of its own (spread over [0, B0 - 1], ends included), whose potential
    log(B1 / B0) per iteration moves by ~40 when that element is lost; the other columns are dealt round to the
    remaining rows, whose potentials differ from 0 by log of the uneven counts.  Needs two rows; edge columns in
    groups of at most B0 - 1."""
    edge = _edge_cols(B1)
    m = min(len(edge), B0 - 1)
    for k in range(0, len(edge), m):
        sub = edge[k:k + m]
        own = np.unique(np.linspace(0, B0 - 1, len(sub)).astype(np.int64))
        assert len(own) == len(sub)
        others = np.setdiff1d(np.arange(B0), own)
        rest = np.setdiff1d(np.arange(B1), sub)
        M = np.full((B0, B1), 40.0 * REG_SENT, dtype=np.float32)
        M[own, sub] = 0.0
        M[others[np.arange(len(rest)) % len(others)], rest] = 0.0
        assert ((M == 0).sum(0) == 1).all() and ((M[own] == 0).sum(1) == 1).all()
        yield M


def _run_sentinel(B0, B1, misaligned, dev, cases=None):
    ot = _ot()
    worst = (0.0, 0.0, 1.0)
    ok = True
    for Mnp in (cases or _sentinel_cases)(B0, B1):
        uo, vo, _, _ = oracle.sinkhorn_log(Mnp, REG_SENT, numItermax=2, stopThr=0.0)
        r = ot.sinkhorn_log(_to_dev(Mnp, dev, misaligned), REG_SENT, max_iter=2, stop_thr=0.0)
        du, dv, sc = _dev_uv(*_potentials(r, B0, B1, dev), uo, vo)
        assert int(r.iters.cpu()) == 2
        ok = ok and du <= 1e-5 * sc and dv <= 1e-5 * sc
        if max(du, dv) / sc >= max(worst[0], worst[1]) / worst[2]:
            worst = (du, dv, sc)
    return ok, worst


def _run_random(B0, B1, misaligned, dev):
    ot = _ot()
    reg, iters = 0.1, 30
    uo, vo, it_o, _ = _oracle_fixed(B0, B1, reg, iters)
    r = ot.sinkhorn_log(_to_dev(_cloud_cost(B0, B1), dev, misaligned), reg, max_iter=iters, stop_thr=0.0)
    du, dv, sc = _dev_uv(*_potentials(r, B0, B1, dev), uo, vo)
    df = float(np.abs(r.f.cpu().numpy() - reg * uo).max())
    dg = float(np.abs(r.g.cpu().numpy() - reg * vo).max())
    return dict(du=du, dv=dv, sc=sc, df=df, dg=dg, iters=int(r.iters.cpu()))


def _assert_random(res, reg=0.1, iters=30):
    assert res["iters"] == iters
    assert res["du"] <= 1e-5 * res["sc"] and res["dv"] <= 1e-5 * res["sc"], res
    # f = reg u, g = reg v in fp32: 1e-5 of the potential scale
    assert res["df"] <= 1e-5 * reg * res["sc"] and res["dg"] <= 1e-5 * reg * res["sc"], res


# ------------------------------------------------------------------------------------------- the selection itself
@pytest.mark.parametrize("B0,B1,mis", SHAPES, ids=_ids)
def test_helper_reports_the_path_of_the_table(dev, B0, B1, mis):
    path, vec, lds, nchunk, rpc = TABLE[(B0, B1, mis)]
    s = _dispatch(B0, B1, not mis)
    assert ("stream" if s["row_fast"] else "generic") == path
    assert (s["vec"], s["v_in_lds"], s["nchunk"], s["rows_per_chunk"]) == (vec, lds, nchunk, rpc)
    if path == "stream":
        assert s["stream_nf4"] == 4 and s["stream_want"] == -(-B0 // 8) and s["lds_bytes"] == 8 * B1
        assert B1 % 1024 == 0 and B1 <= 16384
    else:
        assert s["stream_nf4"] == 0 and s["stream_want"] == 0 and s["row_wgs"] == -(-B0 // 8)
    if (B0, B1) == (2055, 1024):
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        assert s["stream_want"] == 257 > cus and 8 * cus < B0 <= 16 * cus      # grid = CU count: waves walk 2 rows or 1
        assert 63 * rpc >= B0 > 62 * rpc              # 64 strips, the last one empty


# ------------------------------------------------------------------------------------------- (a) sentinel
@pytest.mark.parametrize("B0,B1,mis", SHAPES, ids=_ids)
def test_sentinel_solve(dev, B0, B1, mis):
    """Two iterations on the sentinel matrix: potentials within 1e-5 * max(|u|, |v|, 1) of the oracle, for every shift."""
    ok, (du, dv, sc) = _run_sentinel(B0, B1, mis, dev)
    print(f"sentinel {B0}x{B1}: max|du| {du:.3e} max|dv| {dv:.3e} scale {sc:.3f}")
    assert ok, (du, dv, sc)


@pytest.mark.parametrize("B0,B1,mis", [sh for sh in SHAPES if sh[0] >= 2], ids=[i for sh, i in zip(SHAPES, _ids) if sh[0] >= 2])
def test_sentinel_solve_sharp_in_the_row_pass(dev, B0, B1, mis):
    """The same two iterations on the dual sentinel (one zero per column, edge columns alone in their rows)."""
    ok, (du, dv, sc) = _run_sentinel(B0, B1, mis, dev, _row_sentinel_cases)
    print(f"row sentinel {B0}x{B1}: max|du| {du:.3e} max|dv| {dv:.3e} scale {sc:.3f}")
    assert ok, (du, dv, sc)


# ------------------------------------------------------------------------------------------- (b) random clouds
@pytest.mark.parametrize("B0,B1,mis", SHAPES, ids=_ids)
def test_random_clouds_fixed_iterations(dev, B0, B1, mis):
    res = _run_random(B0, B1, mis, dev)
    print(f"random {B0}x{B1}: {res}")
    _assert_random(res)


# ------------------------------------------------------------------------------------------- (c) fp64 regime
@pytest.mark.parametrize("B0,B1,mis", CONV_SHAPES, ids=_conv_ids)
def test_convergence_through_the_fp64_regime(dev, B0, B1, mis):
    """reg = 2, POT's defaults (stopThr 1e-9, check every 10): the error of the check before the last lies below
    `precise_below`, so the device finishes in fp64 exps and must stop where the oracle stops."""
    ot = _ot()
    uo, vo, it_o, err_o, err_before = _oracle_conv(B0, B1, 2.0, 1e-9)
    # on the oracle alone: the two checks straddle the threshold by a factor of 4 on each side, and the earlier one
    # already engages the precise phase
    assert it_o == 21
    assert err_before >= 4e-9 and err_o <= 1e-9 / 4, (err_before, err_o)
    assert err_before < 1e-4 / np.sqrt(B1)
    r = ot.sinkhorn_log(_to_dev(_cloud_cost(B0, B1), dev, mis), 2.0)
    u, v = _potentials(r, B0, B1, dev)
    du, dv = float(np.abs(u - uo).max()), float(np.abs(v - vo).max())
    print(f"converge {B0}x{B1}: iters {int(r.iters.cpu())} err {float(r.err.cpu()):.3e} (oracle {err_before:.3e} -> "
          f"{err_o:.3e}) max|du| {du:.3e} max|dv| {dv:.3e}")
    assert int(r.iters.cpu()) == it_o
    assert float(r.err.cpu()) < 1e-9
    assert du < 1e-6 and dv < 1e-6, (du, dv)
    assert _precise_word(r) == 1


# ------------------------------------------------------------------------------------------- (d) fp32 early stop
@pytest.mark.parametrize("B0,B1,mis", CONV_SHAPES, ids=_conv_ids)
def test_early_stop_in_the_fp32_regime(dev, B0, B1, mis):
    ot = _ot()
    uo, vo, it_o, err_o, err_before = _oracle_conv(B0, B1, 2.0, 1e-4)
    assert it_o == 11 and err_before >= 4e-4 and err_o <= 1e-4 / 4, (err_before, err_o)
    r = ot.sinkhorn_log(_to_dev(_cloud_cost(B0, B1), dev, mis), 2.0, stop_thr=1e-4)
    assert int(r.iters.cpu()) == it_o
    assert _precise_word(r) == 0             # stop_thr >= precise_below: the fp64 phase is never engaged
    du, dv, sc = _dev_uv(*_potentials(r, B0, B1, dev), uo, vo)
    assert du <= 1e-5 * sc and dv <= 1e-5 * sc, (du, dv, sc)


# ------------------------------------------------------------------------------------------- (e) check bookkeeping
@pytest.mark.parametrize("max_iter,check_every", [(1, 10), (2, 10), (10, 10), (11, 10), (12, 10), (7, 3), (4, 1)])
@pytest.mark.parametrize("B0,B1", [(13, 1024), (33, 1027)])
def test_check_bookkeeping(dev, B0, B1, max_iter, check_every):
    """iters == max_iter, last_err == the oracle's last checked error: the trailing column pass measures the check of
    the last iteration (the `pending` slot of sk_finish) when (max_iter - 1) % check_every == 0."""
    ot = _ot()
    uo, vo, it_o, err_o = _oracle_fixed(B0, B1, 0.1, max_iter, check_every)
    r = ot.sinkhorn_log(_to_dev(_cloud_cost(B0, B1), dev), 0.1, max_iter=max_iter, stop_thr=0.0, check_every=check_every)
    assert int(r.iters.cpu()) == max_iter == it_o
    assert float(r.err.cpu()) == pytest.approx(err_o, rel=1e-3, abs=1e-12)
    du, dv, sc = _dev_uv(*_potentials(r, B0, B1, dev), uo, vo)
    assert du <= 1e-5 * sc and dv <= 1e-5 * sc, (du, dv, sc)


# ------------------------------------------------------------------------------------------- (f) one-shot fast row pass
ONESHOT_SHAPES = [(1, 1024), (13, 1024), (5, 5120), (5, 16384)]      # 5120: two 4096-column segments per row


def _oneshot_child():
    """Runs in a fresh interpreter with CFM_SK_STREAM=0: the streaming row pass is off, every shape below takes
    sk_row_pass<true>.  Prints one JSON line of deviations."""
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    dev_ = _lib.require_gpu()
    out = {}
    for B0, B1 in ONESHOT_SHAPES:
        s = _dispatch(B0, B1, True)
        ok, (du, dv, sc) = _run_sentinel(B0, B1, False, dev_)
        okr, rowsent = (True, (0.0, 0.0, 1.0)) if B0 < 2 else _run_sentinel(B0, B1, False, dev_, _row_sentinel_cases)
        out[f"{B0}x{B1}"] = dict(row_fast=int(s["row_fast"]), sentinel_ok=bool(ok), sentinel=(du, dv, sc),
                                 row_sentinel_ok=bool(okr), row_sentinel=rowsent, random=_run_random(B0, B1, False, dev_))
    print("ONESHOT " + json.dumps(out))


def test_oneshot_fast_row_pass_in_a_child_process(dev):
    env = dict(os.environ, CFM_SK_STREAM="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "oneshot"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("ONESHOT ")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0][len("ONESHOT "):])
    print(out)
    assert sorted(out) == sorted(f"{b0}x{b1}" for b0, b1 in ONESHOT_SHAPES)
    for key, o in out.items():
        assert o["row_fast"] == 1, key
        du, dv, sc = o["sentinel"]
        assert o["sentinel_ok"] and du <= 1e-5 * sc and dv <= 1e-5 * sc, (key, o["sentinel"])
        du, dv, sc = o["row_sentinel"]
        assert o["row_sentinel_ok"] and du <= 1e-5 * sc and dv <= 1e-5 * sc, (key, o["row_sentinel"])
        _assert_random(o["random"])


# ------------------------------------------------------------------------------------------- (g) consumers
def _cdf_margin(cdf, u, idx):
    """Distance of every u to the nearest step of the (normalised, non-decreasing) cdf."""
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], -np.inf)
    hi = cdf[np.minimum(idx, len(cdf) - 1)]
    return float(np.minimum(u - lo, hi - u).min())


def _flat_reference(P, u):
    p = P.flatten()
    p = p / p.sum()
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    idx = cdf.searchsorted(u, side="right")
    i, j = oracle.sample_map_given_u(P, u)
    assert np.array_equal(i * P.shape[1] + j, idx)
    return i, j, _cdf_margin(cdf, u, idx)


def _rows_reference(P, rows, u):
    """np.random.choice(B1, p=pi[i] / pi[i].sum()) per row, given its uniform."""
    out, margin = np.empty(len(rows), dtype=np.int64), np.inf
    for k, (i, uu) in enumerate(zip(rows, u)):
        p = P[i] / P[i].sum()
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        out[k] = cdf.searchsorted(uu, side="right")
        margin = min(margin, _cdf_margin(cdf, np.array([uu]), out[k:k + 1]))
    return out, margin


def _rows_with_ends(B0, n, rng, allowed=None):
    allowed = np.arange(B0) if allowed is None else np.asarray(allowed)
    rows = allowed[rng.integers(0, len(allowed), n)]
    rows[0], rows[-1] = allowed[0], allowed[-1]
    return rows.astype(np.int64)


@pytest.mark.parametrize("B0,B1", [(2055, 1024), (6, 16390), (33, 16388), (1, 5), (5, 1)])
def test_consumers_on_the_solved_state(dev, B0, B1):
    """Plan, <pi, M> and the two dense samplers on the potentials of a solve (reg 0.5, 30 iterations).  reg = 0.5
    keeps every exponent of the plan above -150: at |x| <= 150 the two evaluation orders of u + v - M / reg differ
    by a few 1e-14, inside rtol = 1e-12, and no entry is subnormal."""
    from cfm_amd import _lib
    ot = _ot()
    lib = _lib.load()
    reg = 0.5
    Mnp = _cloud_cost(B0, B1)
    M = _to_dev(Mnp, dev)
    r = ot.sinkhorn_log(M, reg, max_iter=30, stop_thr=0.0)
    u, v = _potentials(r, B0, B1, dev)
    P = oracle.sinkhorn_plan(Mnp, reg, u, v)
    np.testing.assert_allclose(ot.sinkhorn_plan(r).cpu().numpy(), P, rtol=1e-12, atol=0.0)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    _lib.check(lib.cfm_sinkhorn_cost_f64(_lib.ptr(M), B0, B1, reg, _lib.ptr(r.ws), _lib.ptr(out), _lib.stream_ptr()), "cost")
    assert float(out.cpu()) == pytest.approx(float((P * Mnp.astype(np.float64)).sum()), rel=1e-6)
    rng = np.random.default_rng(1)
    uu = rng.random(512)
    i_ref, j_ref, margin = _flat_reference(P, uu)
    assert margin >= 1e-12, margin                       # on the oracle alone: no draw sits on a cdf step
    i, j = ot.sample_dense(r, ot._u01_to_device(uu, dev))
    assert np.array_equal(i.cpu().numpy(), i_ref) and np.array_equal(j.cpu().numpy(), j_ref)
    rows = _rows_with_ends(B0, 512, rng)
    ur = rng.random(512)
    jr_ref, margin = _rows_reference(P, rows, ur)
    assert margin >= 1e-12, margin
    jr = ot.sample_rows_dense(r, torch.from_numpy(rows).to(dev), ot._u01_to_device(ur, dev))
    assert np.array_equal(jr.cpu().numpy(), jr_ref)


@pytest.mark.parametrize("B0,B1", [(2055, 5), (3, 16390)])
def test_explicit_plan_samplers_with_zero_rows_and_leading_columns(dev, B0, B1):
    ot = _ot()
    rng = np.random.default_rng(2)
    P = rng.random((B0, B1))
    zero_rows = [1] if B0 == 3 else [1, 1023, 1024, 2053]
    P[zero_rows] = 0.0
    P[:, :(2 if B1 == 5 else 300)] = 0.0              # zero leading columns: lane segments without mass
    P /= P.sum()
    pi = torch.from_numpy(P).to(dev)
    uu = rng.random(512)
    i_ref, j_ref, margin = _flat_reference(P, uu)
    assert margin >= 1e-12, margin
    i, j = ot.sample_pi(pi, ot._u01_to_device(uu, dev))
    assert np.array_equal(i.cpu().numpy(), i_ref) and np.array_equal(j.cpu().numpy(), j_ref)
    rows = _rows_with_ends(B0, 512, rng, allowed=[q for q in range(B0) if q not in zero_rows])
    assert rows[0] == 0 and rows[-1] == B0 - 1
    ur = rng.random(512)
    jr_ref, margin = _rows_reference(P, rows, ur)
    assert margin >= 1e-12, margin
    jr = ot.sample_rows_pi(pi, torch.from_numpy(rows).to(dev), ot._u01_to_device(ur, dev))
    assert np.array_equal(jr.cpu().numpy(), jr_ref)


# ------------------------------------------------------------------------------------------- (h) points variant
# (B0, B1, d): d = 4, 5 long trips (8 points per lane and trip), d = 6, 7 the short trips d = 8 is tested with;
# the others reach the second staged chunk (stage_cap = 3072 at d = 8, 4096 at d = 6, 8192 at d = 2)
PTS_SHAPES = [(130, 77, 4), (130, 77, 5), (130, 77, 6), (130, 77, 7), (40, 3072, 8), (40, 3073, 8), (3100, 40, 8),
              (40, 3100, 8), (20, 4100, 6), (24, 8200, 2)]
PTS_CHUNKS = {(130, 77, 4): (512, 1, 1), (130, 77, 5): (512, 1, 1), (130, 77, 6): (512, 1, 1), (130, 77, 7): (512, 1, 1),
              (40, 3072, 8): (3072, 1, 1), (40, 3073, 8): (3072, 1, 2), (3100, 40, 8): (3072, 2, 1),
              (40, 3100, 8): (3072, 1, 2), (20, 4100, 6): (4096, 1, 2), (24, 8200, 2): (8192, 1, 2)}
# (c) per trip family: d = 2 (long trips, two staged chunks), d = 6 / 7 / 8 (short trips; 40 x 3073 and 3100 x 40 with a
# second chunk on either side).  At d = 4 and 5 the oracle's checks do not straddle 1e-9 by the factor of 4 asked for.
PTS_CONV = [(24, 8200, 2), (130, 77, 6), (130, 77, 7), (40, 3073, 8), (3100, 40, 8)]


def _direct_cost(a, b):
    """The scratch-free cost entry point (always the direct-difference kernels): the matrix whose entries the points
    variant recomputes bit for bit."""
    from cfm_amd import _lib
    M = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().cfm_sqeuclid_cost_f32(_lib.ptr(a), _lib.ptr(b), a.shape[0], b.shape[0], a.shape[1],
                                                 _lib.ptr(M), None, _lib.stream_ptr()), "cfm_sqeuclid_cost_f32")
    return M


@pytest.mark.parametrize("B0,B1,d", PTS_SHAPES)
def test_points_variant_helper_and_random_clouds(dev, B0, B1, d):
    ot = _ot()
    s = _pts_dispatch(B0, B1, d)
    assert (s["stage_cap"], s["chunks_x0"], s["chunks_x1"]) == PTS_CHUNKS[(B0, B1, d)]
    assert (s["trip_u"], s["pre"]) == ((8, 4) if d <= 5 else (4, 2))
    x0, x1 = _clouds(B0, B1, d)
    a, b = torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev)
    M = _direct_cost(a, b)
    reg = 0.1
    r = ot.sinkhorn_log_points(a, b, M, reg, max_iter=30, stop_thr=0.0)
    uo, vo, _, _ = oracle.sinkhorn_log(M.cpu().numpy(), reg, numItermax=30, stopThr=0.0)
    du, dv, sc = _dev_uv(*_potentials(r, B0, B1, dev), uo, vo)
    print(f"points random {B0}x{B1} d={d}: max|du| {du:.3e} max|dv| {dv:.3e} scale {sc:.3f}")
    assert int(r.iters.cpu()) == 30
    assert du <= 1e-5 * sc and dv <= 1e-5 * sc, (du, dv, sc)
    f, g = r.f.cpu().numpy(), r.g.cpu().numpy()
    assert np.abs(f - reg * uo).max() <= 1e-5 * reg * sc and np.abs(g - reg * vo).max() <= 1e-5 * reg * sc


@pytest.mark.parametrize("B0,B1,d", PTS_CONV)
def test_points_variant_convergence_through_the_fp64_regime(dev, B0, B1, d):
    ot = _ot()
    x0, x1 = _clouds(B0, B1, d)
    a, b = torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev)
    M = _direct_cost(a, b)
    Mnp = M.cpu().numpy()
    reg = 2.0
    uo, vo, it_o, err_o = oracle.sinkhorn_log(Mnp, reg)
    assert 11 < it_o < 1000
    _, _, _, err_before = oracle.sinkhorn_log(Mnp, reg, numItermax=it_o - 10, stopThr=0.0)
    assert err_before >= 4e-9 and err_o <= 1e-9 / 4, (err_before, err_o)
    assert err_before < 1e-4 / np.sqrt(B1)
    r = ot.sinkhorn_log_points(a, b, M, reg)
    u, v = _potentials(r, B0, B1, dev)
    du, dv = float(np.abs(u - uo).max()), float(np.abs(v - vo).max())
    print(f"points converge {B0}x{B1} d={d}: iters {int(r.iters.cpu())} ({it_o}) err {float(r.err.cpu()):.3e} "
          f"(oracle {err_before:.3e} -> {err_o:.3e}) max|du| {du:.3e} max|dv| {dv:.3e}")
    assert int(r.iters.cpu()) == it_o
    assert float(r.err.cpu()) < 1e-9
    assert du < 1e-6 and dv < 1e-6, (du, dv)
    assert _precise_word(r) == 1


def _pts_sentinel_clouds(B0, B1, d, cap):
    """Coordinate-built sentinel.  The smaller cloud's points sit on sites 5 apart along the first axis (squared
    distance >= 25 = 50 reg between any two sites, small offsets on the other axes); every point of the larger cloud
    is an exact copy of one site, so it has exactly ONE near neighbour (cost 0) on the other side.  The points of the
    larger cloud at the staging edges (0, cap - 1, cap, last) each own a site of their own: in the update of that
    site's potential the edge point is the only near term, so losing it in the staging moves the potential by ~50.
    (A one-to-one near pairing of ALL points on both sides needs B0 == B1; the remaining sites share the other points
    of the larger cloud, n_large / n_small each.)"""
    n_large, n_small = max(B0, B1), min(B0, B1)
    edges = sorted({e for e in (0, cap - 1, cap, n_large - 1) if 0 <= e < n_large})
    assert n_small > len(edges) + 1
    rng = np.random.default_rng(3)
    sites = 0.25 * rng.standard_normal((n_small, d))
    sites[:, 0] = 5.0 * rng.permutation(n_small)
    sites = sites.astype(np.float32)
    owner = np.empty(n_large, dtype=np.int64)
    rest = [t for t in range(n_large) if t not in edges]
    owner[edges] = np.arange(len(edges))
    owner[rest] = len(edges) + np.arange(len(rest)) % (n_small - len(edges))
    large = sites[owner]
    return (sites, large) if B0 <= B1 else (large, sites)


@pytest.mark.parametrize("B0,B1,d", PTS_SHAPES)
def test_points_variant_sentinel(dev, B0, B1, d):
    ot = _ot()
    cap = _pts_dispatch(B0, B1, d)["stage_cap"]
    x0, x1 = _pts_sentinel_clouds(B0, B1, d, cap)
    a, b = torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev)
    M = _direct_cost(a, b)
    Mnp = M.cpu().numpy()
    # the construction, on the matrix the kernels see: one exact zero per point of the larger cloud, everything else
    # at least 40 reg away
    near = Mnp == 0.0
    assert (near.sum(0 if B0 <= B1 else 1) == 1).all() and (near.sum(1 if B0 <= B1 else 0) >= 1).all()
    assert Mnp[~near].min() >= 40 * REG_SENT
    r = ot.sinkhorn_log_points(a, b, M, REG_SENT, max_iter=2, stop_thr=0.0)
    uo, vo, _, _ = oracle.sinkhorn_log(Mnp, REG_SENT, numItermax=2, stopThr=0.0)
    du, dv, sc = _dev_uv(*_potentials(r, B0, B1, dev), uo, vo)
    print(f"points sentinel {B0}x{B1} d={d}: max|du| {du:.3e} max|dv| {dv:.3e} scale {sc:.3f}")
    assert int(r.iters.cpu()) == 2
    assert du <= 1e-5 * sc and dv <= 1e-5 * sc, (du, dv, sc)


# ------------------------------------------------------------------------------------------- (i) unbalanced / partial
@pytest.mark.parametrize("B0,B1", [(33, 1027), (5, 300), (2055, 70), (1, 7), (7, 1)])
def test_unbalanced_and_partial_strips(dev, B0, B1):
    """The same strip logic (sk_nchunk) at two strips, one strip, 64 strips with an empty last one, one row / column."""
    ot = _ot()
    Mnp = _cloud_cost(B0, B1)
    M = _to_dev(Mnp, dev)
    plan, info = ot.unbalanced_plan(M, 1.0, 1.0)
    ref, log = oracle.sinkhorn_knopp_unbalanced(Mnp, 1.0, 1.0, log=True)
    p = plan.cpu().numpy()
    print(f"unbalanced {B0}x{B1}: oracle iters {log['iters']} status {log['status']} err {log['err']:.3e}; "
          f"deviation {np.abs(p - ref).max() / np.abs(ref).max():.3e}")
    assert log["status"] == 0 and log["iters"] in (11, 21)
    assert np.abs(p - ref).max() <= RTOL * np.abs(ref).max()
    assert info.tolist()[:2] == [log["iters"], log["status"]]
    plan, info = ot.partial_plan(M, 1.0, max_iter=60)
    ref, log = oracle.entropic_partial_wasserstein(Mnp, 1.0, numItermax=60, log=True)
    p = plan.cpu().numpy()
    print(f"partial {B0}x{B1}: oracle iters {log['iters']} status {log['status']}; "
          f"deviation {np.abs(p - ref).max() / np.abs(ref).max():.3e}")
    assert log["status"] == 0
    assert np.abs(p - ref).max() <= RTOL * np.abs(ref).max()
    assert info.tolist()[:2] == [log["iters"], log["status"]]


if __name__ == "__main__":
    assert sys.argv[1:] == ["oneshot"] and os.environ.get("CFM_SK_STREAM") == "0"
    _oneshot_child()
