"""Tolerance-free tests of the MLP backward chain (csrc/mlp_train.hip on csrc/gemm_core.h) and of the two-net kernels of
the SF2M step, through the C ABI — the conventions of test_gpu_gemm_exact.py: small-integer inputs, the premise (every
product and partial sum an integer below 2^24, times a power of two where a loss seed scales it) asserted on the host for
each test's own data, an int64 matmul as the reference, `torch.equal`, and every output buffer AND the whole workspace
NaN before the call, so that a split-K partial which the reduction reads and no workgroup wrote shows.

  1. split-K edges of the weight gradient: every split count 1 .. 32, a ragged last split, EMPTY trailing splits (whose
     workgroups must still write zero partials and zero column sums), also through the weighted column sum of a time column
  2. dgrad + wgrad in one launch (gemm_pair_f32_mfma) and the SELU' epilogue: two layers with caller-made pre-activations
     in {+1, -200}, where selu'(z) is exactly SELU_SCALE or exactly 0; selu_grad itself at its edges against float64
  3. the two-net kernels of cfm_mlp_sf2m_step_f32, also when one net's operands are off the 16-byte grid (one launch per
     net, on the one-net kernels)
  4. nets deeper than the split-K pool of the workspace holds at once (it is reduced and reused)
  5. the regression step's unfused loss (mse_grad behind a last layer of more workgroups than loss partials)

Which kernel a case reaches follows from the launch rules restated in exact_util.py; each case asserts it."""
import ctypes
import math

import numpy as np
import pytest
import torch

from exact_util import (LIMIT, LOSS_PARTIALS, SELU_ALPHA, SELU_SCALE, _arr, _first_diff, _ints, _layer_data, _nan, _nan_ws,
                        lpart_offset, pair_ok, pick_tile, pool_refills, split_ranges, vec_ok, wgrad_splits)
from exact_util import lib_ as _lib_

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _mm(a, b):
    """the int64 reference product (every exact reference of this file goes through _mm / _colsum)"""
    assert a.dtype == torch.int64 and b.dtype == torch.int64
    return a @ b


def _colsum(a):
    assert a.dtype == torch.int64
    return a.sum(0)


def _exact(got, ref, *what):
    """ref: float64 on the host, exactly representable in fp32 (asserted)"""
    refd = ref.float().to(got.device)
    assert torch.equal(refd.cpu().double(), ref.double()), (*what, "premise: the reference is an fp32 number")
    assert torch.equal(got, refd), (*what, _first_diff(got, refd))


def _ws_bytes(lib, _lib, B, dims):
    n = len(dims) - 1
    return lib.cfm_workspace_bytes(_lib.OP_MLP_TRAIN, B, max(dims), max(dims[l] * dims[l + 1] for l in range(n)))


def _backward(acts, preact, W, dims, B, dout, dW, db, dx, ws):
    _lib, lib = _lib_()
    n = len(dims) - 1
    cd = (ctypes.c_int * (n + 1))(*dims)
    _lib.check(lib.cfm_mlp_backward_f32(_arr(acts), _arr(preact), _arr(W), cd, n, B, _lib.ptr(dout), _arr(dW), _arr(db),
                                        _lib.ptr(dx), _lib.ptr(ws), _lib.stream_ptr()), "cfm_mlp_backward_f32")
    torch.cuda.synchronize()


def _regression_step(xt, t, ut, W, b, dims, B, hidden, preact, g, dW, db, loss, ws, events=None):
    _lib, lib = _lib_()
    n = len(dims) - 1
    cd = (ctypes.c_int * (n + 1))(*dims)
    _lib.check(lib.cfm_mlp_regression_step_f32(_lib.ptr(xt), _lib.ptr(t), _lib.ptr(ut), _arr(W), _arr(b), cd, n, B,
                                               _arr(hidden) if hidden else None, _arr(preact) if preact else None,
                                               _lib.ptr(g), _arr(dW), _arr(db), _lib.ptr(loss), events, _lib.ptr(ws),
                                               _lib.stream_ptr()), "cfm_mlp_regression_step_f32")
    torch.cuda.synchronize()


def _sf2m_step(xt, t, ut, eps, lam, W, b, hidden, preact, dW, db, dims, B, gf, gs, losses, score_weight, ws):
    _lib, lib = _lib_()
    n = len(dims) - 1
    cd = (ctypes.c_int * (n + 1))(*dims)
    _lib.check(lib.cfm_mlp_sf2m_step_f32(_lib.ptr(xt), _lib.ptr(t), _lib.ptr(ut), _lib.ptr(eps), _lib.ptr(lam), _arr(W), _arr(b),
                                         _arr(hidden) if hidden else None, _arr(preact) if preact else None, _arr(dW), _arr(db),
                                         cd, n, B, _lib.ptr(gf), _lib.ptr(gs), _lib.ptr(losses), score_weight, _lib.ptr(ws),
                                         _lib.stream_ptr()), "cfm_mlp_sf2m_step_f32")
    torch.cuda.synchronize()


def _off_grid(t, floats):
    """a copy of t that starts `floats` floats past a 16-byte boundary (a view into a larger allocation)"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * floats
    return v


# ------------------------------------------------------------------ 1. split-K edges of the weight gradient ----
# (B, K, N, the split count the case is meant to reach, its edge).  The first six: one shape per split count.  "ragged":
# the last split is shorter than the others and no multiple of the 32-deep K step; "empty": trailing splits with
# k_begin >= B (B = 2049 at S = 32: k_chunk = 96, splits 22 .. 31).
SPLIT_CASES = [(127, 16, 16, 1, None), (128, 32, 48, 2, None), (256, 64, 64, 4, None), (512, 20, 33, 8, None),
               (1024, 48, 16, 16, None), (2048, 16, 64, 32, None),
               (130, 20, 65, 2, "ragged"), (2047, 16, 16, 16, "ragged"), (2049, 16, 16, 32, "empty"), (2049, 48, 33, 32, "empty")]


def _split_premise(B, K, N, S, edge):
    assert wgrad_splits(N, K, B) == S, ("premise: the split count", wgrad_splits(N, K, B))
    assert pick_tile(N, K, S) == 2
    r = split_ranges(B, S)
    empty = [s for s, (a, b) in enumerate(r) if a >= b]
    full = [(a, b) for a, b in r if a < b]
    assert full[0][0] == 0 and full[-1][1] == B and all(p[1] == q[0] for p, q in zip(full, full[1:]))
    if edge == "empty":
        assert empty and all(r[s][0] >= B for s in empty) and empty[-1] == S - 1, "premise: empty trailing splits"
    else:
        assert not empty
    if edge == "ragged":
        assert S > 1 and (full[-1][1] - full[-1][0]) % 32 != 0 and full[-1][1] - full[-1][0] < full[0][1], "premise: a ragged last split"


@pytest.mark.parametrize("B,K,N,S,edge", SPLIT_CASES)
def test_wgrad_split_edges_are_exact(dev, B, K, N, S, edge):
    """cfm_mlp_backward_f32 with one layer: dW = dout^T x and db = sum dout over S batch splits, dx = dout W.  Values in
    {-2 .. 2}; outputs and workspace NaN.  gemm_f32_mfma<64, 64, 32, A_KMAJOR, B_KMAJOR, EPI_PLAIN> with 16-byte loads
    where N % 4 == 0 (dout) / K % 4 == 0 (x), grid y = S, then reduce_splits_multi over all S partials."""
    _split_premise(B, K, N, S, edge)
    g = torch.Generator().manual_seed(B * 7 + K + N)
    x, w, dout = _ints(g, (B, K), -2, 2), _ints(g, (N, K), -2, 2), _ints(g, (B, N), -2, 2)
    dW, db, dx = _mm(dout.T, x), _colsum(dout), _mm(dout, w)
    assert int((dout.abs().T @ x.abs()).max()) < LIMIT and int(dout.abs().sum(0).max()) < LIMIT
    assert int((dout.abs() @ w.abs()).max()) < LIMIT
    _lib, lib = _lib_()
    xd, wd, dd = x.float().to(dev), w.float().to(dev), dout.float().to(dev)
    dWd, dbd, dxd = _nan((N, K), dev), _nan((N,), dev), _nan((B, K), dev)
    ws = _nan_ws(_ws_bytes(lib, _lib, B, [K, N]), dev)
    _backward([xd], [None], [wd], [K, N], B, dd, [dWd], [dbd], dxd, ws)
    for name, got, ref in (("dW", dWd, dW), ("db", dbd, db), ("dx", dxd, dx)):
        _exact(got, ref.double(), name)


@pytest.mark.parametrize("B,K,N,S,edge", [c for c in SPLIT_CASES if c[4]])
def test_time_column_sum_split_edges_are_exact(dev, B, K, N, S, edge):
    """cfm_mlp_regression_step_f32 with one layer and a time column at the edge shapes: the time weight's gradient is the
    weighted column sum sum_b g[b, :] t[b] of the wgrad workgroups (tvec / tsum), whose guard `k0 + kk < k_end` is the
    ragged-split code.  n = B N is no power of two here, so 2 / n does not scale exactly; instead ut = v + e m with the
    INTEGER m = the odd part of n: g = fl(-e m fl(2 / n)) is then -e times a power of two (asserted on the host with
    the float32 arithmetic of the call), and dW, db and the time column are integers times that power.  The loss
    ((e m)^2 summed) is not exact and only has to be finite.  gemm_f32_mfma<64, 64, 32, true, true, EPI_PLAIN> with
    tvec, one net, unpaired, S splits."""
    _split_premise(B, K, N, S, edge)
    x, w, b, t, v = _layer_data(B, K, N, "row", seed=B + K + N, lo=-2, hi=2)
    n = B * N
    m = n
    while m % 2 == 0:
        m //= 2
    scale = np.float32(2) * (np.float32(1) / np.float32(n))                # 2.0f * (1.0f / (float)n)
    seed = float(np.float32(m) * scale)
    assert math.frexp(seed)[0] == 0.5, ("premise: the loss seed of |e| = 1 is a power of two", seed)
    e = _ints(torch.Generator().manual_seed(5), (B, N), -1, 1)
    ut = v + e * m
    assert int(ut.abs().max()) < LIMIT and int(v.abs().max()) < LIMIT
    xin = torch.cat([x, t.reshape(B, 1)], 1)
    assert int((e.abs().T @ xin.abs()).max()) < LIMIT
    g_ref = (-e).double() * seed
    dW_ref = _mm((-e).T, xin).double() * seed
    db_ref = _colsum(-e).double() * seed
    _lib, lib = _lib_()
    xd, wd, bd, utd, td = (q.float().to(dev) for q in (x, w, b, ut, t))
    gd, dWd, dbd, loss = _nan((B, N), dev), _nan((N, K + 1), dev), _nan((N,), dev), _nan((1,), dev)
    ws = _nan_ws(_ws_bytes(lib, _lib, B, [K + 1, N]), dev)
    _regression_step(xd, td, utd, [wd], [bd], [K + 1, N], B, None, None, gd, [dWd], [dbd], loss, ws)
    _exact(gd, g_ref, "g")
    _exact(dWd[:, :K].contiguous(), dW_ref[:, :K], "dW")
    _exact(dWd[:, K].contiguous(), dW_ref[:, K], "dW[:, time]")
    _exact(dbd, db_ref, "db")
    assert bool(torch.isfinite(loss).all())


# ------------------------------------------------- 2. the paired launch and the SELU' epilogue (two layers) ----
def _two_layer_data(B, H, N, seed, z=None, dout=None, W1=None):
    """dims = [K0 = B, H, N] with caller-made activations: acts[0] = I_B, so that dW[0][:, b] = dz0[b, :] shows the
    dgrad's output through a public one (a sum with zeros: exact); W[0] with at most one +-1 per column, so that
    dx = dz0 W[0] is one term; preact[1] in {+1, -200}: selu' is exactly SELU_SCALE (as fp32) or exactly 0
    (expf(-200) underflows).  Returns the int64 / fp32 inputs and the references."""
    g = torch.Generator().manual_seed(seed)
    h = _ints(g, (B, H), -2, 2)
    W1 = _ints(g, (N, H), -2, 2) if W1 is None else W1
    dout = _ints(g, (B, N), -2, 2) if dout is None else dout
    W0 = torch.zeros((H, B), dtype=torch.int64)
    rows, sign = _ints(g, (B,), 0, H - 1), _ints(g, (B,), -1, 1)          # (sign 0: a column of zeros)
    W0[rows, torch.arange(B)] = sign
    assert int((W0 != 0).sum(0).max()) <= 1
    if z is None:
        z = torch.where(_ints(g, (B, H), 0, 1) == 1, 1.0, -200.0).float()
    a = _mm(dout, W1)                                                      # [B, H] integers
    assert int(_absmm(dout, W1).max()) < LIMIT and int(_absmm(dout.T, h).max()) < LIMIT and int(dout.abs().sum(0).max()) < LIMIT
    sg = torch.where(z > 0, torch.tensor(SELU_SCALE, dtype=torch.float32), torch.tensor(0.0))
    dz0 = a.float() * sg                                                   # ONE fp32 rounding, as the epilogue's
    ref = {"dW1": _mm(dout.T, h).double(), "db1": _colsum(dout).double(), "dz0": dz0,
           "dx": (dz0.double() @ W0.double())}                             # (one nonzero term per element: exact)
    return h, W1, dout, W0, z, ref


def _absmm(a, b):
    return a.abs() @ b.abs()


def _run_two_layer(dev, B, H, N, h, W1, dout, W0, z):
    _lib, lib = _lib_()
    dims = [B, H, N]
    x0 = torch.eye(B, dtype=torch.float32, device=dev)
    hd, W1d, W0d, dd, zd = (q.float().to(dev) for q in (h, W1, W0, dout, z))
    out = {"dW0": _nan((H, B), dev), "db0": _nan((H,), dev), "dW1": _nan((N, H), dev), "db1": _nan((N,), dev),
           "dx": _nan((B, B), dev)}
    ws = _nan_ws(_ws_bytes(lib, _lib, B, dims), dev)
    S1 = wgrad_splits(N, H, B)
    paired = pair_ok(B, H, N, S1, dd, hd, W1d)
    _backward([x0, hd], [None, zd], [W0d, W1d], dims, B, dd, [out["dW0"], out["dW1"]], [out["db0"], out["db1"]], out["dx"], ws)
    return out, paired, S1


# (B = K0, H, N, paired?, S of the second layer or None): paired = gemm_pair_f32_mfma (64 x 64 x 32, VECA = VECB = true, the
# float2 SELU' epilogue); unpaired = gemm_f32_mfma<64, 64, 32, false, true, EPI_SELU_GRAD, N % 4 == 0, H % 4 == 0> behind
# the wgrad launch: (130, 33, 7) and (65, 65, 1) with odd ldc (the scalar epilogue, the column guard), (128, 64, 6) with
# 16-byte loads of W only and the float2 epilogue
TWO_LAYER_CASES = [(64, 64, 64, True, None), (130, 80, 48, True, None), (257, 512, 16, True, None), (130, 33, 7, False, None),
                   (65, 65, 1, False, None), (128, 64, 6, False, None), (512, 64, 64, True, 8)]


@pytest.mark.parametrize("B,H,N,want_pair,want_S", TWO_LAYER_CASES)
def test_two_layer_backward_is_exact(dev, B, H, N, want_pair, want_S):
    """cfm_mlp_backward_f32 with two layers on the data of _two_layer_data: dW[1], db[1] exact integers, dz0 (seen as
    dW[0]^T) and dx exact single roundings, db[0] (a genuine fp32 sum of non-integers) within B 2^-24 sum_b |dz0[b, n]|
    of its float64 value."""
    h, W1, dout, W0, z, ref = _two_layer_data(B, H, N, seed=B + H + N)
    out, paired, S1 = _run_two_layer(dev, B, H, N, h, W1, dout, W0, z)
    assert paired == want_pair, "premise: the pairing condition of mlp_backward_impl"
    assert want_S is None or S1 == want_S, ("premise: split-K in the paired launch", S1)
    _exact(out["dW1"], ref["dW1"], "dW[1]")
    _exact(out["db1"], ref["db1"], "db[1]")
    _exact(out["dW0"].T.contiguous(), ref["dz0"].double(), "dz0 = dW[0]^T")
    _exact(out["dx"], ref["dx"], "dx")
    dz0 = ref["dz0"].double()
    err = (out["db0"].cpu().double() - dz0.sum(0)).abs()
    bound = B * 2.0 ** -24 * dz0.abs().sum(0)
    print(f"db[0]: max error {float(err.max()):.3e}, smallest slack {float((bound - err).min()):.3e}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))


def test_paired_dgrad_index_encoding_names_the_element_that_landed(dev):
    """dout[b, n] = b N + n and W[1][n, k] = (k // N + 1) [n == k mod N], every pre-activation +1:
    dz0[b, k] = fl((b N + k mod N)(k // N + 1) SELU_SCALE) names its own row and column; a wrong element is reported as
    the (row, n) that arrived instead (a swapped fragment or tile of the paired launch)."""
    B, H, N = 130, 80, 48
    b, n, k = torch.arange(B).reshape(B, 1), torch.arange(N).reshape(1, N), torch.arange(H)
    dout = b * N + n
    W1 = torch.zeros((N, H), dtype=torch.int64)
    W1[k % N, k] = k // N + 1
    z = torch.ones((B, H))
    h, W1, dout, W0, z, ref = _two_layer_data(B, H, N, seed=1, z=z, dout=dout, W1=W1)
    a = (b * N + (k % N).reshape(1, H)) * (k // N + 1).reshape(1, H)
    assert torch.equal(_mm(dout, W1), a) and int(a.max()) * 2 < LIMIT
    out, paired, _ = _run_two_layer(dev, B, H, N, h, W1, dout, W0, z)
    assert paired, "premise: gemm_pair_f32_mfma"
    got = out["dW0"].T.contiguous().cpu()
    if not torch.equal(got, ref["dz0"]):
        bad = (~(got == ref["dz0"])).nonzero()
        msgs = []
        for r, c in bad[:6].tolist():
            s, v = c // N + 1, float(got[r, c]) / SELU_SCALE
            q = round(v) if v == v else None
            src = divmod(q // s, N) if q is not None and abs(v - q) < 1e-3 and q % s == 0 else None
            msgs.append(f"dz0[{r},{c}] (n {c % N}, scale {s}) = {float(got[r, c])}: that is (row, n) = {src}")
        pytest.fail(f"{len(bad)} elements differ; " + "; ".join(msgs))


Z_EDGES = [0.0, -0.0, 1e-30, -1e-30, -1e-6, -1.0, -20.0, -87.3, -88.5, -103.0, -104.0, -200.0, 50.0]
# measured on the MI355X against float64, the larger of H = 64 and H = 33 (see the docstring below)
SELU_GRAD_REL_MEASURED = 1.077e-07
SELU_GRAD_ABS_MEASURED = 8.505e-44


@pytest.mark.parametrize("H", [64, 33])
def test_selu_grad_at_its_edges_against_float64(dev, H):
    """selu_grad at pre-activations random data never samples: each of Z_EDGES in every column position of a tile
    (H = 64: the float2 epilogue of the paired launch; H = 33: the scalar one), times an integer dout . W.  Per element
    against float64 scale (z > 0 ? 1 : alpha exp(z)) of the same float32 z.
    Measured (not guessed), the largest over both H:
      relative error where the reference is a normal fp32 number (>= 2^-126):  1.077e-07 (both H)
      absolute error where it is below 2^-126:                                 8.505e-44 (H = 64), 8.265e-44 (H = 33)
    (the second: z = -103 gives expf(z) = one subnormal step, 1.4e-45 for 1.85e-45, times alpha scale and an integer <= 96;
    the device keeps subnormals.)  The asserted bounds are four times these (headroom for another expf expansion of a
    later compiler), the relative one at most 1e-5, the project's fp32 bound."""
    B, N = 65, 16
    g = torch.Generator().manual_seed(H)
    dout, W1 = _ints(g, (B, N), 1, 3), _ints(g, (N, H), 1, 2)             # positive: no cancellation, every product nonzero
    zi = (torch.arange(B).reshape(B, 1) + torch.arange(H).reshape(1, H)) % len(Z_EDGES)
    z = torch.tensor(Z_EDGES, dtype=torch.float32)[zi]
    assert all(len(set(zi[:, c].tolist())) == len(Z_EDGES) for c in range(H)), "premise: every edge in every column"
    h, W1, dout, W0, z, ref = _two_layer_data(B, H, N, seed=H, z=z, dout=dout, W1=W1)
    out, paired, _ = _run_two_layer(dev, B, H, N, h, W1, dout, W0, z)
    assert paired == (H == 64)
    got = out["dW0"].T.contiguous().cpu().double()
    zz = z.double()
    want = _mm(dout, W1).double() * SELU_SCALE * torch.where(zz > 0, torch.ones_like(zz), SELU_ALPHA * torch.exp(zz))
    err = (got - want).abs()
    normal = want.abs() >= 2.0 ** -126
    rel = float((err[normal] / want[normal].abs()).max())
    sub = float(err[~normal].max())
    assert bool(normal.any()) and bool((~normal).any())
    print(f"selu_grad H = {H}: max relative error (normal references) {rel:.3e}, max absolute error (below 2^-126) {sub:.3e}")
    assert 4 * SELU_GRAD_REL_MEASURED <= 1e-5
    assert rel <= 4 * SELU_GRAD_REL_MEASURED, rel
    assert sub <= 4 * SELU_GRAD_ABS_MEASURED, sub


# ------------------------------------------------------------------------------ 3. the two-net kernels ----
def _lin(x, w, b, t):
    K = x.shape[1]
    v = _mm(x, w[:, :K].T.contiguous()) + b
    mag = x.abs() @ w[:, :K].abs().T + b.abs()
    if t is not None:
        v = v + t.reshape(-1, 1) * w[:, K].reshape(1, -1)
        mag = mag + t.abs().reshape(-1, 1) * w[:, K].abs().reshape(1, -1)
    assert int(mag.max()) < LIMIT
    return v


# (B, K, N, time) of test_mse_epilogue_is_exact; `off`: which operand sits off the 16-byte grid (None: all aligned).
# W one float off: plan_layer's VECB differs between the nets (K % 4 == 0 and no time column: the pitch is K), the forward
# takes one launch per net through the one-net form of launch_layer (mlp_layer_glds where K % 16 == 0, else mlp_layer; the
# score net's weighted loss layer, for which mlp_layer has no argument, mlp_layer_two on one net's grid: the K = 20 case).
# g two floats off (8 bytes: the epilogue's float2 stores stay aligned): gemm_vec_ok(dz) differs, launch_gemm runs the
# weight gradient once per net (gemm_f32_mfma).
SF2M_CASES = [(64, 48, 64, False, None), (256, 20, 16, True, None), (128, 64, 128, False, None), (1024, 512, 32, True, None),
              (64, 48, 64, False, "score_W"), (128, 64, 128, False, "flow_W"), (256, 20, 16, True, "score_g"),
              (1024, 512, 32, True, "flow_g"), (128, 64, 128, False, "score_g"), (256, 20, 16, False, "score_W"),
              (256, 20, 16, False, "flow_W")]


@pytest.mark.parametrize("score_weight", [1.0, 0.5])
@pytest.mark.parametrize("B,K,N,timed,off", SF2M_CASES)
def test_sf2m_one_layer_is_exact(dev, B, K, N, timed, off, score_weight):
    """cfm_mlp_sf2m_step_f32 with one layer, n = B N a power of two.  Flow half: ut = v + e, e in {-1, 0, 1}.  Score half:
    lam in {0, 1, 2} per row and eps = r - lam s with r in {-1, 0, 1}, so fma(lam, s, eps) = r.  Exact: both seeds
    (-(2 / n) e and (2 w / n) r lam), both losses (counts over n), every loss partial (an integer over n, one per output
    tile, summing to the count), dW and db of both nets (integers times a power of two).  Forward: mlp_layer_two or
    mlp_layer_glds_two (K % 16 == 0), 64 x 64 tiles; backward: gemm_f32_mfma_two<64, 64, 32, true, true, EPI_PLAIN>, S from
    wgrad_splits, the time column's weighted sum where timed.  A net off the 16-byte grid: the one-net kernels, once per net
    (see SF2M_CASES)."""
    n = B * N
    assert n & (n - 1) == 0
    x, wf, bf, t, vf = _layer_data(B, K, N, "row" if timed else None, seed=B + K + N)
    g = torch.Generator().manual_seed(11)
    wsc, bsc = _ints(g, wf.shape, -3, 3), _ints(g, (N,), -50, 50)
    vs = _lin(x, wsc, bsc, t)
    e, r, lam = _ints(g, (B, N), -1, 1), _ints(g, (B, N), -1, 1), _ints(g, (B,), 0, 2)
    ut, eps = vf + e, r - lam.reshape(B, 1) * vs
    assert int(ut.abs().max()) < LIMIT and int(eps.abs().max()) < LIMIT and int((lam.reshape(B, 1) * vs).abs().max()) < LIMIT
    xin = torch.cat([x, t.reshape(B, 1)], 1) if timed else x
    Kf = K + int(timed)
    sf, ss = -e, r * lam.reshape(B, 1)                                      # the seeds, in units of 2 / n and 2 w / n
    assert int(_absmm(sf.T, xin).max()) < LIMIT and int(_absmm(ss.T, xin).max()) < LIMIT
    cf, cs = 2.0 / n, 2.0 * score_weight / n
    want = {"g0": sf.double() * cf, "g1": ss.double() * cs, "dW0": _mm(sf.T, xin).double() * cf, "dW1": _mm(ss.T, xin).double() * cs,
            "db0": _colsum(sf).double() * cf, "db1": _colsum(ss).double() * cs}
    counts = [int(_colsum((e != 0).long()).sum()), int(_colsum((r != 0).long()).sum())]
    _lib, lib = _lib_()
    dims = [Kf, N]
    xd, utd, epsd, lamd = (q.float().to(dev) for q in (x, ut, eps, lam))
    td = t.float().to(dev) if timed else None
    Wd, bd = [wf.float().to(dev), wsc.float().to(dev)], [bf.float().to(dev), bsc.float().to(dev)]
    gd = [_nan((B, N), dev), _nan((B, N), dev)]
    which = {"score": 1, "flow": 0}[off.split("_")[0]] if off else None
    if off and off.endswith("_W"):
        Wd[which] = _off_grid(Wd[which], 1)
        plan_vb = [K % 4 == 0 and Kf % 4 == 0 and w.data_ptr() % 16 == 0 for w in Wd]
        assert plan_vb[0] != plan_vb[1], "premise: plan_layer differs between the nets"
    if off and off.endswith("_g"):
        gd[which] = _off_grid(gd[which], 2)
        assert vec_ok(gd[0], N, N) != vec_ok(gd[1], N, N), "premise: launch_gemm with unequal flags (one launch per net)"
    dWd, dbd, losses = [_nan((N, Kf), dev) for _ in range(2)], [_nan((N,), dev) for _ in range(2)], _nan((2,), dev)
    one = _ws_bytes(lib, _lib, B, dims)
    assert one % 256 == 0
    ws = _nan_ws(2 * one, dev)
    _sf2m_step(xd, td, utd, epsd, lamd, Wd, bd, None, None, dWd, dbd, dims, B, gd[0], gd[1], losses, score_weight, ws)
    for q in (0, 1):
        _exact(gd[q].contiguous(), want[f"g{q}"], off, q, "g")
        _exact(dWd[q], want[f"dW{q}"], off, q, "dW")
        _exact(dbd[q], want[f"db{q}"], off, q, "db")
        assert float(losses[q].cpu()) == counts[q] / n, (off, q, float(losses[q].cpu()), counts[q] / n)
        lo = q * (one // 4) + lpart_offset(B, dims)
        part = ws[lo:lo + LOSS_PARTIALS].cpu().double()
        part = part[~torch.isnan(part)] * n
        assert pick_tile(B, N, 1) == 2 and part.numel() == ((B + 63) // 64) * ((N + 63) // 64), (off, q, part.numel())
        assert torch.equal(part, part.round()) and int(part.sum()) == counts[q], (off, q, part[:8].tolist(), counts[q])


# (B, K, H, N, time); `off`: None, or the net whose W[1] sits one float and whose hidden / pre-activation buffers sit two
# floats off the 16-byte grid: plan_layer (VECA of the second layer), the pairing condition and gemm_vec_ok of both
# backward products then differ between the nets — the one-launch-per-net path of cfm_mlp_launch_layer and launch_gemm
@pytest.mark.parametrize("B,K,H,N,timed", [(64, 48, 64, 64, False), (256, 20, 64, 16, True), (1024, 512, 64, 32, True)])
def test_sf2m_two_layers_are_bit_equal_to_two_regression_steps(dev, B, K, H, N, timed):
    """Two layers cannot be exact past the SELU, so the property is the one the header promises: with lam = 1 and
    score_weight = 1 the step's gradients and losses are, net for net, the bits of cfm_mlp_regression_step_f32 on the
    same pointers (the flow net on ut, the score net on -eps) — aligned (gemm_pair_f32_mfma_two, mlp_layer_two /
    mlp_layer_glds_two), and with either net off the 16-byte grid (one launch per net on the one-net kernels, unpaired).  The flow net's bits
    do not move when the SCORE net goes off the grid."""
    g = torch.Generator().manual_seed(B + K)
    Kf = K + int(timed)
    dims = [Kf, H, N]
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)                  # noqa: E731
    xt, ut, eps, lam = rnd(B, K), rnd(B, N), rnd(B, N), torch.ones(B, device=dev)
    td = torch.rand(B, generator=g).to(dev) if timed else None
    Wb = [[rnd(H, Kf) / Kf ** 0.5, rnd(N, H) / H ** 0.5] for _ in range(2)]
    bb = [[0.1 * rnd(H), 0.1 * rnd(N)] for _ in range(2)]
    _lib, lib = _lib_()
    one = _ws_bytes(lib, _lib, B, dims)
    flow_aligned = None
    for off in (None, 1, 0):
        W = [list(Wb[0]), list(Wb[1])]
        hid, pre = [_nan((B, H), dev), _nan((B, H), dev)], [_nan((B, H), dev), _nan((B, H), dev)]
        if off is not None:
            W[off][1] = _off_grid(W[off][1], 1)
            hid[off], pre[off] = _off_grid(hid[off], 2), _off_grid(pre[off], 2)
            assert vec_ok(W[0][1], H, H) != vec_ok(W[1][1], H, H) and vec_ok(hid[0], H, H) != vec_ok(hid[1], H, H), "premise"
        gq = [_nan((B, N), dev), _nan((B, N), dev)]
        dW = [[_nan((H, Kf), dev), _nan((N, H), dev)] for _ in range(2)]
        db = [[_nan((H,), dev), _nan((N,), dev)] for _ in range(2)]
        losses = _nan((2,), dev)
        _sf2m_step(xt, td, ut, eps, lam, W[0] + W[1], bb[0] + bb[1], hid, pre, dW[0] + dW[1], db[0] + db[1], dims, B, gq[0], gq[1],
                   losses, 1.0, _nan_ws(2 * one, dev))
        got = [[t.clone() for t in dW[q] + db[q]] + [losses[q].clone()] for q in (0, 1)]
        assert all(bool(torch.isfinite(t).all()) for q in (0, 1) for t in got[q]), off
        for q in (0, 1):
            dW1, db1, loss1 = [_nan((H, Kf), dev), _nan((N, H), dev)], [_nan((H,), dev), _nan((N,), dev)], _nan((1,), dev)
            _regression_step(xt, td, ut if q == 0 else -eps, W[q], bb[q], dims, B, [hid[q]], [pre[q]], gq[q], dW1, db1, loss1,
                             _nan_ws(one, dev))
            for name, a, b in zip(("dW0", "dW1", "db0", "db1", "loss"), got[q], dW1 + db1 + [loss1[0]]):
                assert torch.equal(a, b), (off, q, name, _first_diff(a.reshape(-1, 1), b.reshape(-1, 1)))
        if off is None:
            flow_aligned = got[0]
        elif off == 1:
            assert all(torch.equal(a, b) for a, b in zip(flow_aligned, got[0])), "the flow net moved with the score net's alignment"


# ------------------------------------------- 4. nets deeper than the split-K pool holds at once ----
DEEP6 = [4, 16, 16, 16, 16, 16, 3]
DEEP15 = [4] + [16] * 14 + [3]
DEEP_B = 2048


def _deep_net(dims, seed, dev):
    """seeded weights at SELU's fixed point (variance 1 / fan_in), small biases"""
    g = torch.Generator().manual_seed(seed)
    n = len(dims) - 1
    W = [(torch.randn(dims[l + 1], dims[l], generator=g) / dims[l] ** 0.5).to(dev) for l in range(n)]
    b = [(0.1 * torch.randn(dims[l + 1], generator=g)).to(dev) for l in range(n)]
    return W, b, g


def _forward_train(x, W, b, dims, B, dev):
    _lib, lib = _lib_()
    n = len(dims) - 1
    hidden = [_nan((B, dims[l + 1]), dev) for l in range(n - 1)]
    preact = [_nan((B, dims[l + 1]), dev) for l in range(n - 1)]
    out = _nan((B, dims[n]), dev)
    cd = (ctypes.c_int * (n + 1))(*dims)
    _lib.check(lib.cfm_mlp_forward_train_f32(_lib.ptr(x), _arr(W), _arr(b), cd, n, B, _arr(hidden), _arr(preact), _lib.ptr(out),
                                             _lib.stream_ptr()), "cfm_mlp_forward_train_f32")
    torch.cuda.synchronize()
    return hidden, preact, out


@pytest.mark.parametrize("dims", [DEEP6, DEEP15], ids=["6-layers", "15-layers"])
def test_deep_backward_at_a_training_batch_matches_float64(dev, dims):
    """Every layer of these nets splits 32 ways at B = 2048 and the pool holds four such layers: the backward has to
    reduce and reuse it (asserted from the restated sizes).  dW, db, dx against float64 autograd of the same weights,
    SELU' evaluated at the float32 pre-activations, within 1e-5 of each tensor's largest entry."""
    import cfm_oracle as oracle
    B, n = DEEP_B, len(dims) - 1
    assert pool_refills(dims, B) >= 1 and all(wgrad_splits(dims[l + 1], dims[l], B) == 32 for l in range(n))
    W, b, g = _deep_net(dims, seed=n, dev=dev)
    x, dout = torch.randn(B, dims[0], generator=g).to(dev), torch.randn(B, dims[n], generator=g).to(dev)
    hidden, preact, _ = _forward_train(x, W, b, dims, B, dev)
    _lib, lib = _lib_()
    dW, db, dx = [_nan(tuple(w.shape), dev) for w in W], [_nan(tuple(v.shape), dev) for v in b], _nan((B, dims[0]), dev)
    _backward([x] + hidden, [None] + preact, W, dims, B, dout, dW, db, dx, _nan_ws(_ws_bytes(lib, _lib, B, dims), dev))
    _, rW, rb, rx = oracle.mlp_backward_f64([w.cpu().numpy() for w in W], [v.cpu().numpy() for v in b], x.cpu().numpy(),
                                            dout.cpu().numpy(), preact=[p.cpu().numpy() for p in preact])
    worst = 0.0
    for name, got, ref in [(f"dW[{l}]", dW[l], rW[l]) for l in range(n)] + [(f"db[{l}]", db[l], rb[l]) for l in range(n)] + [("dx", dx, rx)]:
        ref = torch.from_numpy(np.asarray(ref))
        dev_ = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, dev_)
        assert dev_ <= 1e-5, (name, dev_)
    print(f"{n} layers at B = {B}: largest deviation {worst:.2e} of a tensor's maximum")


def test_deep_backward_last_layer_is_exact_while_the_pool_is_reused(dev):
    """A chain cannot be exact past its first SELU', so of the 6-layer net at B = 2048 the LAST layer is: integer dout and
    integer acts[5] give dW[5], db[5] exactly (S = 32), on a NaN workspace, in a call whose pool is reduced and reused
    (its partials are the first to be reduced and the first to be overwritten).  The other layers carry random data and
    must come out finite: no NaN of the workspace reaches them."""
    dims, B = DEEP6, DEEP_B
    n = len(dims) - 1
    assert pool_refills(dims, B) >= 1 and wgrad_splits(dims[n], dims[n - 1], B) == 32
    W, b, g = _deep_net(dims, seed=3, dev=dev)
    h5, dout = _ints(g, (B, dims[n - 1]), -2, 2), _ints(g, (B, dims[n]), -2, 2)
    dW5, db5 = _mm(dout.T, h5), _colsum(dout)
    assert int(_absmm(dout.T, h5).max()) < LIMIT and int(dout.abs().sum(0).max()) < LIMIT
    acts = [torch.randn(B, dims[l], generator=g).to(dev) for l in range(n - 1)] + [h5.float().to(dev)]
    preact = [None] + [torch.randn(B, dims[l], generator=g).to(dev) for l in range(1, n)]
    _lib, lib = _lib_()
    dW, db, dx = [_nan(tuple(w.shape), dev) for w in W], [_nan(tuple(v.shape), dev) for v in b], _nan((B, dims[0]), dev)
    _backward(acts, preact, W, dims, B, dout.float().to(dev), dW, db, dx, _nan_ws(_ws_bytes(lib, _lib, B, dims), dev))
    _exact(dW[n - 1], dW5.double(), "dW[5]")
    _exact(db[n - 1], db5.double(), "db[5]")
    assert all(bool(torch.isfinite(t).all()) for t in dW + db + [dx])


def test_deep_regression_step_plain_and_bucketed_are_bit_equal(dev):
    """The 6-layer net with a time column through cfm_mlp_regression_step_f32 at B = 2048, with one final reduction
    (here: one per refill of the pool) and with `layer_done` events (one reduction per layer, every layer's partials at
    the pool's start): the same partials summed in the same order — gradients and loss bit-equal, and close to float64."""
    import cfm_oracle as oracle
    dims, B = DEEP6, DEEP_B
    n = len(dims) - 1
    assert pool_refills(dims, B, timed=True) >= 1
    W, b, g = _deep_net(dims, seed=9, dev=dev)
    xt, t, ut = torch.randn(B, dims[0] - 1, generator=g).to(dev), torch.rand(B, generator=g).to(dev), torch.randn(B, dims[n], generator=g).to(dev)
    _lib, lib = _lib_()
    events = [torch.cuda.Event() for _ in range(n)]
    for ev in events:
        ev.record(torch.cuda.current_stream())                             # (torch creates the HIP event at its first record)
    evp = (ctypes.c_void_p * n)(*[ev.cuda_event for ev in events])
    res = []
    for layer_done in (None, evp):
        hidden = [_nan((B, dims[l + 1]), dev) for l in range(n - 1)]
        preact = [_nan((B, dims[l + 1]), dev) for l in range(n - 1)]
        gbuf, loss = _nan((B, dims[n]), dev), _nan((1,), dev)
        dW, db = [_nan(tuple(w.shape), dev) for w in W], [_nan(tuple(v.shape), dev) for v in b]
        _regression_step(xt, t, ut, W, b, dims, B, hidden, preact, gbuf, dW, db, loss, _nan_ws(_ws_bytes(lib, _lib, B, dims), dev),
                         events=layer_done)
        res.append((dW + db + [loss], preact, gbuf))
    for i, (a, c) in enumerate(zip(res[0][0], res[1][0])):
        assert torch.equal(a, c) and bool(torch.isfinite(a).all()), (i, _first_diff(a.reshape(-1, 1), c.reshape(-1, 1)))
    x = torch.cat([xt, t.reshape(B, 1)], 1)
    _, rW, rb, _ = oracle.mlp_backward_f64([w.cpu().numpy() for w in W], [v.cpu().numpy() for v in b], x.cpu().numpy(),
                                           res[0][2].cpu().numpy(), preact=[p.cpu().numpy() for p in res[0][1]])
    for l in range(n):
        for got, ref in ((res[0][0][l], rW[l]), (res[0][0][n + l], rb[l])):
            ref = torch.from_numpy(np.asarray(ref))
            assert float((got.cpu().double() - ref).abs().max() / ref.abs().max()) <= 1e-5, l


def test_sf2m_step_of_two_seven_layer_nets_at_a_training_batch(dev):
    """cfm_amd.SF2MStep promises 7 layers; at B = 2048 every layer of width 16 splits 32 ways and both nets' pools are
    reused.  Losses and gradients against float64 autograd of the reference's lines, within 1e-5."""
    import copy

    import cfm_amd
    B, d, w, layers = DEEP_B, 3, 16, 7
    dims = [d + 1] + [w] * (layers - 1) + [d]
    assert pool_refills(dims, B, timed=True) >= 1 and layers == cfm_amd.SF2MStep.MAX_LAYERS
    torch.manual_seed(2048)
    nets = []
    for _ in range(2):
        net = cfm_amd.MLP(dim=d, time_varying=True, w=w)
        mods = []
        for k in range(layers):
            mods += ([torch.nn.SELU()] if k else []) + [torch.nn.Linear(dims[k], dims[k + 1])]
        net.net = torch.nn.Sequential(*mods)
        nets.append(net.to(dev))
    flow, score = nets
    t = torch.rand(B, device=dev)
    xt, ut, eps = torch.randn(B, d, device=dev), torch.randn(B, d, device=dev), torch.randn(B, d, device=dev)
    lam = 2 * torch.sqrt(t * (1 - t)) / 0.5
    params = [p for net in nets for p in net.parameters()]
    step = cfm_amd.SF2MStep(flow, score, cfm_amd.FusedAdam(params, lr=1e-3))
    losses = step.backward_only(t, xt, ut, eps, lam).cpu().double()
    f, s = copy.deepcopy(flow).double().cpu(), copy.deepcopy(score).double().cpu()
    for p in list(f.parameters()) + list(s.parameters()):
        p.grad = None
    x = torch.cat([xt.double().cpu(), t.double().cpu()[:, None]], dim=-1)
    fl = torch.mean((f.net(x) - ut.double().cpu()) ** 2)
    sl = torch.mean((lam.double().cpu()[:, None] * s.net(x) + eps.double().cpu()) ** 2)
    (fl + sl).backward()
    devs = [abs(float(losses[0]) - float(fl)) / float(fl), abs(float(losses[1]) - float(sl)) / float(sl)]
    devs += [float((p.grad.double().cpu() - q.grad).abs().max() / q.grad.abs().max())
             for p, q in zip(params, list(f.parameters()) + list(s.parameters()))]
    print(f"two 7-layer nets at B = {B}: losses {devs[0]:.2e} {devs[1]:.2e}, gradients max {max(devs[2:]):.2e}")
    assert max(devs) <= 1e-5, devs


# ------------------------------------------------------------------- 5. the regression step's unfused loss ----
def test_regression_step_unfused_loss_behind_a_tall_last_layer(dev):
    """A last layer of more 64 x 64 output tiles than the workspace has loss partials (B = 64 * 4097 rows, N = 1): the
    regression step runs it as a plain layer and forms seed and loss in mse_grad (MSE_BLOCKS = 256 partials), the SF2M step,
    which has no such launch, answers CFM_EINVAL.  One untimed layer on integer data, ut = v - e with e in {-3 .. 3}:
      g      bit-equal to fl((v - ut) fl(2 fl(1 / n))): v - ut is an exact integer, the product one rounding — torch's CPU
             float32 multiply is the reference
      loss   against the float64 mean of squares within 16 * 2^-24 relative: every term is non-negative, each of the 256
             partials an exact integer sum below 2^24 (asserted: the sum of ALL squares is) times inv_n, one rounding; the
             reduction adds at most four per lane and six tree levels
      dW, db genuine fp32 sums of the seeds: against float64 within B 2^-24 sum |terms|, the bound of db[0] above."""
    B, K, N = 64 * 4097, 4, 1
    assert ((B + 63) // 64) * ((N + 63) // 64) > LOSS_PARTIALS, "premise: more output tiles than loss partials"
    x, w, b, _, v = _layer_data(B, K, N, None, seed=B + K + N)
    e = _ints(torch.Generator().manual_seed(17), (B, N), -3, 3)
    ut = v - e
    n = B * N
    assert int(ut.abs().max()) < LIMIT and int(v.abs().max()) < LIMIT
    assert int((e * e).sum()) < LIMIT, "premise: every loss partial is an exact integer below 2^24"
    scale = np.float32(2) * (np.float32(1) / np.float32(n))                # 2.0f * (1.0f / (float)n)
    g_ref = (v - ut).float() * torch.tensor(scale, dtype=torch.float32)
    loss_ref = float((e * e).sum()) / n
    terms_W = g_ref.double() * x.double()                                  # [B, K]: dW[0, k] = sum_b g[b] x[b, k]
    terms_b = g_ref.double()
    _lib, lib = _lib_()
    dims = [K, N]
    xd, wd, bd, utd = (q.float().to(dev) for q in (x, w, b, ut))
    gd, dWd, dbd, loss = _nan((B, N), dev), _nan((N, K), dev), _nan((N,), dev), _nan((1,), dev)
    one = _ws_bytes(lib, _lib, B, dims)
    _regression_step(xd, None, utd, [wd], [bd], dims, B, None, None, gd, [dWd], [dbd], loss, _nan_ws(one, dev))
    assert torch.equal(gd.cpu(), g_ref), _first_diff(gd, g_ref)
    got_loss = float(loss.cpu().double())
    print(f"unfused loss: {got_loss!r} against {loss_ref!r}, relative error {abs(got_loss - loss_ref) / loss_ref:.3e}")
    assert abs(got_loss - loss_ref) <= 16 * 2.0 ** -24 * loss_ref, (got_loss, loss_ref)
    for name, got, terms in (("dW", dWd.reshape(K), terms_W), ("db", dbd, terms_b)):
        err = (got.cpu().double() - terms.sum(0)).abs()
        bound = B * 2.0 ** -24 * terms.abs().sum(0)
        print(f"{name}: max error {float(err.max()):.3e}, smallest slack {float((bound - err).min()):.3e}")
        assert bool((err <= bound).all()), (name, float(err.max()), float(bound.min()))
    # the SF2M step at this shape: refused, nothing launched
    cd = (ctypes.c_int * 2)(*dims)
    gs, dW2, db2, losses = _nan((B, N), dev), [_nan((N, K), dev) for _ in range(2)], [_nan((N,), dev) for _ in range(2)], _nan((2,), dev)
    lam = torch.ones(B, device=dev)
    rc = lib.cfm_mlp_sf2m_step_f32(_lib.ptr(xd), None, _lib.ptr(utd), _lib.ptr(utd), _lib.ptr(lam), _arr([wd, wd]), _arr([bd, bd]), None, None,
                                   _arr(dW2), _arr(db2), cd, 1, B, _lib.ptr(gd), _lib.ptr(gs), _lib.ptr(losses), 1.0, _lib.ptr(_nan_ws(2 * one, dev)),
                                   _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1, ("CFM_EINVAL", rc)
