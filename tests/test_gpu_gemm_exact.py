"""Tolerance-free tests of the dense engines (csrc/gemm_core.h, gemm_glds.h, gemm_glds64.h) behind the MLP entry points.

With small-integer inputs every product and every partial sum of a layer is an integer below 2^24: the fp32 result does
not depend on the summation order and is EXACT.  The reference is an int64 matmul on the host and the comparison is
`torch.equal` — every element of every launch, no tolerance, nothing masked.  Each test first asserts the premise on the
host for its own data (sum_k |x| |w| + |b| + |t w_t| < 2^24), so it is checked and not assumed.

The fp64 tests of test_gpu_glds64.py / test_gpu_train.py bound the error by 1e-5 of the tensor's maximum: a stale
accumulator in one tile of one launch, or an error confined to small outputs, can stay below that.  Here it cannot.
The kernels are driven through the C ABI with ctypes (n_layers = 1 or 2), as `_abi_step` of test_gpu_train.py does."""
import ctypes

import pytest
import torch

from exact_util import LIMIT, _Mode, _arr, _first_diff, _ints, _layer_data, _nan, _nan_ws
from exact_util import lib_ as _lib_

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _forward1(lib, _lib, dev, xd, wd, bd, td, t_per_row, dims, B):
    out = _nan((B, dims[1]), dev)
    cd = (ctypes.c_int * 2)(*dims)
    _lib.check(lib.cfm_mlp_forward_f32(_lib.ptr(xd), _lib.ptr(td), t_per_row, _arr([wd]), _arr([bd]), cd, 1, B,
                                       _lib.ptr(out), ctypes.c_void_p(0), _lib.stream_ptr()), "cfm_mlp_forward_f32")
    torch.cuda.synchronize()
    return out


# (B, K, N, time): K = 16 (the tail step alone), 32, 48 (step + tail), 64, 512, 784, 20 (not a multiple of 16: the
# register-staged core in every mode), 784 + time = the 785-wide first layer (4-byte aligned weight rows: the DMA engine
# in mode 2 only); B in {1, 63, 64, 65, 130, 257, 4096}; N in {1, 16, 48, 64, 65, 80, 512, 784}; 4096 x 2048 outputs are
# 512 tiles of 128 x 128: the 128-tile core.
FORWARD_CASES = [
    (1, 16, 1, None), (63, 16, 16, "row"), (64, 32, 48, "scalar"), (65, 48, 64, None), (130, 64, 65, "row"),
    (257, 512, 80, None), (4096, 784, 512, "row"), (4096, 512, 512, None), (4096, 512, 784, None),
    (257, 20, 48, "scalar"), (130, 20, 65, None), (63, 784, 784, "row"), (64, 784, 1, "scalar"), (65, 16, 784, "row"),
    (1, 512, 512, None), (1, 784, 16, "row"), (130, 48, 80, "scalar"), (257, 32, 64, "row"), (4096, 64, 2048, None),
    (4096, 64, 2048, "row"), (63, 64, 512, None), (64, 512, 16, "row"), (65, 784, 48, None), (130, 784, 512, "scalar"),
    (257, 16, 65, None), (4096, 48, 80, "row"), (4096, 16, 1, None), (130, 32, 784, None), (64, 20, 16, "row"),
    (257, 64, 64, "scalar"), (63, 48, 65, "row"), (65, 512, 64, "scalar"),
]


@pytest.mark.parametrize("B,K,N,time", FORWARD_CASES)
def test_forward_one_layer_is_exact_in_every_mode(dev, B, K, N, time):
    _lib, lib = _lib_()
    x, w, b, t, ref = _layer_data(B, K, N, time, seed=1000 * B + 10 * K + N)
    xd, wd, bd = x.float().to(dev), w.float().to(dev), b.float().to(dev)
    td = None if t is None else t.float().to(dev)
    refd = ref.float().to(dev)
    assert torch.equal(refd.cpu().long(), ref)
    dims = [K + (time is not None), N]
    for mode in (0, 1, 2):
        with _Mode(lib, mode):
            out = _forward1(lib, _lib, dev, xd, wd, bd, td, 1 if time == "row" else 0, dims, B)
        assert torch.equal(out, refd), (mode, _first_diff(out, refd))


@pytest.mark.parametrize("B,K,N", [(257, 48, 144), (4096, 64, 192), (130, 16, 80), (4096, 784, 784)])
def test_forward_index_encoding_names_the_element_that_landed(dev, B, K, N):
    """X[i, k] = i K + k and W[j] one-hot at k = j mod K, scaled by j // K + 1: out[i, j] = (i K + j mod K) (j // K + 1)
    names its own row and k (the engine stores the B rows of a tile permuted in LDS: a wrong permutation, a swapped
    fragment or a stale accumulator shows up as the coordinates of the element that arrived instead)."""
    _lib, lib = _lib_()
    assert B * K * (N // K + 1) < LIMIT
    i, k, j = torch.arange(B).reshape(B, 1), torch.arange(K).reshape(1, K), torch.arange(N)
    x = i * K + k
    w = torch.zeros((N, K), dtype=torch.int64)
    w[j, j % K] = j // K + 1
    ref = x @ w.T
    assert torch.equal(ref, (i * K + (j % K).reshape(1, N)) * (j // K + 1).reshape(1, N))
    assert int((x.abs() @ w.abs().T).max()) < LIMIT
    xd, wd, bd, refd = x.float().to(dev), w.float().to(dev), torch.zeros(N, device=dev), ref.float().to(dev)
    for mode in (0, 1, 2):
        with _Mode(lib, mode):
            out = _forward1(lib, _lib, dev, xd, wd, bd, None, 0, [K, N], B)
        if not torch.equal(out, refd):
            o = out.cpu().double()
            bad = (~(o == ref.double())).nonzero()
            msgs = []
            for r, c in bad[:6].tolist():
                s, v = c // K + 1, o[r, c].item()
                src = divmod(int(v) // s, K) if v == v and v % s == 0 else None
                msgs.append(f"out[{r},{c}] (k {c % K}, scale {s}) = {v}: that is (row, k) = {src}")
            pytest.fail(f"mode {mode}: {len(bad)} elements differ; " + "; ".join(msgs))


@pytest.mark.parametrize("K,N,time", [(784, 512, "row"), (512, 512, None), (512, 784, None)])
def test_repeat_launches_of_the_c3_layers_are_exact_every_time(dev, K, N, time):
    """25 launches of each C3 layer shape on the default engine, every output compared on the device.  A fixed small
    count: a determinism check (a hazard shows on some waves of some launches), not a stress loop."""
    _lib, lib = _lib_()
    B = 4096
    x, w, b, t, ref = _layer_data(B, K, N, time, seed=K + N)
    xd, wd, bd = x.float().to(dev), w.float().to(dev), b.float().to(dev)
    td = None if t is None else t.float().to(dev)
    refd = ref.float().to(dev)
    dims = [K + (time is not None), N]
    bad = []
    with _Mode(lib, 2):
        for it in range(25):
            out = _forward1(lib, _lib, dev, xd, wd, bd, td, 1 if time == "row" else 0, dims, B)
            if not torch.equal(out, refd):
                bad.append((it, _first_diff(out, refd)))
    assert not bad, bad


@pytest.mark.parametrize("B,K,H,N", [(4096, 784, 512, 16), (130, 48, 80, 16), (65, 16, 65, 1), (257, 512, 784, 64),
                                     (4096, 512, 512, 48)])
def test_activated_layer_preact_exact_and_selu_close(dev, B, K, H, N):
    """cfm_mlp_forward_train_f32 with two layers: preact[0] (the `zout` store of the activated instantiation) exact;
    hidden[0] against fp64 selu(z) on the exact z, per element within 1e-5 max(1, |h|) (the project's fp32 bound; the
    device expm1f is good to a few ulp — the exact pre-activation is the point)."""
    _lib, lib = _lib_()
    x, w, b, _, z = _layer_data(B, K, H, None, seed=B + K + H)
    g = torch.Generator().manual_seed(7)
    w2, b2 = _ints(g, (N, H), -1, 1), _ints(g, (N,), -3, 3)
    xd, wd, bd, w2d, b2d = (v.float().to(dev) for v in (x, w, b, w2, b2))
    zref = z.float().to(dev)
    href = torch.nn.functional.selu(z.double())
    cd = (ctypes.c_int * 3)(K, H, N)
    for mode in (0, 1, 2):
        hidden, preact, out = _nan((B, H), dev), _nan((B, H), dev), _nan((B, N), dev)
        with _Mode(lib, mode):
            _lib.check(lib.cfm_mlp_forward_train_f32(_lib.ptr(xd), _arr([wd, w2d]), _arr([bd, b2d]), cd, 2, B,
                                                     _arr([hidden]), _arr([preact]), _lib.ptr(out), _lib.stream_ptr()),
                       "cfm_mlp_forward_train_f32")
            torch.cuda.synchronize()
        assert torch.equal(preact, zref), (mode, _first_diff(preact, zref))
        h = hidden.cpu().double()
        err = (h - href).abs() / href.abs().clamp(min=1.0)
        print(f"mode {mode}: max selu error {float(err.max()):.3e} (bound 1e-5)")
        assert bool((err <= 1e-5).all()), (mode, float(err.max()))
        assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("B,K,N", [(130, 20, 65), (257, 48, 80), (63, 784, 33), (65, 16, 1), (1, 16, 16),
                                   (4096, 784, 512), (4096, 512, 784), (4096, 512, 512)])
def test_backward_one_layer_is_exact(dev, B, K, N):
    """cfm_mlp_backward_f32 with one layer: dW = dout^T x, db = sum dout, dx = dout W on gemm_core.h (B = 4096: split-K
    partials and their fixed-order reduction).  Values in {-2 .. 2}.  The workspace starts as NaN: a partial that the
    reduction reads and no workgroup wrote shows.  (Split-K edges: test_gpu_backward_exact.py.)"""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(B * 7 + K + N)
    x, w, dout = _ints(g, (B, K), -2, 2), _ints(g, (N, K), -2, 2), _ints(g, (B, N), -2, 2)
    dW, db, dx = dout.T @ x, dout.sum(0), dout @ w
    assert int((dout.abs().T @ x.abs()).max()) < LIMIT and int(dout.abs().sum(0).max()) < LIMIT
    assert int((dout.abs() @ w.abs()).max()) < LIMIT
    xd, wd, dd = x.float().to(dev), w.float().to(dev), dout.float().to(dev)
    dWd, dbd, dxd = _nan((N, K), dev), _nan((N,), dev), _nan((B, K), dev)
    ws = _nan_ws(lib.cfm_workspace_bytes(_lib.OP_MLP_TRAIN, B, max(K, N), K * N), dev)
    cd = (ctypes.c_int * 2)(K, N)
    _lib.check(lib.cfm_mlp_backward_f32(_arr([xd]), _arr([None]), _arr([wd]), cd, 1, B, _lib.ptr(dd), _arr([dWd]),
                                        _arr([dbd]), _lib.ptr(dxd), _lib.ptr(ws), _lib.stream_ptr()), "cfm_mlp_backward_f32")
    torch.cuda.synchronize()
    for name, got, ref in (("dW", dWd, dW), ("db", dbd, db), ("dx", dxd, dx)):
        refd = ref.float().to(dev)
        assert torch.equal(got, refd), (name, _first_diff(got, refd))


@pytest.mark.parametrize("B,K,N,timed", [(64, 48, 64, False), (4096, 784, 512, True), (256, 20, 16, True),
                                         (128, 64, 128, False), (1024, 512, 32, True), (8192, 16, 4096, False)])
def test_mse_epilogue_is_exact(dev, B, K, N, timed):
    """cfm_mlp_regression_step_f32 with one layer, n = B N a power of two and ut = v + e, e in {-1, 0, 1}:
    g = (2 / n)(v - ut) = -(2 / n) e and loss = #{e != 0} / n are exact, and so is every per-workgroup partial (an
    integer count over n).  The gradients that follow from g are exact too (integers times 2 / n).  The last case has
    more workgroups than loss-partial slots: the stand-alone MSE kernel."""
    _lib, lib = _lib_()
    n = B * N
    assert n & (n - 1) == 0
    x, w, b, t, v = _layer_data(B, K, N, "row" if timed else None, seed=B + K + N)
    g = torch.Generator().manual_seed(3)
    e = _ints(g, (B, N), -1, 1)
    ut = v + e
    assert int(ut.abs().max()) < LIMIT
    count = int((e != 0).sum())
    Kf = K + int(timed)
    xin = torch.cat([x, t.reshape(B, 1)], 1) if timed else x
    # everything below is an integer times 2 / n, |integer| < 2^24: exact in fp32
    assert int((e.abs().T @ xin.abs()).max()) < LIMIT
    scale = 2.0 / n
    g_ref = (-e).double() * scale
    dW_ref = ((-e).T @ xin).double() * scale
    db_ref = (-e).sum(0).double() * scale
    xd, wd, bd, utd = (q.float().to(dev) for q in (x, w, b, ut))
    td = t.float().to(dev) if timed else None
    cd = (ctypes.c_int * 2)(Kf, N)
    fused = ((B + 63) // 64) * ((N + 63) // 64) <= 4096
    for mode in (0, 2):
        gd, dWd, dbd, loss = _nan((B, N), dev), _nan((N, Kf), dev), _nan((N,), dev), _nan((1,), dev)
        nbytes = lib.cfm_workspace_bytes(_lib.OP_MLP_TRAIN, B, max(Kf, N), Kf * N)
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
        with _Mode(lib, mode):
            _lib.check(lib.cfm_mlp_regression_step_f32(_lib.ptr(xd), _lib.ptr(td), _lib.ptr(utd), _arr([wd]), _arr([bd]), cd, 1, B,
                                                       None, None, _lib.ptr(gd), _arr([dWd]), _arr([dbd]), _lib.ptr(loss),
                                                       None, _lib.ptr(ws), _lib.stream_ptr()), "cfm_mlp_regression_step_f32")
            torch.cuda.synchronize()
        for name, got, ref in (("g", gd, g_ref), ("dW", dWd, dW_ref), ("db", dbd, db_ref)):
            refd = ref.float().to(dev)
            assert torch.equal(refd.cpu().double(), ref)
            assert torch.equal(got, refd), (mode, name, _first_diff(got, refd))
        assert float(loss.cpu()[0]) == count / n, (mode, float(loss.cpu()[0]), count / n)
        # the loss partials sit in the last 4096 floats of the workspace (include/cfm_gfx950.h, CFM_OP_MLP_TRAIN); the
        # split-K pool in front of them is far from full at these shapes, so the slots nobody wrote are still NaN
        tail = ws[-(4096 + 64):].cpu().double()
        part = tail[~torch.isnan(tail)] * n
        assert torch.equal(part, part.round()) and int(part.sum()) == count, (mode, part[:8].tolist(), count)
        if fused and ((B + 127) // 128) * ((N + 127) // 128) < 512:          # 64 x 64 tiles: one partial per tile
            tiles = [int((e[r:r + 64, c:c + 64] != 0).sum()) for r in range(0, B, 64) for c in range(0, N, 64)]
            assert sorted(int(p) for p in part.tolist()) == sorted(tiles), (mode, "per-workgroup loss partials")
