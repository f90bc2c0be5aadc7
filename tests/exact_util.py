"""Shared pieces of the tolerance-free GPU tests (test_gpu_gemm_exact.py, test_gpu_backward_exact.py): integer data, NaN
output buffers, the failure message, and the host restatement of the launch rules of csrc/mlp_train.hip / csrc/mlp.hip.
The restated rules are used ONLY to assert the premise of a case (the split count, the tile, the pairing it is meant to
reach): if a rule moves, the case fails its premise instead of silently covering something else."""
import ctypes

import torch

LIMIT = 2 ** 24
MAX_SPLITS = 32                                 # MLP_MAX_SPLITS
LOSS_PARTIALS = 4096                            # MLP_LOSS_PARTIALS
SELU_SCALE = 1.0507009873554805
SELU_ALPHA = 1.6732632423543772


def lib_():
    from cfm_amd import _lib
    return _lib, _lib.load()


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else 0 for t in ts])


def _ints(gen, shape, lo, hi):
    """int64 tensor, uniform in {lo .. hi}"""
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


def _nan(shape, dev):
    """an output buffer no kernel has written yet: an element the kernel skips stays NaN and fails torch.equal"""
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def _nan_ws(nbytes, dev):
    """a workspace no kernel has written yet, as floats: a partial that is read before it is written poisons the result"""
    return torch.full(((nbytes + 3) // 4,), float("nan"), device=dev, dtype=torch.float32)


def _first_diff(got, ref):
    """(index, got, expected) of the first differing element and the number of them (for the failure message)"""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    bad = ~(g == r)
    n = int(bad.sum())
    if n == 0:
        return "equal"
    idx = tuple(int(v) for v in bad.nonzero()[0])
    rows = sorted(set(int(v) for v in bad.nonzero()[:, 0][:2000]))[:8]
    return f"{n} of {g.numel()} differ; first at {idx}: got {float(g[idx])}, expected {float(r[idx])}; rows {rows}"


class _Mode:
    """cfm_mlp_set_glds(mode) for the body, the previous mode back in every case"""

    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.prev = self.lib.cfm_mlp_get_glds()
        self.lib.cfm_mlp_set_glds(self.mode)

    def __exit__(self, *exc):
        self.lib.cfm_mlp_set_glds(self.prev)
        return False


def _layer_data(B, K, N, time, seed, lo=-3, hi=3):
    """One Linear layer's integer data and its int64 result.  time: None | "scalar" | "row"; with a time the weight has
    K + 1 columns (the time column last: rows of 4 (K + 1) bytes, 4-byte aligned only when K + 1 is odd)."""
    g = torch.Generator().manual_seed(seed)
    x = _ints(g, (B, K), lo, hi)
    w = _ints(g, (N, K + (time is not None)), lo, hi)
    b = _ints(g, (N,), -50, 50)
    t = None if time is None else (_ints(g, (B,), lo, hi) if time == "row" else torch.tensor([2], dtype=torch.int64))
    ref = x @ w[:, :K].T + b
    mag = x.abs() @ w[:, :K].abs().T + b.abs()
    if t is not None:
        tt = t.reshape(-1, 1) if time == "row" else t.reshape(1, 1).expand(B, 1)
        ref = ref + tt * w[:, K].reshape(1, N)
        mag = mag + tt.abs() * w[:, K].abs().reshape(1, N)
    assert int(mag.max()) < LIMIT, "premise: every partial sum is an exact fp32 integer"
    return x, w, b, t, ref


# ---------------------------------------------------------------- the launch rules, restated ----
def pick_tile(M, N, splits):
    """cfm_gemm_pick_tile (mlp.hip): 0 = 128 x 128 x 16, 2 = 64 x 64 x 32"""
    return 0 if ((M + 127) // 128) * ((N + 127) // 128) * splits >= 512 else 2


def wgrad_splits(N, K, B):
    """wgrad_splits (mlp_train.hip): batch splits of dW[N, K]"""
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    S = 1
    while S < MAX_SPLITS and tiles * S < 256 and B // (2 * S) >= 64:
        S *= 2
    return S


def k_chunk(Kc, S):
    """launch_gemm: the contraction length of one split, a multiple of 32"""
    return ((Kc + S - 1) // S + 31) // 32 * 32


def split_ranges(B, S):
    """[k_begin, k_end) of every split of a contraction over B; k_begin >= k_end: an empty split"""
    kc = k_chunk(B, S)
    return [(s * kc, min(s * kc + kc, B)) for s in range(S)]


def vec_ok(t, ld, extent):
    """gemm_vec_ok: 16-byte loads of an operand (t: tensor or address)"""
    p = t if isinstance(t, int) else t.data_ptr()
    return ld % 4 == 0 and p % 16 == 0 and extent % 4 == 0


def pair_ok(B, K, N, S, dz, act, W):
    """the pairing condition of mlp_backward_impl for a layer dW[N, K] with l > 0: dgrad + wgrad in one launch"""
    return (pick_tile(N, K, S) == 2 and pick_tile(B, K, 1) == 2 and vec_ok(dz, N, N) and vec_ok(act, K, K)
            and vec_ok(W, K, K))


def pool_floats(dims):
    """the split-K pool of a CFM_OP_MLP_TRAIN workspace (cfm_mlp_train_ws_bytes_internal), in floats"""
    n = len(dims) - 1
    return MAX_SPLITS * (max(dims[l] * dims[l + 1] for l in range(n)) + max(dims)) * 4


def lpart_offset(B, dims):
    """where the loss partials of the fused steps start in their workspace, in floats: behind two [B, widest] buffers
    and the pool"""
    return 2 * B * max(dims) + pool_floats(dims)


def pool_refills(dims, B, timed=False):
    """how often a backward over `dims` at batch B finds its pool full (0: every layer's partials fit at once)"""
    n, used, refills = len(dims) - 1, 0, 0
    for l in range(n - 1, -1, -1):
        K = dims[l] - int(timed and l == 0)
        N = dims[l + 1]
        need = wgrad_splits(N, K, B) * (N * K + N * (2 if timed and l == 0 else 1))
        if used + need > pool_floats(dims):
            refills, used = refills + 1, 0
        used += need
    return refills
