"""Host restatement (NumPy only) of the noise stream the one-launch SDE samplers draw under noise="philox":
Philox4x32-10, the 24-bit uniforms, Box-Muller and the map from a (row, column) of the batch to a counter, as
conditional-flow-matching_amd/csrc/sde_small.h writes them (philox_round :18-23, philox_normal4_w3 :25-38, the draws
of ode_small_em :114 and ode_small_srk :207-210).

The generator is Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11): multipliers 0xD2511F53 on word
0 and 0xCD9E8D57 on word 2, round output {hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)}, the key bumped by
0x9E3779B9 / 0xBB67AE85 after each of the 10 rounds.  tests/test_philox_host.py pins this file to the published
known-answer vectors; tests/test_gpu_sde_philox.py pins the kernels to this file."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_XI1 = 0x5F2D          # the Euler-Maruyama increments and xi1 of srk
STREAM_XI2 = 0x5F2E          # xi2 of srk
TILE_ROWS, TILE_LANES = 16, 256
MASK32 = np.uint64(0xFFFFFFFF)
TWO_PI_F32 = np.float32(6.283185307179586)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcast against each other) of 32-bit words -> [..., 4] uint32."""
    ctr = np.asarray(ctr, dtype=np.uint64) & MASK32
    key = np.asarray(key, dtype=np.uint64) & MASK32
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape) for i in range(4)]
    k0, k1 = np.broadcast_to(key[..., 0], shape), np.broadcast_to(key[..., 1], shape)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no wrap in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(c, axis=-1).astype(np.uint32)


def _words(seed, step, elem, stream):
    """The block of one draw: counter {elem lo, elem hi, step, stream}, key {seed lo, seed hi}."""
    elem = np.asarray(elem, dtype=np.uint64)
    step = np.broadcast_to(np.asarray(step, dtype=np.uint64), elem.shape)
    stream = np.broadcast_to(np.asarray(stream, dtype=np.uint64), elem.shape)
    ctr = np.stack([elem & MASK32, elem >> np.uint64(32), step & MASK32, stream & MASK32], axis=-1)
    seed = int(seed)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))


def normals(seed, step, elem, stream=STREAM_XI1):
    """[..., 4] float64: the four N(0, 1) of every counter in `elem`, exact arithmetic on the kernel's 24-bit uniforms."""
    c = _words(seed, step, elem, stream)
    m = (c >> np.uint32(8)).astype(np.float64)
    u0, u1 = (m[..., 0] + 1.0) / 2.0 ** 24, m[..., 1] / 2.0 ** 24
    u2, u3 = (m[..., 2] + 1.0) / 2.0 ** 24, m[..., 3] / 2.0 ** 24
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    a0, a1 = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def normals_f32(seed, step, elem, stream=STREAM_XI1):
    """`normals` with every operation in float32, the 6.283185307179586f * u product included (philox_normal4_w3's own
    statements).  It serves only to size the tolerance of the device comparison."""
    f = np.float32
    c = _words(seed, step, elem, stream)
    m = (c >> np.uint32(8)).astype(f)                                  # < 2^24: exact
    inv = f(1.0) / f(16777216.0)
    u0, u1 = (m[..., 0] + f(1.0)) * inv, m[..., 1] * inv
    u2, u3 = (m[..., 2] + f(1.0)) * inv, m[..., 3] * inv
    r0, r1 = np.sqrt(f(-2.0) * np.log(u0)), np.sqrt(f(-2.0) * np.log(u2))
    a0, a1 = TWO_PI_F32 * u1, TWO_PI_F32 * u3
    out = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)
    assert out.dtype == np.float32
    return out


def tile_map(row, col):
    """(elem, component) of batch row `row` and state column `col` < 64: which counter, and which of its four normals.

    A workgroup of 256 threads owns the 16-row tile `row // 16`.  Thread tid = 64 * wave + lane holds column
    16 * wave + (lane & 15) (sde_small.h:93 and :170) of the four rows sm_row(i, lane) = 4 * (lane >> 4) + i, i < 4
    (small_field.h:32, one 16-row block per tile), draws ONE block at elem = 256 * tile + tid (sde_small.h:114, :208) and
    gives normal i to element i."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    tile, r = row // TILE_ROWS, row % TILE_ROWS
    tid = (col // 16) * 64 + (r // 4) * 16 + col % 16
    return tile * TILE_LANES + tid, r % 4


def step_normals(seed, step, B, d, stream=STREAM_XI1, f32=False):
    """[B, d]: the normals one step of the kernel gives to rows 0 ... B - 1 and columns 0 ... d - 1."""
    assert 1 <= d <= 64
    elem, comp = tile_map(np.arange(B)[:, None], np.arange(d)[None, :])
    z = (normals_f32 if f32 else normals)(seed, step, elem, stream)
    return np.take_along_axis(z, comp[..., None], axis=-1)[..., 0]


def noise_tensor(seed, n_steps, B, d, srk=False, f32=False):
    """The tensor the kernel draws in Philox mode: [n_steps, B, d], or [n_steps, 2, B, d] (xi1, xi2) for srk.  Step k of
    the REFINED grid uses counter word step = k."""
    if srk:
        return np.stack([np.stack([step_normals(seed, k, B, d, s, f32) for s in (STREAM_XI1, STREAM_XI2)])
                         for k in range(n_steps)])
    return np.stack([step_normals(seed, k, B, d, STREAM_XI1, f32) for k in range(n_steps)])


def f32_gap(seed, n_steps, B, d, srk=False):
    """max |normals_f32 - normals| over the counters of a case: what float32 Box-Muller alone costs."""
    return float(np.abs(noise_tensor(seed, n_steps, B, d, srk, True).astype(np.float64)
                        - noise_tensor(seed, n_steps, B, d, srk, False)).max())
