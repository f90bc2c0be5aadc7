"""CPU: tests/philox_ref.py, the host restatement of the SDE samplers' in-kernel noise stream — the published
known-answer vectors of Philox4x32-10, the tile map's bijection, and the moments of one step's normals.  The GPU side
(tests/test_gpu_sde_philox.py) compares the kernels with this restatement element by element."""
import math

import numpy as np
import pytest

import philox_ref as P

# Random123's kat_vectors for philox4x32 at 10 rounds: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SEED, STEP = 123456789012345, 3
N_ELEM = 4097 * 256               # the counters of one step of a batch of 16 * 4096 + 16 rows


@pytest.fixture(scope="module")
def streams():
    """{(step, stream): [N_ELEM, 4] float64} for (STEP, STEP + 1) x (xi1, xi2); computed once, never changed."""
    elem = np.arange(N_ELEM)
    return {(k, s): P.normals(SEED, k, elem, s) for k in (STEP, STEP + 1) for s in (P.STREAM_XI1, P.STREAM_XI2)}


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        got = P.philox4x32_10(np.array(ctr), np.array(key))
        assert [int(x) for x in got] == list(want), [hex(int(x)) for x in got]
    # vectorised over an array of counters and keys: the same words, row by row
    got = P.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT]
    # one key broadcast over many counters
    got = P.philox4x32_10(np.array([KAT[0][0], KAT[0][0]]), np.array(KAT[0][1]))
    assert got.tolist() == [list(KAT[0][2])] * 2


def test_counter_and_key_words():
    """normals() places elem in words 0 and 1, step in word 2, the stream in word 3 and the seed's halves in the key."""
    seed, step, elem = (0xa4093822 | (0x299f31d0 << 32)), 0x13198a2e, (0x243f6a88 | (0x85a308d3 << 32))
    got = P._words(seed, step, np.array([elem], dtype=np.uint64), 0x03707344)
    assert got[0].tolist() == list(KAT[2][2])


def test_tile_map_is_a_bijection_onto_lanes_and_components():
    row, col = np.meshgrid(np.arange(16), np.arange(64), indexing="ij")
    elem, comp = P.tile_map(row, col)
    assert elem.min() == 0 and elem.max() == 255 and comp.min() == 0 and comp.max() == 3
    assert len({(int(e), int(c)) for e, c in zip(elem.ravel(), comp.ravel())}) == 16 * 64 == 256 * 4
    # rows 16 apart: the same lane and component of the next tile
    for shift in (16, 16 * 4096, 16 * 4097):
        e2, c2 = P.tile_map(row + shift, col)
        assert np.array_equal(e2, elem + 256 * (shift // 16)) and np.array_equal(c2, comp)
    # the kernel's own layout: thread tid holds column 16 * wave + (lane & 15) of rows 4 * (lane >> 4) + i
    for tid in (0, 15, 16, 63, 64, 200, 255):
        lane, wave = tid & 63, tid >> 6
        for i in range(4):
            e, c = P.tile_map(4 * (lane >> 4) + i, 16 * wave + (lane & 15))
            assert (int(e), int(c)) == (tid, i)


def test_moments_of_one_step(streams):
    z = streams[(STEP, P.STREAM_XI1)].ravel()
    n = z.size
    assert n == 4 * N_ELEM
    # standard errors of the first, second and fourth sample moments of N(0, 1): 1, sqrt(2), sqrt(96) over sqrt(n)
    m1, m2, m4 = z.mean(), (z ** 2).mean(), (z ** 4).mean()
    print(f"n = {n}: mean {m1:.3e}, variance {m2 - 1:+.3e}, fourth moment {m4 - 3:+.3e} "
          f"(4 se: {4 / math.sqrt(n):.2e}, {4 * math.sqrt(2 / n):.2e}, {4 * math.sqrt(96 / n):.2e})")
    assert abs(m1) <= 4.0 / math.sqrt(n)
    assert abs(m2 - 1.0) <= 4.0 * math.sqrt(2.0 / n)
    assert abs(m4 - 3.0) <= 4.0 * math.sqrt(96.0 / n)
    # the smallest uniform is 2^-24: r <= sqrt(-2 ln 2^-24)
    assert np.abs(z).max() <= math.sqrt(48.0 * math.log(2.0))
    assert np.isfinite(z).all()


def test_the_four_streams_differ(streams):
    keys = sorted(streams)
    assert len(keys) == 4
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            x, y = streams[a], streams[b]
            assert not np.array_equal(x, y)
            # not equal anywhere near wholesale: uncorrelated within 5 standard errors, and no shared block
            assert abs(float((x * y).mean())) <= 5.0 / math.sqrt(x.size), (a, b)
            assert int((x == y).all(axis=-1).sum()) == 0, (a, b)


def test_float32_box_muller_gap(streams):
    """What the float32 form of the same statements costs: it sizes the tolerance of the device comparison.  Measured
    here: 1.7e-6 over these counters."""
    z32 = P.normals_f32(SEED, STEP, np.arange(N_ELEM), P.STREAM_XI1)
    assert z32.dtype == np.float32
    gap = float(np.abs(z32.astype(np.float64) - streams[(STEP, P.STREAM_XI1)]).max())
    print(f"max |normals_f32 - normals| = {gap:.3e} over {N_ELEM} counters")
    # r <= 5.77 and the angle 2 pi u <= 6.29 carries half an ulp of 8: 5.77 * 2.4e-7 * 2 plus a few ulp of z itself
    assert 0.0 < gap <= 1e-5


def test_noise_tensor_layout():
    a = P.noise_tensor(SEED, 3, 37, 17)
    b = P.noise_tensor(SEED, 3, 37, 17, srk=True)
    assert a.shape == (3, 37, 17) and b.shape == (3, 2, 37, 17)
    assert np.array_equal(b[:, 0], a) and not np.array_equal(b[:, 1], a)
    # a row's noise is a function of its position and the seed, not of the batch size
    assert np.array_equal(P.noise_tensor(SEED, 3, 300, 17)[:, :37], a)
    # element by element against the scalar definition
    for k, row, col in ((0, 0, 0), (2, 36, 16), (1, 17, 5)):
        e, c = P.tile_map(row, col)
        assert a[k, row, col] == P.normals(SEED, k, np.array([e]))[0, c]
