"""GPU (-m gpu): the noise the one-launch SDE samplers draw under noise="philox" (cfm_sde_em_mlp_f32,
cfm_sde_srk_mlp_f32; csrc/sde_small.h), element by element against the host restatement tests/philox_ref.py, which
tests/test_philox_host.py pins to the published known-answer vectors of Philox4x32-10.

Reading the kernel's own normals: with every parameter of the nets zero, y0 = 0, sigma = 1, ts = [0, 1] and dt = 1 the
Euler-Maruyama update is fma(1, z, fma(1, 0, 0)), so the returned state IS z, bit for bit; srk with zero nets has
k1 = k2 = k3 = 0 and returns xi1.  xi2 reaches the state only through a field, so it is compared on random fields
against the same entry run on the injected restatement (test_srk_xi2_...).

Tolerance: TOL = 4 max |normals_f32 - normals| over the counters a case draws — every lane of every tile of every step
and stream it uses, all four normals of each (a 16-row tile draws its 256 blocks whatever B and d leave live).  Both
sides of that difference are host restatements (float32 and float64 Box-Muller on the same 24-bit uniforms); nothing
of it comes from the device.  The factor 4: the device's logf, sincosf and sqrtf may be a couple of ulp where NumPy's
are within one, and r <= 5.77 multiplies the error of the angle.  Every test prints the device's gap beside its TOL.

Measured on the MI355X (the tests print their own): the device's normals are at most 1.34e-06 from the float64
restatement (B = 65541, TOL 6.45e-06); where TOL is smallest, 3.07e-06 (one tile), at most 7.1e-07.  The 12-step running
sums: at most 7.2e-07 against bounds of 1.7e-05 and 2.1e-05 (the step word shifted by one: 1.0 to 1.4 off).  srk on random
fields, Philox mode against the injected restatement: 7.2e-07 against a bound of 9.4e-05 (xi2 := xi1: 3.5e-02)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import philox_ref as P

pytestmark = pytest.mark.gpu

SEED = 123456789012345            # above 2^32: both key words are live
NONUNIFORM = [0.0, 0.13, 0.5, 1.0]
BIG = 16 * 4096 + 5               # one tile past the 4096-workgroup grid: workgroup 0 takes a second pass


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _zero_mlp(dev, d, w=16):
    """[d + 1, w, w, w, d] with every weight and bias zero: the field is 0 everywhere"""
    import cnf_restate as R
    dims = [d + 1, w, w, w, d]
    Ws = [np.zeros((b, a), dtype=np.float32) for a, b in zip(dims[:-1], dims[1:])]
    return R.make_mlp(Ws, [np.zeros(b, dtype=np.float32) for b in dims[1:]], dev)


def _random_pair(dev, d, w, seed):
    import cnf_restate as R
    return R.make_mlp(*R.mlp_params(d, w, seed), dev), R.make_mlp(*R.mlp_params(d, w, seed + 1), dev)


def _launch(dev, v, s, y0, ts, dt, g, seed, srk=False, xi=None, reverse=False, logqp=False):
    """The C entry itself on the grid of `ts` refined to `dt`, as cfm_amd.sde._run_one_launch marshals it, with the SEED
    the test's to choose.  g: a number, or one value per refined step.  s None: Ws = bs = NULL (the single-drift mode).
    Returns the trajectory after y0 [n_out, B, d] (and the log-ratio [n_out, B]) on the host."""
    from cfm_amd import _lib
    from cfm_amd import sde as S
    lib = _lib.load()
    steps = S._grid(ts, float(dt))
    g_steps = [float(g)] * len(steps) if isinstance(g, (int, float)) else [float(x) for x in g]
    assert len(g_steps) == len(steps)
    qw = S._logqp_weights(steps, g_steps, srk) if logqp else None
    blob, ws_bytes = S._packed_steps(steps, g_steps, srk, reverse, qw)
    host = (ctypes.c_char * ws_bytes).from_buffer_copy(blob)
    B, d = y0.shape
    n_out = sum(1 for st in steps if st[2])
    Wf, bf, cd, keep_f = v.hip_params(dev)
    Ws, bs, _, keep_s = s.hip_params(dev) if s is not None else (None, None, None, None)
    y = _lib.to_dev_f32(y0, dev)
    xid = _lib.to_dev_f32(xi, dev) if xi is not None else None
    out = torch.full((n_out * B * d + (n_out * B if logqp else 0),), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
    name = "cfm_sde_srk_mlp_f32" if srk else "cfm_sde_em_mlp_f32"
    flags = (1 if (reverse and s is not None) else 0) | (2 if logqp else 0)
    _lib.check(getattr(lib, name)(Wf, bf, Ws, bs, cd, 4, _lib.ptr(y), B, host, len(steps), flags, _lib.ptr(xid), seed,
                                  _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr()), name)
    torch.cuda.synchronize()
    traj = out[:n_out * B * d].view(n_out, B, d).cpu()
    return (traj, out[n_out * B * d:].view(n_out, B).cpu()) if logqp else traj


@functools.lru_cache(maxsize=None)
def _block_gap(seed, step, tiles, stream):
    elem = np.arange(tiles * 256)
    return float(np.abs(P.normals_f32(seed, step, elem, stream).astype(np.float64) - P.normals(seed, step, elem, stream)).max())


def _tol(seed, step_words, B, streams=(P.STREAM_XI1,)):
    """4 max |normals_f32 - normals| over every block the kernel draws for B rows at these step words and streams"""
    gap = max(_block_gap(seed, int(k), (B + 15) // 16, st) for k in step_words for st in streams)
    assert gap > 0.0
    return 4.0 * gap


def _gap(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max())


# ---------------------------------------------------------------------------------------------- a. every element ----
@pytest.mark.parametrize("d", [1, 2, 17, 64])
@pytest.mark.parametrize("B", [1, 16, 17, 300])
def test_every_normal_of_one_step_is_the_restatement_s(dev, B, d):
    """One step of h = 1 on zero nets from y0 = 0 at sigma = 1: the returned state is the kernel's z (module docstring).
    d = 17 and d = 64 put live columns in waves 1-3, B = 17 and B = 300 rows in a partial tile."""
    v, s = _zero_mlp(dev, d), _zero_mlp(dev, d)
    y0 = torch.zeros((B, d))
    want = P.noise_tensor(SEED, 1, B, d)[0]
    tol = _tol(SEED, [0], B)
    for what, got in (("em, two nets", _launch(dev, v, s, y0, [0.0, 1.0], 1.0, 1.0, SEED)),
                      ("em, one net", _launch(dev, v, None, y0, [0.0, 1.0], 1.0, 1.0, SEED)),
                      ("srk xi1", _launch(dev, v, s, y0, [0.0, 1.0], 1.0, 1.0, SEED, srk=True))):
        assert got.shape == (1, B, d)
        gap = _gap(got[0].numpy(), want)
        print(f"[philox] B={B} d={d} {what}: device gap {gap:.3e}, TOL {tol:.3e}")
        assert gap <= tol, (what, gap, tol)


# ---------------------------------------------------------------------------------------------- b. seed words ----
def test_both_seed_words_reach_the_key(dev):
    B, d = 33, 17
    v, s = _zero_mlp(dev, d), _zero_mlp(dev, d)
    y0 = torch.zeros((B, d))
    seeds = [0, 1, 2 ** 32, 2 ** 32 + 1, 2 ** 62 - 1]
    for srk in (False, True):
        outs = []
        for seed in seeds:
            got = _launch(dev, v, s, y0, [0.0, 1.0], 1.0, 1.0, seed, srk=srk)[0].numpy()
            tol = _tol(seed, [0], B)
            gap = _gap(got, P.noise_tensor(seed, 1, B, d)[0])
            print(f"[philox] srk={srk} seed={seed:#x}: device gap {gap:.3e}, TOL {tol:.3e}")
            assert gap <= tol, (seed, gap, tol)
            outs.append(got)
        for i in range(len(seeds)):
            for j in range(i + 1, len(seeds)):
                assert not np.array_equal(outs[i], outs[j]), (seeds[i], seeds[j])
                assert np.abs(outs[i] - outs[j]).max() > 1.0            # (far apart, not a rounding apart)


# ---------------------------------------------------------------------------------------------- c, d. step word ----
def _running_sum(seed, step_words, gs, is_out, B, d):
    """The state of zero nets from y0 = 0 as the kernel carries it, restated: y <- fl(y + fl(gs_k z_k)) in float32 with z_k
    the float64 restatement at counter word step_words[k]; the states after the output steps, [n_out, B, d] float64."""
    y = np.zeros((B, d), dtype=np.float32)
    out = []
    for word, g, o in zip(step_words, gs, is_out):
        if g != 0.0:
            y = (y + (np.float64(g) * P.step_normals(seed, word, B, d)).astype(np.float32)).astype(np.float32)
        if o:
            out.append(y.astype(np.float64))
    return np.stack(out)


def _records(ts, dt, g_steps):
    """(gs_k, is_out_k) as the kernel reads them: the float32 fields of cfm_amd.sde._em_records"""
    import struct
    from cfm_amd import sde as S
    steps = S._grid(ts, dt)
    blob = S._em_records(steps, g_steps, False)
    recs = [struct.unpack_from("<fffi", blob, 16 * k) for k in range(len(steps))]
    return [r[2] for r in recs], [r[3] for r in recs]


def _schedule(kind):
    import cfm_amd
    # cosine with sigma_min = 0: g(0) = 0 exactly, the first step draws nothing and adds nothing
    return {"constant": 0.8, "linear": cfm_amd.LinearDecreasingNoiseScheduler(0.1, 1.0),
            "cosine": cfm_amd.CosineNoiseScheduler(0.0, 0.5)}[kind]


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_the_step_word_is_the_index_into_the_refined_grid(dev, kind):
    """ts = linspace(0, 1, 4) at dt = 0.1: 12 steps, three of them outputs.  The states at the outputs are the float32
    running sum of gs_k z_k with z_k drawn at step word k, within n_steps TOL max gs; the same sum with the words shifted
    by one (k - 1), or all 0, misses that bound by more than 10x (the check has power).  kind: a constant sigma, and two
    built-in schedules whose g(t_k) differs per step (the cosine one has gs_0 = 0)."""
    from cfm_amd import sde as S
    B, d = 37, 17
    ts, dt = [float(x) for x in torch.linspace(0, 1, 4)], 0.1
    steps = S._grid(ts, dt)
    n = len(steps)
    assert n == 12 and sum(1 for st in steps if st[2]) == 3 and not steps[0][2]
    sig = _schedule(kind)
    g_steps = S._schedule_values(sig, steps) if callable(sig) else [sig] * n
    gs, is_out = _records(ts, dt, g_steps)
    assert max(gs) - min(gs) <= 1e-6 if kind == "constant" else len(set(gs)) >= n - 1
    assert (gs[0] == 0.0) == (kind == "cosine")
    v = _zero_mlp(dev, d)
    got = _launch(dev, v, _zero_mlp(dev, d), torch.zeros((B, d)), ts, dt, g_steps, SEED).numpy()
    one = _launch(dev, v, None, torch.zeros((B, d)), ts, dt, g_steps, SEED).numpy()
    assert np.array_equal(got, one)
    tol = _tol(SEED, range(n), B)
    bound = n * tol * max(gs)
    gap = _gap(got, _running_sum(SEED, list(range(n)), gs, is_out, B, d))
    shifted = _gap(got, _running_sum(SEED, [(k - 1) % 2 ** 32 for k in range(n)], gs, is_out, B, d))
    fixed = _gap(got, _running_sum(SEED, [0] * n, gs, is_out, B, d))
    print(f"[philox] {kind}: device gap {gap:.3e}, bound {bound:.3e} (TOL {tol:.3e}, max gs {max(gs):.4f}); "
          f"step - 1: {shifted:.3e}, step = 0: {fixed:.3e}")
    assert gap <= bound, (gap, bound)
    assert shifted > 10 * bound and fixed > 10 * bound
    if kind == "cosine":
        # nothing of step 0 in the first output: it is the sum over steps 1, 2, 3 alone
        assert _gap(got[:1], _running_sum(SEED, [1, 2, 3], gs[1:4], [0, 0, 1], B, d)) <= bound


# ---------------------------------------------------------------------------------------------- e. srk xi2 ----
def test_srk_xi2_is_the_second_stream_of_the_same_counters(dev):
    """xi2 enters the state through the third stage's field evaluation alone.  Two random w = 64 fields (seed 45,
    sigma = 1.0, start point (0.3, -0.2): the pair test_gpu_sde_srk.py::test_philox_xi2_is_independent_of_xi1 chose for
    its large Jacobian there), B = 300, d = 2, ts = (0, .13, .5, 1) at dt = 0.1 (11 steps): the entry in Philox mode
    against the same entry on the injected restatement [11, 2, 300, 2].  Bound: that file's 2e-5 max|ref| plus
    TOL sigma sum_k sqrt(h_k).  An injected tensor with plane 1 := plane 0, and one with plane 1 drawn at stream 0x5f2d
    (by construction the same tensor: same key, counter and stream words), each miss the bound by more than 10x."""
    import cfm_amd
    from cfm_amd import sde as S
    torch.manual_seed(45)
    v, s = (cfm_amd.MLP(dim=2, time_varying=True, w=64).to(dev) for _ in range(2))
    B, d, sigma, dt = 300, 2, 1.0, 0.1
    steps = S._grid(NONUNIFORM, dt)
    n = len(steps)
    assert n == 11
    y0 = torch.tensor([[0.3, -0.2]]).repeat(B, 1)
    got = _launch(dev, v, s, y0, NONUNIFORM, dt, sigma, SEED, srk=True).numpy()
    xi = P.noise_tensor(SEED, n, B, d, srk=True)
    assert xi.shape == (n, 2, B, d)
    ref = _launch(dev, v, s, y0, NONUNIFORM, dt, sigma, SEED + 1, srk=True, xi=torch.from_numpy(xi)).numpy()
    tol = _tol(SEED, range(n), B, (P.STREAM_XI1, P.STREAM_XI2))
    bound = 2e-5 * float(np.abs(ref).max()) + tol * sigma * sum(math.sqrt(h) for _, h, _ in steps)
    gap = _gap(got, ref.astype(np.float64))
    same = xi.copy()
    same[:, 1] = same[:, 0]
    first = xi.copy()
    first[:, 1] = np.stack([P.step_normals(SEED, k, B, d, P.STREAM_XI1) for k in range(n)])
    assert np.array_equal(same, first)
    bad = [_gap(got, _launch(dev, v, s, y0, NONUNIFORM, dt, sigma, 0, srk=True, xi=torch.from_numpy(t)).numpy().astype(np.float64))
           for t in (same, first)]
    print(f"[philox] srk xi2: device gap {gap:.3e}, bound {bound:.3e} (TOL {tol:.3e}, max|ref| {np.abs(ref).max():.3f}); "
          f"xi2 := xi1 {bad[0]:.3e}, xi2 at stream 0x5f2d {bad[1]:.3e}")
    assert gap <= bound, (gap, bound)
    assert min(bad) > 10 * bound, (bad, bound)


# ---------------------------------------------------------------------------------------------- f. public API ----
def _clone(g, dev):
    c = torch.Generator(device=dev)
    c.set_state(g.get_state())
    return c


def _seed_of(clone, dev):
    return int(torch.randint(0, 2 ** 62, (1,), device=dev, generator=clone).item())


@pytest.mark.parametrize("method", ["euler", "srk"])
def test_sdeint_seeds_the_kernel_with_the_generator_s_next_draw(dev, method):
    from cfm_amd.sde import FlowScoreSDE, sdeint
    B, d = 37, 17
    g = torch.Generator(device=dev).manual_seed(20261021)
    seed = _seed_of(_clone(g, dev), dev)
    sde = FlowScoreSDE(_zero_mlp(dev, d), _zero_mlp(dev, d), sigma=1.0)
    traj = sdeint(sde, torch.zeros((B, d), device=dev), torch.tensor([0.0, 1.0]), method=method, dt=1.0, noise="philox",
                  generator=g)
    assert sde.last_path == "hip" and traj.shape == (2, B, d) and not bool(traj[0].any())
    tol = _tol(seed, [0], B)
    gap = _gap(traj[1].cpu().numpy(), P.noise_tensor(seed, 1, B, d)[0])
    print(f"[philox] sdeint({method}) seed {seed:#x}: device gap {gap:.3e}, TOL {tol:.3e}")
    assert gap <= tol, (gap, tol)


def test_resample_pairs_draws_one_seed_per_half(dev):
    """DSBMFlowSolver.resample_pairs on zero nets at constant sigma = 1, dt = 1: the forward half is seeded by the
    generator's first draw and the backward half by its second, each on the rows of its own batch (75 rows: 37 + 38)."""
    import cfm_amd
    from cfm_amd.utils import torch_wrapper
    B, d = 75, 5
    half = B // 2
    solver = cfm_amd.DSBMFlowSolver(torch_wrapper(_zero_mlp(dev, d)), d, score_field=torch_wrapper(_zero_mlp(dev, d)),
                                    sigma=cfm_amd.ConstantNoiseScheduler(1.0), dt=1.0)
    g = torch.Generator(device=dev).manual_seed(77)
    clone = _clone(g, dev)
    s1, s2 = _seed_of(clone, dev), _seed_of(clone, dev)
    assert s1 != s2
    zeros = torch.zeros((B, d), device=dev)
    pairs = solver.resample_pairs(zeros, zeros, generator=g).cpu().numpy()
    assert solver.last_path == "hip" and pairs.shape == (B, 2, d)
    assert not pairs[:half, 0].any() and not pairs[half:, 1].any()              # the ends the solves started from
    for what, got, seed, rows in (("forward", pairs[:half, 1], s1, half), ("backward", pairs[half:, 0], s2, B - half)):
        tol = _tol(seed, [0], rows)
        gap = _gap(got, P.noise_tensor(seed, 1, rows, d)[0])
        other = _gap(got, P.noise_tensor(s2 if seed == s1 else s1, 1, rows, d)[0])
        print(f"[philox] resample_pairs {what} half, seed {seed:#x}: device gap {gap:.3e}, TOL {tol:.3e} (other seed: {other:.3e})")
        assert gap <= tol, (what, gap, tol)
        assert other > 1.0


# ---------------------------------------------------------------------------------------------- g. position ----
@pytest.mark.parametrize("method", ["euler", "srk"])
@pytest.mark.parametrize("logqp", [False, True], ids=["plain", "logqp"])
def test_a_row_s_noise_depends_on_its_position_not_on_the_batch(dev, method, logqp):
    """Real nets, the same seed, B = 300 and B = 77 (a partial fifth tile): rows 0 ... 76 of the trajectories are
    bit-equal, and of the log-ratio under logqp."""
    from cfm_amd.sde import FlowScoreSDE, sdeint
    d = 5
    v, s = _random_pair(dev, d, (33, 16, 24), seed=7)
    x0 = torch.randn((300, d), generator=torch.Generator().manual_seed(8)).to(dev)
    sde = FlowScoreSDE(v, s, sigma=0.6)
    run = lambda x: sdeint(sde, x, torch.tensor(NONUNIFORM), method=method, dt=0.1, noise="philox", fused=True, logqp=logqp,
                           generator=torch.Generator(device=dev).manual_seed(5))
    a, b = run(x0), run(x0[:77].contiguous())
    assert sde.last_path == "hip"
    if logqp:
        (a, la), (b, lb) = a, b
        assert la.shape == (3, 300) and lb.shape == (3, 77) and torch.equal(la[:, :77], lb)
    assert a.shape == (4, 300, d) and b.shape == (4, 77, d)
    assert torch.equal(a[:, :77], b)
    assert not torch.equal(a[-1, :77], a[-1, 77:154])


# ---------------------------------------------------------------------------------------------- h. second pass ----
@pytest.mark.parametrize("srk", [False, True], ids=["em", "srk"])
def test_the_second_grid_pass_draws_the_next_tile_s_counters(dev, srk):
    """B = 16 * 4096 + 5 on zero nets, one step: the grid is capped at 4096 workgroups, so workgroup 0 also runs tile
    4096.  Its rows 65536 ... match the restatement at elem = 4096 * 256 + tid, and are not the normals of rows 0 ... 4
    (what elem = tid alone would give)."""
    d = 2
    v, s = _zero_mlp(dev, d), _zero_mlp(dev, d)
    got = _launch(dev, v, s, torch.zeros((BIG, d)), [0.0, 1.0], 1.0, 1.0, SEED, srk=srk)[0].numpy()
    tol = _tol(SEED, [0], BIG)
    gap = _gap(got, P.noise_tensor(SEED, 1, BIG, d)[0])
    # the tail by its definition: lane index (r // 4) * 16 + col, component r % 4, in tile 4096
    tail = np.empty((5, d))
    for r in range(5):
        for c in range(d):
            tail[r, c] = P.normals(SEED, 0, np.array([4096 * 256 + (r // 4) * 16 + c]))[0, r % 4]
    tail_gap = _gap(got[65536:], tail)
    print(f"[philox] srk={srk} B={BIG}: device gap {gap:.3e} (tail rows {tail_gap:.3e}), TOL {tol:.3e}")
    assert gap <= tol and tail_gap <= tol, (gap, tail_gap, tol)
    assert np.abs(got[65536:] - got[:5]).max() > 1.0
    assert not np.array_equal(got[65536 - 16:65536], got[:16])
