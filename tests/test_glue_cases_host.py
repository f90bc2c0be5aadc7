"""CPU: the references of tests/glue_cases.py are what tests/test_gpu_glue_kernels.py takes them for.

  * the dyadic plans are exact: integer multiples of 2^-30, a power-of-two total (per row for the per-row plans), and
    np.cumsum forwards, backwards and NumPy's pairwise sum give the same total bit for bit; the zero layout is there;
  * the step draws sit ON the cdf steps, one ulp below and one ulp above them, inside [0, 1);
  * the search reference equals np.random.choice on the same stream (off the steps, and, the totals being powers of two,
    on them as well); the restated replace=False loop equals np.random.choice(replace=False) and runs several rounds;
  * the permutation reference equals oracle.sample_perm_given_u for power-of-two B;
  * the one-rounding-at-a-time float32 Schrodinger-bridge reference equals oracle.xt_ut("sb") wherever torch's CPU sqrt
    agrees with the correctly rounded one;
  * the float64 RBF / MMD restatements agree with the obvious dense formulas, and the case tables hold the sizes the
    GPU tests name (above each grid cap)."""
import numpy as np
import pytest
import torch

import cfm_oracle as oracle
import glue_cases as cases


# ----------------------------------------------------------------------------------------------- dyadic plans
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("B0,B1", cases.PLAN_SHAPES)
def test_dyadic_plans_are_exact(B0, B1, per_row):
    P = cases.dyadic_plan(B0, B1, per_row=per_row)
    W = P / cases.UNIT
    assert P.shape == (B0, B1) and P.dtype == np.float64
    assert np.array_equal(W, np.round(W)) and W.min() >= 0 and W.sum() < 2 ** 40
    big = W > 2 ** 10                                           # only closing entries may exceed 2^10
    assert big.sum() <= (B0 if per_row else 1)
    for p in ([P[r] for r in range(B0) if P[r].any()] if per_row else [P.ravel()]):
        fwd, bwd, pair = np.cumsum(p)[-1], np.cumsum(p[::-1])[-1], np.sum(p)
        assert fwd == bwd == pair and cases.is_pow2(fwd), (fwd, bwd, pair)
    # and in a random order
    q = np.random.default_rng(0).permutation(P.ravel())
    assert np.cumsum(q)[-1] == np.sum(P)


@pytest.mark.parametrize("B0,B1", cases.PLAN_SHAPES)
def test_dyadic_plan_zero_layout(B0, B1):
    P = cases.dyadic_plan(B0, B1)
    empty = [r for r in range(B0) if not P[r].any()]
    if B0 >= 5:
        assert {0, B0 // 2, B0 - 1} <= set(empty)
        assert {r for r in (1023, 1024, 2047, 2048) if r < B0} <= set(empty)
    else:
        assert not empty
    if B0 >= 3:
        assert np.flatnonzero(P[cases.SPECIAL_ROW]).tolist() == [B1 - 1]
    if B1 >= 5:
        others = np.delete(P, cases.SPECIAL_ROW, axis=0) if B0 >= 3 else P
        assert not others[:, [0, 1, B1 - 1]].any()
    assert all(P[r].any() for r in range(B0) if r not in empty)
    if B0 * B1 > 64:
        assert (P == 0).mean() > 0.2                            # scattered interior zeros: repeated cdf values


@pytest.mark.parametrize("B0,B1", cases.PLAN_SHAPES)
def test_step_draws_sit_on_and_next_to_the_steps(B0, B1):
    P = cases.dyadic_plan(B0, B1)
    u = cases.step_draws(P.ravel())
    T = P.sum()
    cdf = np.cumsum(P.ravel())
    assert ((u >= 0) & (u < 1)).all() and 0.0 in u and np.nextafter(1.0, 0.0) in u
    on = np.isin(u * T, cdf) & (u > 0)                          # u * T is exact: T is a power of two
    n_steps = np.unique(cdf[cdf > 0]).size
    assert on.sum() == min(n_steps, cases.MAX_STEPS) - 1        # every step but the last (u = 1 is no draw)
    assert np.isin(np.nextafter(u[on], 0.0), u).all() and np.isin(np.nextafter(u[on], 2.0), u).all()
    if n_steps <= cases.MAX_STEPS:
        assert np.isin(np.unique(cdf[(cdf > 0) & (cdf < T)]) / T, u).all()
    # side="right": a draw ON step k belongs to the NEXT entry carrying mass, one ulp below it to entry k itself
    k = cases.searchsorted_ref(P, u[on])
    assert (cdf[k] > u[on] * T).all() and (P.ravel()[k] > 0).all()
    assert (cdf[k - 1][k > 0] <= (u[on] * T)[k > 0]).all()
    below = cases.searchsorted_ref(P, np.nextafter(u[on], 0.0))
    assert (below < k).all()


@pytest.mark.parametrize("B0,B1", cases.PLAN_SHAPES)
def test_search_reference_equals_numpy_choice(B0, B1):
    P = cases.dyadic_plan(B0, B1)
    p = (P / P.sum()).ravel()
    for n in cases.DRAW_COUNTS:
        np.random.seed(B0 + B1 + n)
        ref = np.random.choice(B0 * B1, p=p, size=n)
        np.random.seed(B0 + B1 + n)
        u = np.random.random_sample(n)                          # off the steps (with probability one)
        assert np.array_equal(cases.searchsorted_ref(P, u), ref)
    # on the steps: np.random.choice's own arithmetic (cdf = cumsum(p); cdf /= cdf[-1]; searchsorted right) is exact here too
    u = cases.step_draws(P.ravel())
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    assert np.array_equal(cdf.searchsorted(u, side="right"), cases.searchsorted_ref(P, u))
    i, j = cases.sample_pi_ref(P, u)
    io, jo = oracle.sample_map_given_u(P, u)
    assert np.array_equal(i, io) and np.array_equal(j, jo)


@pytest.mark.parametrize("B0,B1", cases.PLAN_SHAPES)
def test_row_reference_equals_numpy_choice_per_row(B0, B1):
    P = cases.dyadic_plan(B0, B1, per_row=True)
    rows, u = cases.row_step_cases(P)
    assert len(rows) == len(u) and ((u >= 0) & (u < 1)).all()
    ref = cases.sample_rows_ref(P, rows, u)
    for r in np.unique(rows):
        sel = rows == r
        if not P[r].any():
            assert (ref[sel] == B1 - 1).all()
            continue
        cdf = np.cumsum(P[r] / P[r].sum())
        cdf /= cdf[-1]
        assert np.array_equal(ref[sel], cdf.searchsorted(u[sel], side="right"))
        assert (P[r][ref[sel]] > 0).all()
    # clamped rows
    uu = np.array([0.0, 0.3, np.nextafter(1.0, 0.0)])
    lo = cases.sample_rows_ref(P, np.full(3, -7), uu)
    hi = cases.sample_rows_ref(P, np.full(3, B0 + 5), uu)
    assert np.array_equal(lo, cases.sample_rows_ref(P, np.zeros(3, dtype=np.int64), uu))
    assert np.array_equal(hi, cases.sample_rows_ref(P, np.full(3, B0 - 1), uu))


# ----------------------------------------------------------------------------------------------- permutation plans
@pytest.mark.parametrize("B", [1, 2, 64, 4096])
def test_perm_reference_equals_oracle_for_power_of_two(B):
    assert B in cases.PERM_SIZES or B in (2, 64)
    perm = np.random.default_rng(B).permutation(B)
    u = cases.perm_step_draws(B)
    i, j = cases.sample_perm_ref(perm, u)
    io, jo = oracle.sample_perm_given_u(perm, u)
    assert np.array_equal(i, io) and np.array_equal(j, jo)


@pytest.mark.parametrize("B", cases.PERM_SIZES)
def test_perm_reference_is_the_stated_definition(B):
    u = cases.perm_step_draws(B)
    assert u.size >= min(3 * B - 1, 3) and ((u >= 0) & (u < 1)).all()
    i, _ = cases.sample_perm_ref(np.arange(B), u)
    hi = (i + 1).astype(np.float64) / np.float64(B)
    lo = i.astype(np.float64) / np.float64(B)
    assert (hi > u).all() and (lo[i > 0] <= u[i > 0]).all() and i.min() == 0 and i.max() == B - 1
    # off the steps it is np.random.choice on the uniform plan
    np.random.seed(B)
    ref = np.random.choice(B, p=np.full(B, 1.0 / B) / np.full(B, 1.0 / B).sum(), size=300)
    np.random.seed(B)
    assert np.array_equal(cases.sample_perm_ref(np.arange(B), np.random.random_sample(300))[0], ref)


def test_no_replace_restatement_equals_numpy_and_runs_several_rounds():
    P, perm = cases.perm_plan_dyadic(64)
    assert cases.is_pow2(P.sum()) and np.count_nonzero(P) == 64
    assert np.array_equal(np.nonzero(P)[1], perm)
    p = (P / P.sum()).ravel()
    np.random.seed(11)
    ref = np.random.choice(64 * 64, p=p, size=64, replace=False)
    after = np.random.random_sample()
    np.random.seed(11)
    got, rounds = cases.choice_noreplace(p, 64, np.random.random_sample)
    assert np.array_equal(got, ref) and np.random.random_sample() == after
    assert rounds >= 3, rounds
    assert sorted(np.divmod(got, 64)[0].tolist()) == list(range(64))


# ----------------------------------------------------------------------------------------------- x_t / u_t
def test_xt_inputs_reach_the_ends_of_the_clouds():
    x0, x1, eps, t, i, j = cases.xt_inputs(96, 8, n0=300, n1=41)
    assert x0.shape == (300, 8) and x1.shape == (41, 8) and eps.shape == (96, 8) and t.shape == (96,)
    assert i.max() == 299 and i.min() == 0 and j.max() == 40 and j.min() == 0
    assert all(a.dtype == np.float32 for a in (x0, x1, eps, t)) and ((t >= 0) & (t < 1)).all()
    assert np.array_equal(t.astype(np.float64) * 2 ** 24, np.round(t.astype(np.float64) * 2 ** 24))
    # the grid-stride shapes of the GPU test exceed the 8192 * 256 work items of one sweep
    assert 2051 * 4100 // 4 > 8192 * 256 and 2051 * 1023 > 8192 * 256 and 4100 % 4 == 0 and 1023 % 4 != 0


def test_sb_float32_reference_equals_oracle_where_the_sqrts_agree():
    t = cases.sb_t_grid()
    assert t.size == 4099 and t[-3] == 0.0 and t[-2] == 0.5 and t[-1] == np.float32(1.0 - 2.0 ** -24)
    assert (t[:-3] >= 2.0 ** -24).all() and (t < 1).all()
    rng = np.random.default_rng(0)
    B, d, sigma = t.size, 3, 0.5
    x0, x1, eps = (rng.standard_normal((B, d), dtype=np.float32) for _ in range(3))
    tt = torch.from_numpy(t)
    sig_torch = (sigma * torch.sqrt(tt * (1 - tt))).numpy()
    sig_np = cases.sb_sigma_t_f32(t, sigma)
    # np.sqrt on float32 is correctly rounded: it equals the rounding of the float64 root (float64 carries more than
    # 2 * 24 + 2 bits, so the double rounding is innocuous)
    prod = t * (np.float32(1) - t)
    assert np.array_equal(np.sqrt(prod), np.sqrt(prod.astype(np.float64)).astype(np.float32))
    agree = sig_torch == sig_np
    print(f"torch CPU sqrt agrees with the correctly rounded one on {agree.mean():.4%} of {B} values")
    assert agree.mean() > 0.9
    xo, uo = oracle.xt_ut("sb", torch.from_numpy(x0), torch.from_numpy(x1), tt, torch.from_numpy(eps), sigma)
    xr, ur = cases.sb_ref_f32(x0, x1, t, eps, sigma)
    assert np.array_equal(xr[agree], xo.numpy()[agree]) and np.array_equal(ur[agree], uo.numpy()[agree])
    # with torch's own scales handed over (what the Python wrapper does) every row agrees
    xr, ur = cases.sb_ref_f32(x0, x1, t, eps, sigma, sig_t=sig_torch)
    assert np.array_equal(xr, xo.numpy()) and np.array_equal(ur, uo.numpy())
    assert np.isfinite(ur).all()


# ----------------------------------------------------------------------------------------------- Adam, RBF, cost tails
def test_adam_case_table():
    n = cases.ADAM_NUMELS
    assert len(n) == 40 > 2 * 16                                 # more tensors than grid rows, in each group of 20
    assert {1, 255, 256, 257, 65535, 65536, 65537, 70001} <= set(n)
    assert max(n) > 256 * 256                                    # above one x-sweep (256 blocks of 256)
    assert any(1 - b1 >= 0.5 for b1, _ in cases.ADAM_BETAS) and any(1 - b1 < 0.5 for b1, _ in cases.ADAM_BETAS)


def test_rbf_references():
    g = cases.rbf_gammas(cases.RBF_SIGMAS)
    assert g.dtype == np.float32 and np.allclose(g, [5000, 50, 0.5, 0.005, 0.00005])
    assert max(cases.RBF_SIZES) > 2048 * 256
    for n in cases.RBF_SIZES:
        D = cases.rbf_distances(n)
        assert D.dtype == np.float32 and D.shape == (n,) and (D >= 0).all() and np.isfinite(D).all()
        if n >= 255:
            assert (D == 0).any() and (np.abs(D - 1) < 2e-3).any()
            assert (np.exp(-float(g.min()) * D.astype(np.float64)) < 1e-45).any()     # every term below fp32's smallest
        dense = np.exp(-np.outer(D.astype(np.float64), g.astype(np.float64))).sum()
        assert abs(cases.rbf_sum_f64(D, g) - dense) <= 1e-12 * dense
        assert cases.rbf_sum_f64(D, g[:1]) <= cases.rbf_sum_f64(D, g)


def test_mmd_reference():
    X, Y = cases.mmd_clouds(300, 8)
    val, sums = cases.mmd2_ref(X, Y, cases.RBF_SIGMAS)
    assert val > 0 and all(s > 0 for s in sums)
    same, _ = cases.mmd2_ref(X, X, cases.RBF_SIGMAS)
    assert same == 0.0
    # the symmetric V-statistic written out
    K = lambda A, B: sum(np.exp(-cases.sqdist_f64(A, B) / (2.0 * s * s)) for s in cases.RBF_SIGMAS)
    direct = K(X, X).mean() + K(Y, Y).mean() - 2 * K(X, Y).mean()
    assert abs(val - direct) <= 1e-12
    assert 0 < cases.mmd2_abs_bound(sums, 300, 8, 5) < 1e-4


@pytest.mark.parametrize("max_at", ["first", "last"])
def test_cost_tail_clouds_put_the_maximum_where_they_say(max_at):
    B0, B1, d = cases.COST_TAIL_SHAPE
    assert B0 * B1 > 4096 * 256
    x0, x1 = cases.cost_tail_clouds(max_at)
    M = cases.sqdist_f64(x0, x1)
    at = np.unravel_index(M.argmax(), M.shape)
    assert at == ((0, 0) if max_at == "first" else (B0 - 1, B1 - 1))
    assert M.max() > 1.5 * np.partition(M.ravel(), -2)[-2]
