"""Case table of tests/test_gpu_glue_kernels.py and tests/test_glue_cases_host.py: inputs and plain NumPy references for the
small once-per-step kernels (csrc/sample.hip, csrc/elem.hip, the Adam launch of csrc/mlp_train.hip, the elementwise tails
of csrc/cost.hip) at the shapes where their code takes another branch.  NumPy only: no device, no library.

Dyadic plans.  Every entry is an integer times 2^-30 (integers in [0, 2^10], except the one closing entry that brings the
total, or each row's total, up to a power of two); the integer totals stay far below 2^53, so EVERY partial sum, in any
order, is exact in float64, and so are u * T and cdf_k / T for a power-of-two T.  A device search on such a plan has no
rounding to hide behind: it must return searchsorted(cumsum(P), u * T, side="right"), index for index, also for u ON a
cdf step (where `>` against `>=` decides) and one ulp on either side of it.

Zero layout of dyadic_plan (what applies at a shape):
  B0 >= 5   rows 0, B0 // 2 and B0 - 1 empty; rows 1023, 1024, 2047, 2048 empty where they exist (the 1024-row chunk of
            the row scan and its carry)
  B0 >= 3   row SPECIAL_ROW = 1 carries its whole mass in column B1 - 1
  B1 >= 5   columns 0, 1 and B1 - 1 empty in every other row (leading / trailing empty columns)
  plus ~30 % zeros scattered over the rest; every other row keeps at least one entry.
"""
import functools

import numpy as np

UNIT = 2.0 ** -30
SPECIAL_ROW = 1

PLAN_SHAPES = [(1, 1), (1, 130), (5, 1), (3, 63), (3, 64), (3, 65), (1023, 2), (1024, 2), (1025, 2), (2049, 3), (2, 4097)]
DRAW_COUNTS = [0, 1, 3, 5, 515]            # sd_sample / sd_sample_rows: 4 draws per workgroup
MAX_STEPS = 512                            # cdf steps sampled of a large case (every step of a small one)
PERM_SIZES = [1, 3, 7, 100, 1000, 1023, 4096]


def _empty_rows(B0):
    rows = set()
    if B0 >= 5:
        rows |= {0, B0 // 2, B0 - 1}
        rows |= {r for r in (1023, 1024, 2047, 2048) if r < B0}
    return sorted(rows)


def _pow2_above(s):
    """Smallest power of two > s (s a non-negative integer)."""
    return 1 << int(s).bit_length()


@functools.lru_cache(maxsize=None)
def _dyadic_ints(B0, B1):
    rng = np.random.default_rng(1000 * B0 + B1)
    W = rng.integers(1, 2 ** 10 + 1, size=(B0, B1)).astype(np.int64)
    W[rng.random((B0, B1)) < 0.3] = 0
    cols = np.arange(B1)
    live = np.ones(B1, dtype=bool)
    if B1 >= 5:
        live[[0, 1, B1 - 1]] = False
    W[:, ~live] = 0
    empty = _empty_rows(B0)
    for r in range(B0):
        if r in empty:
            W[r] = 0
        elif B0 >= 3 and r == SPECIAL_ROW:
            W[r] = 0
            W[r, B1 - 1] = int(rng.integers(1, 2 ** 10 + 1))
        elif not W[r].any():
            W[r, int(rng.choice(cols[live]))] = int(rng.integers(1, 2 ** 10 + 1))
    W.setflags(write=False)
    return W


def dyadic_plan(B0, B1, per_row=False):
    """float64 [B0, B1] plan as described in the module docstring.  per_row=False: the LAST non-zero entry (row-major) is
    set so that the total is a power of two; per_row=True: the last non-zero entry of every non-empty row is set so that
    the row's total is a power of two (the plan of sample_rows_pi: u * T_row exact for every row)."""
    W = _dyadic_ints(B0, B1).copy()
    if per_row:
        for r in range(B0):
            nz = np.flatnonzero(W[r])
            if nz.size:
                rest = int(W[r].sum() - W[r, nz[-1]])
                W[r, nz[-1]] = _pow2_above(rest) - rest
    else:
        flat = W.reshape(-1)
        nz = np.flatnonzero(flat)
        rest = int(flat.sum() - flat[nz[-1]])
        flat[nz[-1]] = _pow2_above(rest) - rest
    return W.astype(np.float64) * UNIT


def is_pow2(x):
    m, _ = np.frexp(x)
    return bool(x > 0 and m == 0.5)


def step_draws(p, seed=0, max_steps=MAX_STEPS):
    """Uniforms that sit on, just below and just above the cdf steps of the 1-D weights `p` (total a power of two):
    {cdf_k / T} for every distinct step (MAX_STEPS sampled ones, first and last step included, of a long cdf),
    nextafter of each in both directions, 0.0 and nextafter(1, 0); kept inside [0, 1) like random_sample()'s."""
    cdf = np.unique(np.cumsum(p))
    cdf = cdf[cdf > 0]
    T = cdf[-1]
    assert is_pow2(T)
    if cdf.size > max_steps:
        rng = np.random.default_rng(seed)
        pick = rng.choice(np.arange(1, cdf.size - 1), size=max_steps - 2, replace=False)
        cdf = cdf[np.sort(np.r_[0, pick, cdf.size - 1])]
    u = cdf / T
    u = np.r_[u, np.nextafter(u, 0.0), np.nextafter(u, 2.0), 0.0, np.nextafter(1.0, 0.0)]
    return u[(u >= 0.0) & (u < 1.0)]


def shuffled(u, seed=0):
    return np.random.default_rng(seed).permutation(u)


def searchsorted_ref(p, u):
    """np.random.choice's index for the uniforms u on the weights p, without its renormalisation:
    searchsorted(cumsum(p), u * sum(p), side="right")."""
    p = np.asarray(p, dtype=np.float64).ravel()
    c = np.cumsum(p)
    return np.searchsorted(c, np.asarray(u, dtype=np.float64) * c[-1], side="right")


def sample_pi_ref(P, u):
    return np.divmod(searchsorted_ref(P, u), P.shape[1])


def sample_rows_ref(P, rows, u):
    """Per draw k: column drawn by u[k] from row rows[k] of P, rows clamped into [0, B0); a row without mass gives B1 - 1
    (the kernel's documented fallback; numpy raises there)."""
    B0, B1 = P.shape
    out = np.empty(len(rows), dtype=np.int64)
    for k, (r, uk) in enumerate(zip(rows, u)):
        row = P[min(max(int(r), 0), B0 - 1)]
        out[k] = searchsorted_ref(row, [uk])[0] if row.sum() > 0 else B1 - 1
    return out


def row_step_cases(P, seed=0, max_rows=24, max_steps=16):
    """(rows, u) for sample_rows_pi: for a selection of rows (all of a short plan; else the first / last rows, the special
    row, the neighbours of the 1024-row boundaries and random ones) the on / below / above-step uniforms of that row; an
    empty row gets 0.0, 0.5 and nextafter(1, 0)."""
    B0, _ = P.shape
    if B0 <= max_rows:
        sel = list(range(B0))
    else:
        rng = np.random.default_rng(seed)
        fixed = [0, 1, 2, B0 // 2, B0 - 2, B0 - 1] + [r for r in (1022, 1023, 1024, 1025) if r < B0]
        sel = sorted(set(fixed) | set(int(r) for r in rng.choice(B0, size=max_rows - len(set(fixed)), replace=False)))
    rows, us = [], []
    for r in sel:
        u = step_draws(P[r], seed=seed + r, max_steps=max_steps) if P[r].sum() > 0 \
            else np.array([0.0, 0.5, np.nextafter(1.0, 0.0)])
        rows.append(np.full(u.size, r, dtype=np.int64))
        us.append(u)
    return np.concatenate(rows), np.concatenate(us)


# --------------------------------------------------------------------------- permutation plans
def perm_step_draws(B):
    """k / B for every k < B (float64 division), its two neighbours, 0.0 and nextafter(1, 0), inside [0, 1)."""
    u = np.arange(B, dtype=np.float64) / np.float64(B)
    u = np.r_[u, np.nextafter(u, -1.0), np.nextafter(u, 2.0), 0.0, np.nextafter(1.0, 0.0)]
    return u[(u >= 0.0) & (u < 1.0)]


def sample_perm_ref(perm, u):
    """sample_perm_kernel's stated definition: i = the first m with (m + 1) / B > u, in float64; j = perm[i].
    (m + 1) / B is non-decreasing in m, so the first such m is a right-sided search.)"""
    B = len(perm)
    steps = np.arange(1, B + 1, dtype=np.float64) / np.float64(B)
    i = np.searchsorted(steps, u, side="right").astype(np.int64)
    return i, np.asarray(perm, dtype=np.int64)[i]


def perm_plan_dyadic(B, seed=0):
    """A permutation-like dyadic plan: one entry per row and column, integer weights, total a power of two."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(B)
    w = rng.integers(1, 2 ** 10 + 1, size=B).astype(np.int64)
    rest = int(w[:-1].sum())
    w[-1] = _pow2_above(rest) - rest
    P = np.zeros((B, B), dtype=np.float64)
    P[np.arange(B), perm] = w * UNIT
    return P, perm


def choice_noreplace(p, size, rand):
    """numpy's legacy RandomState.choice(len(p), p=p, size=size, replace=False), restated; `rand(n)` draws n uniforms.
    Returns (indices, number of rounds of the rejection loop)."""
    p = np.array(p, dtype=np.float64)
    found = np.zeros(size, dtype=np.int64)
    n_uniq = rounds = 0
    while n_uniq < size:
        x = rand(size - n_uniq)
        if n_uniq > 0:
            p[found[:n_uniq]] = 0
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        new = cdf.searchsorted(x, side="right")
        _, first = np.unique(new, return_index=True)
        first.sort()
        new = new.take(first)
        found[n_uniq:n_uniq + new.size] = new
        n_uniq += new.size
        rounds += 1
    return found, rounds


# --------------------------------------------------------------------------- x_t / u_t
VARIANTS = {"icfm": 0, "sb": 1, "target": 2, "vp": 3}


def variant_sigmas(method):
    return (0.5,) if method == "sb" else (0.5, 0.0)


@functools.lru_cache(maxsize=4)
def xt_inputs(B, d, n0=None, n1=None, seed=0):
    """float32 clouds x0 [n0, d], x1 [n1, d] (default B rows), eps [B, d], t [B] on torch.rand's grid (k * 2^-24), and
    int64 gathers i, j of length B that reach the first and the last row of each cloud."""
    n0, n1 = n0 or B, n1 or B
    rng = np.random.default_rng(seed + 31 * B + d)
    x0 = rng.standard_normal((n0, d), dtype=np.float32)
    x1 = rng.standard_normal((n1, d), dtype=np.float32) + np.float32(0.25)
    eps = rng.standard_normal((B, d), dtype=np.float32)
    t = (rng.integers(0, 2 ** 24, size=B).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    i, j = rng.integers(0, n0, size=B), rng.integers(0, n1, size=B)
    i[0], i[-1], j[0], j[-1] = n0 - 1, 0, 0, n1 - 1
    out = (x0, x1, eps, t, i.astype(np.int64), j.astype(np.int64))
    for a in out:
        a.setflags(write=False)
    return out


def sb_t_grid(n=4096, seed=7):
    """n values k * 2^-24 (k >= 1: no zero among the random ones, and torch.rand cannot give a subnormal), then the
    edges 0, 0.5 and 1 - 2^-24."""
    k = np.random.default_rng(seed).integers(1, 2 ** 24, size=n).astype(np.float64)
    t = np.r_[k * 2.0 ** -24, 0.0, 0.5, 1.0 - 2.0 ** -24]
    return t.astype(np.float32)


def sb_sigma_t_f32(t, sigma):
    """sigma * sqrt(t * (1 - t)) in float32, one rounded operation at a time (np.sqrt is correctly rounded)."""
    t = np.asarray(t, dtype=np.float32)
    one = np.float32(1.0)
    return np.float32(sigma) * np.sqrt(t * (one - t))


def sb_ref_f32(x0, x1, t, eps, sigma, sig_t=None):
    """The Schrodinger-bridge x_t / u_t of csrc/elem.hip in float32, one rounded operation at a time, in the kernel's
    (= the reference's) order.  sig_t: the [B] noise scales to use instead of this file's own sqrt."""
    f = np.float32
    x0, x1, eps = (np.asarray(a, dtype=f) for a in (x0, x1, eps))
    t = np.asarray(t, dtype=f)[:, None]
    one, two = f(1.0), f(2.0)
    omt = one - t
    sig = (sb_sigma_t_f32(t[:, 0], sigma) if sig_t is None else np.asarray(sig_t, dtype=f))[:, None]
    two_t = two * t
    a = (one - two_t) / (two_t * omt + f(1e-8))
    mu = t * x1 + omt * x0
    xt = mu + sig * eps
    ut = (a * (xt - mu) + x1) - x0
    assert xt.dtype == f and ut.dtype == f
    return xt, ut


# --------------------------------------------------------------------------- Adam
ADAM_NUMELS = [1, 255, 256, 257, 65535, 65536, 65537, 70001,
               2, 3, 7, 63, 64, 65, 127, 128, 129, 191, 511, 512, 513, 777, 1000, 1023, 1024, 1025, 2047, 2049, 3001,
               4095, 4096, 4097, 5000, 6001, 8191, 8192, 8193, 10000, 12345, 16385]
ADAM_GROUPS = [dict(lr=2e-4, weight_decay=0.0), dict(lr=1e-3, weight_decay=0.01)]     # first / second 20 tensors
ADAM_BETAS = [(0.9, 0.999), (0.8, 0.99), (0.5, 0.999), (0.0, 0.9)]
ADAM_EPS = [1e-8, 1e-3]
ADAM_STEPS = 20
assert len(ADAM_NUMELS) == 40 and len(set(ADAM_NUMELS)) == 40


# --------------------------------------------------------------------------- RBF sums
RBF_SIGMAS = [0.01, 0.1, 1, 10, 100]       # the runner's list (distribution_distances.py)
RBF_SIZES = [1, 255, 256, 257, 725 * 725]  # 525 625 > 2048 * 256: the grid stride of rbf_mix_sum_kernel
RBF_RTOL = 1e-6


def rbf_gammas(sigmas):
    return np.array([1.0 / (2.0 * s * s) for s in sigmas], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def rbf_distances(n, seed=0):
    """float32 'squared distances': a chi-square-like bulk on many scales, exact zeros, values next to 1, and values
    at which every term of the mixture underflows (gamma_min * D > 104 needs D > 2.1e6 at sigma = 100)."""
    rng = np.random.default_rng(seed + n)
    D = (rng.standard_normal(n) ** 2 * 10.0 ** rng.integers(-6, 5, size=n)).astype(np.float32)
    k = np.arange(n)
    D[k % 7 == 0] = 0.0
    D[k % 7 == 1] = (1.0 + rng.uniform(-1e-3, 1e-3, size=n)).astype(np.float32)[k % 7 == 1]
    D[k % 7 == 2] = np.float32(1e9)
    D[k % 7 == 3] = np.float32(3.0e38)
    D.setflags(write=False)
    return D


def rbf_sum_f64(D, gammas):
    """sum_e sum_q exp(-gamma_q * D_e) in float64 on the SAME float32 D and float32 gammas."""
    D = np.asarray(D, dtype=np.float64).ravel()
    tot = 0.0
    for gq in np.asarray(gammas, dtype=np.float32):
        tot += float(np.exp(-np.float64(gq) * D).sum())
    return tot


def sqdist_f64(X, Y):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    D = np.zeros((X.shape[0], Y.shape[0]))
    for k in range(X.shape[1]):             # one feature at a time: no [m, m, d] temporary
        diff = X[:, k, None] - Y[None, :, k]
        D += diff * diff
    return D


def mmd2_ref(X, Y, sigmas):
    """Biased mixture-RBF MMD^2 in float64 from float64 distances (float64 1 / (2 sigma^2)), and the three kernel sums."""
    sums = []
    for A, Bm in ((X, X), (Y, Y), (X, Y)):
        D = sqdist_f64(A, Bm)
        sums.append(sum(float(np.exp(-D / (2.0 * s * s)).sum()) for s in sigmas))
    m = len(X)
    return (sums[0] + sums[1] - 2.0 * sums[2]) / (m * m), sums


def mmd2_abs_bound(sums, m, d, n_sigma):
    """[1e-6 (S_XX + S_YY + 2 S_XY) + 0.37 n_sigma tol_D 4 m^2] / m^2.  First term: the RBF_RTOL of each kernel sum.
    Second: a relative error tol_D of a distance D moves exp(-gamma D) by at most gamma D exp(-gamma D) tol_D <=
    tol_D / e < 0.37 tol_D, for each of n_sigma kernels and 4 m^2 entries (XX, YY and XY twice).
    tol_D = 4e-7 max(4, sqrt(d)) is the bound of the cost kernel's own tests (tests/test_gpu_kernels.py)."""
    tol_d = 4e-7 * max(4.0, np.sqrt(d))
    return (RBF_RTOL * (sums[0] + sums[1] + 2.0 * sums[2]) + 0.37 * n_sigma * tol_d * 4.0 * m * m) / (m * m)


@functools.lru_cache(maxsize=None)
def mmd_clouds(m, d):
    rng = np.random.default_rng(17 * m + d)
    X = rng.standard_normal((m, d)).astype(np.float32)
    Y = (0.8 * rng.standard_normal((m, d)) + 0.3).astype(np.float32)
    X.setflags(write=False); Y.setflags(write=False)
    return X, Y


# --------------------------------------------------------------------------- cost tails
COST_TAIL_SHAPE = (1025, 1025, 2)          # 1 050 625 entries: above the 2048-block (max) and 4096-block (scale, sqrt) caps


@functools.lru_cache(maxsize=None)
def cost_tail_clouds(max_at):
    """Clouds of COST_TAIL_SHAPE whose largest squared distance is the pair (0, 0) (max_at="first") or the pair
    (B0 - 1, B1 - 1) (max_at="last") by a wide margin."""
    B0, B1, d = COST_TAIL_SHAPE
    rng = np.random.default_rng(5)
    x0 = rng.standard_normal((B0, d)).astype(np.float32)
    x1 = rng.standard_normal((B1, d)).astype(np.float32)
    r = 0 if max_at == "first" else B0 - 1
    c = 0 if max_at == "first" else B1 - 1
    x0[r] = (-40.0, -40.0)
    x1[c] = (40.0, 40.0)
    x0.setflags(write=False); x1.setflags(write=False)
    return x0, x1
