"""CPU: properties of the candidate-list rule as tests/asg_build_restate.py states it (the restatement is what
tests/test_gpu_asg_build.py compares the kernel with, bit for bit).  Random and adversarial rows:

  * the member count is in [32, 64], or the rule took its documented exit (the bisection ran out of fp32 thresholds or
    of its 48 steps with fewer than 32 members below `lo`);
  * every column that is not listed satisfies c + p >= cT — the bound the solver's a-posteriori test relies on;
  * duplicated costs and all-equal rows terminate;
  * the written order is slot-major, then lane, with each path's lane-to-column map.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asg_build_restate as R


def _instances():
    rng = np.random.default_rng(7)
    out = {}
    for n in (128, 200, 1024):          # slow path (full / ragged strips) and the smallest fast-path size
        out[f"uniform_{n}"] = (rng.random((n, n), dtype=np.float32), rng.random(n) * 0.5)
    n = 1024
    x0, x1 = rng.standard_normal((n, 8)), rng.standard_normal((n, 8))
    out["sqeuclid_1024"] = (((x0[:, None, :] - x1[None, :, :]) ** 2).sum(-1).astype(np.float32), rng.random(n) * 3.0)
    out["ties_int_1024"] = (rng.integers(0, 4, (n, n)).astype(np.float32), np.zeros(n))
    out["ties_int_200"] = (rng.integers(0, 3, (200, 200)).astype(np.float32), rng.integers(0, 2, 200).astype(np.float64))
    out["all_equal_1024"] = (np.full((n, n), 2.5, dtype=np.float32), np.zeros(n))
    out["all_equal_130"] = (np.full((130, 130), 1.0, dtype=np.float32), np.full(130, 0.25))
    m = rng.random((n, n), dtype=np.float32)
    m[:, ::2] = m[:, 1::2]               # every cost twice
    out["duplicated_1024"] = (m, np.zeros(n))
    m = rng.random((n, n), dtype=np.float32) + 1.0
    m[:, :100] = 0.0                     # one hundred exact zeros per row: hi = 0, t1 = the smallest denormal
    out["zeros_1024"] = (m, np.zeros(n))
    out["huge_range_128"] = ((10.0 ** rng.uniform(-30, 30, (128, 128))).astype(np.float32), np.zeros(128))
    out["all_listed_64"] = (rng.random((64, 64), dtype=np.float32), rng.random(64))
    out["all_listed_40"] = (rng.random((40, 40), dtype=np.float32), rng.random(40))
    return out


INST = _instances()


@pytest.fixture(scope="module")
def built():
    return {k: R.build_lists(M, p) for k, (M, p) in INST.items()}


@pytest.mark.parametrize("name", sorted(INST))
def test_count_bound_and_order(built, name):
    M, p = INST[name]
    cl, cT, tau, cnt = built[name]
    n = M.shape[0]
    lane, slot = R.lane_slot(n)
    key = slot * 64 + lane
    for i in range(n):
        s = M[i].astype(np.float64) + p
        m = s.min()
        r = (s - m).astype(np.float32)
        c = int(cnt[i])
        cols = cl[i, :c, 0].astype(np.int64)
        assert np.all(cl[i, c:, 0] == R.NOCOL) and np.all(cl[i, c:, 1] == R.INF_BITS)
        assert len(set(cols.tolist())) == c and np.all(cols < n)
        assert np.array_equal(cl[i, :c, 1], M[i, cols].view(np.uint32))
        assert np.all(np.diff(key[cols]) > 0), "slot-major, then lane"
        if n <= R.SP_K:
            assert c == n and cT[i] == np.inf
            continue
        listed = np.zeros(n, dtype=bool)
        listed[cols] = True
        assert np.array_equal(listed, r < tau[i])
        assert np.all(s[~listed] >= cT[i]), "a dropped column lies below the bound"
        assert cT[i] <= m + float(tau[i])
        how = R.row_tau(r, lane)[1]
        if how == "t1":
            assert c == 64 or (n % 64 != 0 and 32 <= c <= 64)
        elif how == "window":
            assert 32 <= c <= 64
        else:
            assert how in ("collapsed", "cap") and c < 32       # the documented exit


def test_tied_rows_take_the_exit_and_terminate(built):
    for name in ("all_equal_1024", "all_equal_130", "ties_int_1024", "zeros_1024"):
        cl, cT, tau, cnt = built[name]
        assert np.all(cnt < 32), name           # more than 64 columns share the smallest r: nothing can be listed
        assert np.all(np.isfinite(cT)), name


def test_generic_rows_are_listed_in_the_window(built):
    for name in ("uniform_128", "uniform_200", "uniform_1024", "sqeuclid_1024"):
        cnt = built[name][3]
        assert np.all((cnt >= 32) & (cnt <= 64)), name


def test_the_two_paths_use_different_lane_maps():
    lane_f, slot_f = R.lane_slot(1024)
    lane_s, slot_s = R.lane_slot(1000)
    assert lane_f[5] == 1 and slot_f[5] == 1 and lane_f[256] == 0 and slot_f[256] == 4
    assert lane_s[5] == 5 and slot_s[5] == 0 and lane_s[64] == 0 and slot_s[64] == 1
    assert not R.is_fast(64) and not R.is_fast(576) and R.is_fast(2048)
