"""GPU: the behaviour of OTPlanSampler's Python layer that its callers rely on and that no kernel test sees — which
draws consume the global ``np.random`` stream and how many, what is printed, warned and raised for a plan that is
not finite or has no mass (ref:88-96, :118), that the batched and the single entry points agree, and that a solver's
``info`` belongs to its coupling.

Shapes: 32 x 32, and 5 x 7 / 12 x 18 (lcm 35 / 36) where rows and columns, or two kinds of coupling, can be mixed up.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UNIFORM = "reverting to uniform plan"
NOT_FINITE = "ERROR: p is not finite"
CHOICE_NAN = "probabilities contain NaN"


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def clouds(dev, B0, B1, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B0, d, generator=g).to(dev), (torch.randn(B1, d, generator=g) * 0.8 + 0.3).to(dev)


def next_after(seed, count):
    """What a fresh stream seeded with `seed` gives after `count` uniforms."""
    rs = np.random.RandomState(seed)
    rs.random_sample(count)
    return rs.random_sample()


KINDS = {
    "exact": ("exact", 32, 32, 2, {}),
    "exact-lcm": ("exact", 12, 18, 2, {}),
    "sinkhorn-points": ("sinkhorn", 32, 32, 2, {"reg": 1.0}),
    "sinkhorn-matrix": ("sinkhorn", 32, 32, 5, {"reg": 1.0}),
    "unbalanced": ("unbalanced", 32, 32, 2, {"reg": 1.0, "reg_m": 2.0}),
    "partial": ("partial", 32, 32, 2, {"reg": 1.0}),
}


@pytest.mark.parametrize("name", list(KINDS))
def test_sample_indices_is_get_map_then_sample_map(dev, name):
    """ref:123-145: sample_plan is get_map + sample_map; here the plan stays on the device (or is never built)."""
    from cfm_amd.optimal_transport import OTPlanSampler
    method, B0, B1, d, kw = KINDS[name]
    x0, x1 = clouds(dev, B0, B1, d, 3)
    s = OTPlanSampler(method=method, **kw)
    np.random.seed(17)
    i, j = s._sample_indices(x0, x1)
    assert np.random.random_sample() == next_after(17, B0)
    np.random.seed(17)
    pi = s.get_map(x0, x1)
    i2, j2 = s.sample_map(pi, B0)
    assert np.random.random_sample() == next_after(17, B0)
    i, j = i.cpu().numpy(), j.cpu().numpy()
    assert i.shape == (B0,) and (pi[i, j] > 0).all()
    assert np.array_equal(i, i2) and np.array_equal(j, j2)


def plan_5x7(dev):
    from cfm_amd.optimal_transport import OTPlanSampler
    x0, x1 = clouds(dev, 5, 7, 2, 4)
    c = OTPlanSampler(method="exact")._solve(x0, x1)
    assert c.kind == "plan" and tuple(c.sol.shape) == (5, 7) and c.info is None
    return x0, x1, c


def test_plan_without_mass_draws_first_then_reverts_to_uniform(dev):
    from cfm_amd.optimal_transport import OTPlanSampler
    x0, x1, c = plan_5x7(dev)
    c = c._replace(sol=torch.zeros_like(c.sol))
    flat = np.minimum(np.floor(np.random.RandomState(23).random_sample(5) * 35), 34).astype(np.int64)
    want = np.divmod(flat, 7)
    for warn in (True, False):
        s = OTPlanSampler(method="exact", warn=warn)
        np.random.seed(23)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            i, j = s._indices_from_solution(x0, x1, c)
        assert np.random.random_sample() == next_after(23, 5)
        assert any(UNIFORM in str(x.message) for x in w) == warn and len(w) == int(warn)
        assert np.array_equal(i.cpu().numpy(), want[0]) and np.array_equal(j.cpu().numpy(), want[1])


def test_plan_with_a_nan_is_reported_and_raises_before_the_draw(dev, capsys):
    from cfm_amd.optimal_transport import OTPlanSampler
    x0, x1, c = plan_5x7(dev)
    plan = c.sol.clone()
    plan[2, 3] = float("nan")
    np.random.seed(29)
    with pytest.raises(ValueError, match=CHOICE_NAN):
        OTPlanSampler(method="exact")._indices_from_solution(x0, x1, c._replace(sol=plan))
    assert np.random.random_sample() == next_after(29, 0)
    out = capsys.readouterr().out
    assert out.startswith(NOT_FINITE + "\ntensor(") and "nan" in out.split("Cost mean, max")[0]
    assert "Cost mean, max tensor(" in out


def test_dense_coupling_with_a_nan_potential_raises_before_the_draw(dev, capsys):
    from cfm_amd.optimal_transport import OTPlanSampler
    x0, x1 = clouds(dev, 32, 32, 5, 3)
    s = OTPlanSampler(method="sinkhorn", reg=1.0)
    c = s._solve(x0, x1)
    assert c.kind == "dense" and c.info is None
    c.sol.f = c.sol.f.clone()
    c.sol.f[7] = float("nan")
    np.random.seed(31)
    with pytest.raises(ValueError, match=CHOICE_NAN):
        s._indices_from_solution(x0, x1, c)
    assert np.random.random_sample() == next_after(31, 0)
    out = capsys.readouterr().out
    # the potential form has no plan to print: the cost line follows the headline directly
    assert out.startswith(NOT_FINITE + "\nCost mean, max tensor(")


def test_get_map_warnings(dev):
    from cfm_amd.optimal_transport import OTPlanSampler
    g = torch.Generator().manual_seed(0)        # the inputs of test_unbalanced_underflow_reverts_and_falls_back
    x0 = torch.randn(32, 2, generator=g) * 40
    x1 = torch.randn(32, 2, generator=g) * 40 + 300
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pi = OTPlanSampler(method="unbalanced", reg=0.05).get_map(x0, x1)
    assert sorted(str(x.message) for x in w) == ["Numerical errors at iteration 0",
                                                 "Numerical errors in OT plan, reverting to uniform plan."]
    assert np.array_equal(pi, np.full((32, 32), 1.0 / 1024))
    # a rectangular exact plan carries no solver info: nothing to warn about
    x0, x1 = clouds(dev, 12, 18, 2, 3)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pi = OTPlanSampler(method="exact").get_map(x0, x1)
    assert not w and pi.shape == (12, 18) and pi.dtype == np.float64
    # multiples of 1 / 36: the sums are exact up to the rounding of 1 / 36 itself
    assert np.abs(pi.sum(1) - 1 / 12).max() < 1e-15 and np.abs(pi.sum(0) - 1 / 18).max() < 1e-15
    assert abs(pi.sum() - 1.0) < 1e-14


def matcher(name):
    import cfm_amd
    if name == "exact":
        return cfm_amd.ExactOptimalTransportConditionalFlowMatcher(sigma=0.1)
    return cfm_amd.SchrodingerBridgeConditionalFlowMatcher(sigma=1.0, ot_method="sinkhorn")


@pytest.mark.parametrize("name", ["exact", "sinkhorn"])
def test_group_call_is_the_single_calls(dev, name):
    fm = matcher(name)
    batches = [clouds(dev, 32, 32, 2, 40 + k) for k in range(3)]

    def seed():
        np.random.seed(5); torch.manual_seed(5)     # torch.manual_seed seeds the CPU and the device generators

    seed()
    group = fm.sample_location_and_conditional_flow_group(batches, return_noise=True)
    after = (np.random.random_sample(), torch.rand(1).item(), torch.rand(1, device=dev).item())
    seed()
    single = [fm.sample_location_and_conditional_flow(x0, x1, return_noise=True) for x0, x1 in batches]
    assert after == (np.random.random_sample(), torch.rand(1).item(), torch.rand(1, device=dev).item())
    assert len(group) == 3
    for a, b in zip(group, single):
        assert len(a) == len(b) == 4 and all(torch.equal(p, q) for p, q in zip(a, b))


def shifted_pairs(dev):
    """Four 33 x 31 pairs whose solves end with four different infos: the farther the target, the more iterations and
    the more entries of K = exp(-M / reg) that underflow to zero (float64 restatement of the loop: 21 iterations and no
    zero, then 31 iterations with 0, 4 and 68 zeros; every status 0)."""
    pairs = [clouds(dev, 33, 31, 2, 50 + k) for k in range(4)]
    return [(a, b + shift) for (a, b), shift in zip(pairs, (0.0, 16.0, 17.0, 18.0))]


def test_solve_many_keeps_each_info_with_its_coupling(dev):
    """Worker threads solve the four pairs on three streams; every coupling comes back with ITS solver's info."""
    from cfm_amd.optimal_transport import OTPlanSampler
    pairs = shifted_pairs(dev)
    s = OTPlanSampler(method="unbalanced", reg=1.0, reg_m=2.0)
    serial = [s._solve(a, b) for a, b in pairs]
    again = [s._solve(a, b) for a, b in pairs]
    many = s._solve_many(pairs, workers=3)
    infos = [c.info.tolist() for c in serial]
    assert len({tuple(r) for r in infos}) == 4, infos
    assert [c.info.tolist() for c in many] == infos
    for c, a, b in zip(many, serial, again):
        assert c.kind == "plan" and c.sol.shape == (33, 31)
        spread = (a.sol - b.sol).abs().max().item()           # run to run: the solvers' sums use atomics
        assert (c.sol - a.sol).abs().max().item() <= spread
