"""sdeint(..., logqp=True) on the eager path and the host side of the HIP paths (CPU, no library call).

torchsde is not installable next to this suite: the log-ratio column (torchsde's SDELogqp for diagonal noise: drift
0.5 * (u ** 2).sum(1), u = stable_division(f - h, g), zero diffusion, zero start, returned per interval of ts) is pinned to
closed forms here: a constant drift c and a constant or scheduled g make the integrand a known function of time."""
import math
import struct

import pytest
import torch

from cfm_amd import sde as S
from cfm_amd.schedule import LinearDecreasingNoiseScheduler
from cfm_amd.sde import DriftSDE, DSBMFlowSolver, FlowScoreSDE, FlowSolver, sdeint

TS = torch.tensor([0.0, 0.25, 1.0], dtype=torch.float64)
DT = 0.125                      # 2 + 6 dyadic steps, two intervals of different length
C = torch.tensor([0.5, -1.5, 0.25], dtype=torch.float64)
HALF_C2 = 0.5 * float((C * C).sum())


def _const(x):
    return C.to(x.dtype).expand(x.shape[0], -1)


def _zero(x):
    return torch.zeros_like(x[:, :-1])


def _wiggle(x):
    y, t = x[:, :-1], x[:, -1:]
    return torch.sin(2.0 * y) - 0.7 * y + torch.cos(3.0 * t)


def _y0(B=5, seed=0):
    return torch.randn((B, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _noise(method, n, B, seed=1):
    shape = (n, 2, B, 3) if method == "srk" else (n, B, 3)
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_logqp_returns_the_pair_with_torchsde_shapes():
    y0 = _y0()
    out = sdeint(FlowScoreSDE(_wiggle, _zero, sigma=0.5), y0, TS, dt=DT, noise="torch", logqp=True)
    assert isinstance(out, tuple) and len(out) == 2
    ys, lr = out
    assert ys.shape == (3, 5, 3) and lr.shape == (2, 5) and ys.dtype == lr.dtype == torch.float64
    assert torch.is_tensor(sdeint(FlowScoreSDE(_wiggle, _zero, sigma=0.5), y0, TS, dt=DT, noise="torch"))


class _Field(torch.nn.Module):
    """f(t, x) as the solver classes call their nets"""

    def forward(self, t, x):
        return 0.3 * x + 0.1


def test_solver_classes_return_the_pair():
    x0 = torch.randn((4, 2), generator=torch.Generator().manual_seed(0))
    t_span = torch.linspace(0, 1, 3)
    fs = FlowSolver(_Field(), 2, score_field=_Field(), sigma=lambda t: 0.5, dt=0.25)
    traj, kl = fs.sdeint(x0, t_span + 1, logqp=True)
    assert traj.shape == (3, 4, 2) and kl.shape == (2, 4) and fs.last_path == "eager" and fs.nfe == 4
    ds = DSBMFlowSolver(_Field(), 2, score_field=_Field(), sigma=0.5, dt=0.25)
    traj, kl = ds.sdeint(x0, t_span, reverse=True, logqp=True)
    assert traj.shape == (3, 4, 2) and kl.shape == (2, 4) and ds.last_path == "eager" and ds.nfe == 4
    # forward: f = 0.6 y + 0.2 -> the first step's integrand, by hand
    traj, kl = fs.sdeint(x0, torch.tensor([0.0, 0.25]), logqp=True)
    want = 0.25 * 0.5 * (((0.6 * x0 + 0.2) / 0.5) ** 2).sum(1)
    assert torch.allclose(kl[0], want, rtol=1e-6, atol=0)
    # the positional order of the existing arguments is what it was
    g = torch.Generator().manual_seed(3)
    a = fs.sdeint(x0, t_span, True, g)
    b = fs.sdeint(x0, t_span, reverse=True, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, b)


def test_adaptive_is_refused_with_a_reason():
    x0 = torch.zeros((2, 2))
    for solver in (FlowSolver(_Field(), 2, score_field=_Field(), sigma=lambda t: 0.5),
                   DSBMFlowSolver(_Field(), 2, score_field=_Field(), sigma=0.5)):
        with pytest.raises(NotImplementedError, match="fixed steps"):
            solver.sdeint(x0, torch.linspace(0, 1, 2), logqp=True, adaptive=True)
        with pytest.raises(TypeError):
            solver.sdeint(x0, torch.linspace(0, 1, 2), False, None, "philox", None, True)       # the new ones are keyword-only


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("method", ["euler", "srk"])
def test_constant_drift_constant_sigma_is_the_closed_form(method, reverse):
    """f = +-c whatever the state and the noise: every interval gives (t_{i+1} - t_i) 1/2 |c|^2 / sigma^2"""
    sigma = 0.7
    n = len(S._grid(TS, DT))
    ys, lr = sdeint(FlowScoreSDE(_const, _zero, sigma=sigma, reverse=reverse), _y0(), TS, method=method, dt=DT,
                    noise=_noise(method, n, 5), logqp=True)
    want = torch.tensor([0.25, 0.75], dtype=torch.float64)[:, None] * HALF_C2 / sigma ** 2
    assert torch.allclose(lr, want.expand(2, 5), rtol=1e-13, atol=0), (lr, want)


def test_constant_drift_under_a_schedule_sums_the_steps():
    sched = LinearDecreasingNoiseScheduler(0.1, 1.0)
    grid = S._grid(TS, DT)
    ys, lr = sdeint(DriftSDE(_const, sigma=sched), _y0(), TS, dt=DT, noise=_noise("euler", len(grid), 5), logqp=True)
    want, acc = [], 0.0
    for t, h, is_out in grid:
        acc += h * HALF_C2 / float(sched(torch.tensor(t, dtype=torch.float64))) ** 2
        if is_out:
            want.append(acc)
            acc = 0.0
    assert torch.allclose(lr, torch.tensor(want, dtype=torch.float64)[:, None].expand(2, 5), rtol=1e-12, atol=0)


class _WithPrior:
    """constant f, g and a NON-zero prior drift h"""
    noise_type, sde_type = "diagonal", "ito"

    def __init__(self, g=0.5, prior=True):
        self.gval = g
        if prior:
            self.h = lambda t, y: torch.full_like(y, 0.25)

    def f(self, t, y):
        return torch.full_like(y, 1.0)

    def g(self, t, y):
        return torch.full_like(y, self.gval)


def test_a_prior_drift_enters_as_f_minus_h():
    y0 = _y0(B=2)
    _, with_h = sdeint(_WithPrior(), y0, TS, dt=DT, noise="torch", logqp=True)
    _, without = sdeint(_WithPrior(prior=False), y0, TS, dt=DT, noise="torch", logqp=True)
    w = torch.tensor([0.25, 0.75], dtype=torch.float64)[:, None].expand(2, 2)
    assert torch.allclose(with_h, w * 0.5 * 3 * (0.75 / 0.5) ** 2, rtol=1e-13, atol=0)
    assert torch.allclose(without, w * 0.5 * 3 * (1.0 / 0.5) ** 2, rtol=1e-13, atol=0)


@pytest.mark.parametrize("g, used", [(1e-8, 1e-7), (-1e-9, -1e-7), (1e-7, 1e-7), (2e-7, 2e-7)])
def test_tiny_g_follows_stable_division(g, used):
    _, lr = sdeint(_WithPrior(g=g, prior=False), _y0(B=2), torch.tensor([0.0, 0.5], dtype=torch.float64), dt=0.5,
                   noise="torch", logqp=True)
    assert torch.allclose(lr, torch.full((1, 2), 0.5 * 0.5 * 3 / used ** 2, dtype=torch.float64), rtol=1e-12, atol=0)
    # and the HIP paths' per-step weight takes the same g (float32 of the float64 quotient)
    qw = S._logqp_weights([(0.0, 0.5, True)], [g], False)
    assert qw == [struct.unpack("<f", struct.pack("<f", 0.25 / used ** 2))[0]]


def test_stable_division_is_torchsde_s():
    b = torch.tensor([0.0, 1e-7, -1e-7, 5e-8, -5e-8, 2e-7, -3.0], dtype=torch.float64)
    got = S._stable_division(torch.ones_like(b), b)
    assert torch.isinf(got[0])
    assert torch.allclose(got[1:], 1.0 / torch.tensor([1e-7, -1e-7, 1e-7, -1e-7, 2e-7, -3.0], dtype=torch.float64), rtol=1e-15)


def test_zero_g_is_refused_by_the_hip_weights():
    with pytest.raises(ValueError, match="g = 0"):
        S._logqp_weights([(0.0, 0.5, False), (0.5, 0.5, True)], [0.3, 0.0], False)


@pytest.mark.parametrize("method", ["euler", "srk"])
def test_the_trajectory_keeps_its_bits(method):
    n = len(S._grid(TS, DT))
    xi = _noise(method, n, 5)
    sde = FlowScoreSDE(_wiggle, _zero, sigma=0.4, reverse=True)
    plain = sdeint(sde, _y0(), TS, method=method, dt=DT, noise=xi)
    ys, lr = sdeint(sde, _y0(), TS, method=method, dt=DT, noise=xi, logqp=True)
    assert torch.equal(plain, ys)
    assert bool((lr > 0).all())


def test_increments_are_per_interval_not_cumulative():
    xi = _noise("euler", 8, 5)
    sde = FlowScoreSDE(_wiggle, _zero, sigma=0.4)
    _, two = sdeint(sde, _y0(), TS, dt=DT, noise=xi, logqp=True)
    _, one = sdeint(sde, _y0(), torch.tensor([0.0, 1.0], dtype=torch.float64), dt=DT, noise=xi, logqp=True)
    assert torch.allclose(two.sum(0), one[0], rtol=1e-13, atol=0)


def test_packed_blob_against_a_case_computed_by_hand():
    """ts = (0, 0.25, 1), dt = 1/4: four steps of 1/4, outputs after the first and the last.  Records first, bytes as
    _em_records / _srk_records give them, then qw; the workspace holds (record + 4) n_steps bytes."""
    steps = S._grid([0.0, 0.25, 1.0], 0.25)
    assert steps == [(0.0, 0.25, True), (0.25, 0.25, False), (0.5, 0.25, False), (0.75, 0.25, True)]
    g = [0.5, 0.25, 1.0, 2.0]
    qw = S._logqp_weights(steps, g, False)
    assert qw == [0.5, 2.0, 0.125, 0.03125]                     # h / (2 g^2), all dyadic
    blob, ws_bytes = S._packed_steps(steps, g, False, True, qw)
    assert ws_bytes == len(blob) == (16 + 4) * 4
    assert blob[:64] == S._em_records(steps, g, True)
    assert blob[:16] == struct.pack("<fffi", 1.0, 0.25, 0.25, 1)          # te = 1 - t, h, g sqrt|h| = 0.5 * 0.5, is_out
    assert blob[64:] == struct.pack("<4f", 0.5, 2.0, 0.125, 0.03125)
    plain, plain_bytes = S._packed_steps(steps, g, False, True)
    assert plain == blob[:64] and plain_bytes == 64
    # srk, sigma = 0.5: h / (12 sigma^2) = 1/12 per step, rounded to float32 once
    qs = S._logqp_weights(steps, [0.5] * 4, True)
    w = struct.unpack("<f", struct.pack("<f", 0.25 / (12.0 * 0.25)))[0]
    assert qs == [w] * 4
    blob, ws_bytes = S._packed_steps(steps, [0.5] * 4, True, False, qs)
    assert ws_bytes == len(blob) == (32 + 4) * 4
    assert blob[:128] == S._srk_records(steps, 0.5, False) and blob[128:] == struct.pack("<4f", *qs)
    assert blob[:32] == struct.pack("<ffffffii", 0.0, 0.25, 0.125, 0.25, 0.25, 0.1875, 1, 0)


def test_the_sde_classes_have_a_zero_prior():
    y = torch.ones((2, 3))
    fs = FlowSolver(_Field(), 3, score_field=_Field(), sigma=lambda t: 0.5)
    for obj in (FlowScoreSDE(_const, _zero), DriftSDE(_const), S._SolverSDE(fs, False)):
        assert torch.equal(obj.h(0.0, y), torch.zeros_like(y))
