"""sdeint(method="srk") on the eager path (CPU, float64, no library call): the scheme itself.

torchsde is not installable next to this suite, so `srk` (Roessler's SRI2W1 for constant diagonal noise) is pinned to
restatements: its strong order on an exactly aggregated Brownian path, its sigma = 0 limit (Shu-Osher SSPRK3), and a
step-by-step NumPy restatement on a refined grid."""
import math

import numpy as np
import pytest
import torch

from cfm_amd.sde import FlowScoreSDE, FlowSolver, sdeint

SQ3 = math.sqrt(3.0)


def _drift(x):                      # x = [y, t]
    y, t = x[:, :-1], x[:, -1:]
    return -1.5 * y + torch.sin(2.0 * y) + 0.5 * torch.cos(3.0 * t)


def _zero(x):
    return torch.zeros_like(x[:, :-1])


def _score(x):
    y, t = x[:, :-1], x[:, -1:]
    return -0.3 * y * (1.0 + t)


def _f_np(t, y):
    return -1.5 * y + np.sin(2.0 * y) + 0.5 * np.cos(3.0 * t) - 0.3 * y * (1.0 + t)


def _srk_np(f, y, grid, sigma, xi):
    """the scheme of the issue, step by step: grid = [(t, h)], xi [n_steps, 2, B, d]"""
    out = []
    for k, (t, h) in enumerate(grid):
        x1, x2 = xi[k, 0], xi[k, 1]
        k1 = f(t, y)
        k2 = f(t + h, y + h * k1)
        k3 = f(t + h / 2, y + (h / 4) * (k1 + k2) + 0.75 * sigma * math.sqrt(h) * (x1 + x2 / SQ3))
        y = y + h * (k1 / 6 + k2 / 6 + (2.0 / 3.0) * k3) + sigma * math.sqrt(h) * x1
        out.append(y)
    return out


def _coarsen(I1, I10, h):
    """two steps of length h -> one of length 2h, exactly: I1 = I1a + I1b, I10 = I10a + I10b + h I1a"""
    a1, b1, a10, b10 = I1[0::2], I1[1::2], I10[0::2], I10[1::2]
    return a1 + b1, a10 + b10 + h * a1


def _to_xi(I1, I10, h):
    x1 = I1 / math.sqrt(h)
    x2 = SQ3 * (2.0 * I10 / h ** 1.5 - x1)
    return torch.stack([x1, x2], 1)          # [n, 2, B, d]


def test_strong_order_on_one_brownian_path():
    """RMS endpoint error against srk on the 1024-step grid, same path: fitted order of srk >= 1.3 between h = 1/16
    and 1/64 (Euler-Maruyama: 1.0, theory: 1.5), and srk's error at 1/64 at most a tenth of Euler's."""
    g = torch.Generator().manual_seed(0)
    n, B, sigma = 1024, 4000, 0.7
    xi = torch.randn((n, 2, B, 1), dtype=torch.float64, generator=g)
    h = 1.0 / n
    I1 = math.sqrt(h) * xi[:, 0]
    I10 = (h ** 1.5 / 2.0) * (xi[:, 0] + xi[:, 1] / SQ3)
    sde = FlowScoreSDE(_drift, _zero, sigma=sigma)
    y0 = torch.full((B, 1), 0.3, dtype=torch.float64)
    ts = torch.tensor([0.0, 1.0], dtype=torch.float64)
    ref = sdeint(sde, y0, ts, method="srk", dt=h, noise=xi)[-1]
    err = {}
    while n > 16:
        I1, I10 = _coarsen(I1, I10, h)
        n, h = n // 2, 2.0 * h
        if n in (64, 32, 16):
            x = _to_xi(I1, I10, h)
            a = sdeint(sde, y0, ts, method="srk", dt=h, noise=x)[-1]
            b = sdeint(sde, y0, ts, method="euler", dt=h, noise=x[:, 0])[-1]
            err[n] = (float(((a - ref) ** 2).mean().sqrt()), float(((b - ref) ** 2).mean().sqrt()))
    print("rms endpoint error (srk, euler) by steps:", err)
    order_srk = math.log(err[16][0] / err[64][0]) / math.log(4.0)
    order_em = math.log(err[16][1] / err[64][1]) / math.log(4.0)
    print("fitted orders:", order_srk, order_em)
    assert order_srk >= 1.3, (order_srk, err)
    assert err[64][0] <= 0.1 * err[64][1], err
    assert 0.8 <= order_em <= 1.2, order_em          # the path aggregation is right: Euler shows its own order


def test_without_noise_it_is_ssprk3():
    y0 = torch.linspace(-2.0, 2.0, 14, dtype=torch.float64).reshape(7, 2)
    ts = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    tr = sdeint(FlowScoreSDE(_drift, _score, sigma=0.0), y0, ts, method="srk", dt=0.05, noise="torch").numpy()
    y, out, h = y0.numpy(), [y0.numpy()], 0.05
    for k in range(20):
        t = k * h
        y1 = y + h * _f_np(t, y)
        y2 = 0.75 * y + 0.25 * (y1 + h * _f_np(t + h, y1))
        y = y / 3.0 + (2.0 / 3.0) * (y2 + h * _f_np(t + h / 2, y2))
        if k % 5 == 4:
            out.append(y)
    ref = np.stack(out)
    assert tr.shape == ref.shape
    assert np.abs(tr - ref).max() <= 1e-12 * np.abs(ref).max()


def test_reverse_is_the_forward_solve_of_the_written_out_backward_drift():
    g = torch.Generator().manual_seed(1)
    y0 = torch.randn((9, 3), dtype=torch.float64, generator=g)
    ts = torch.linspace(0.0, 1.0, 4, dtype=torch.float64)
    xi = torch.randn((12, 2, 9, 3), dtype=torch.float64, generator=g)
    a = sdeint(FlowScoreSDE(_drift, _score, sigma=0.5, reverse=True), y0, ts, method="srk", dt=0.1, noise=xi)

    def flip(x):
        return torch.cat([x[:, :-1], 1.0 - x[:, -1:]], 1)
    b = sdeint(FlowScoreSDE(lambda x: -_drift(flip(x)), lambda x: _score(flip(x)), sigma=0.5), y0, ts, method="srk", dt=0.1,
               noise=xi)
    assert a.shape == (4, 9, 3)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    assert float((a[-1] - sdeint(FlowScoreSDE(_drift, _score, sigma=0.5), y0, ts, method="srk", dt=0.1, noise=xi)[-1]).abs().max()) > 1e-3


def test_refined_grid_against_the_restatement():
    g = torch.Generator().manual_seed(2)
    ts = [0.0, 0.13, 0.5, 1.0]
    grid = [(0.13 * k / 2, 0.13 / 2) for k in range(2)] + [(0.13 + 0.37 * k / 4, 0.37 / 4) for k in range(4)] + \
           [(0.5 + 0.5 * k / 5, 0.5 / 5) for k in range(5)]
    y0 = torch.randn((6, 2), dtype=torch.float64, generator=g)
    xi = torch.randn((11, 2, 6, 2), dtype=torch.float64, generator=g)
    tr = sdeint(FlowScoreSDE(_drift, _score, sigma=0.8), y0, torch.tensor(ts, dtype=torch.float64), method="srk", dt=0.1, noise=xi)
    states = _srk_np(_f_np, y0.numpy(), grid, 0.8, xi.numpy())
    ref = np.stack([y0.numpy(), states[1], states[5], states[10]])
    assert tr.shape == (4, 6, 2)
    assert np.abs(tr.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    # float32 callers stay in float32
    assert sdeint(FlowScoreSDE(_drift, _score, sigma=0.8), y0.float(), torch.tensor(ts), method="srk", dt=0.1).dtype == torch.float32


def test_noise_tensor_of_the_wrong_shape_and_decreasing_ts_raise_value_error():
    y0 = torch.zeros((5, 2), dtype=torch.float64)
    sde = FlowScoreSDE(_drift, _score, sigma=0.5)
    ts = torch.tensor([0.0, 0.5, 1.0])
    with pytest.raises(ValueError, match=r"\[10, 2, 5, 2\]"):
        sdeint(sde, y0, ts, method="srk", dt=0.1, noise=torch.zeros((10, 5, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[10, 2, 5, 2\]"):
        sdeint(sde, y0, ts, method="srk", dt=0.1, noise=torch.zeros((9, 2, 5, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[10, 5, 2\]"):
        sdeint(sde, y0, ts, method="euler", dt=0.1, noise=torch.zeros((10, 2, 5, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        sdeint(sde, y0, ts, method="srk", dt=0.1, noise="sobol")
    with pytest.raises(ValueError, match="increasing"):
        sdeint(sde, y0, torch.tensor([1.0, 0.5, 0.0]), method="srk", dt=0.1)
    with pytest.raises(ValueError, match="increasing"):
        sdeint(sde, y0, torch.tensor([0.0, 0.5, 0.5]), method="srk", dt=0.1)


def test_what_is_out_of_scope_raises_not_implemented_with_the_reason():
    y0 = torch.zeros((5, 2), dtype=torch.float64)
    ts = torch.tensor([0.0, 1.0])
    with pytest.raises(NotImplementedError, match="constant"):
        sdeint(FlowScoreSDE(_drift, _score, sigma=lambda t: 0.5), y0, ts, method="srk", dt=0.1)

    class Other:
        noise_type, sde_type = "diagonal", "ito"

        def f(self, t, y):
            return -y

        def g(self, t, y):
            return torch.ones_like(y)
    with pytest.raises(NotImplementedError, match="FlowScoreSDE"):
        sdeint(Other(), y0, ts, method="srk", dt=0.1)
    solver = FlowSolver(lambda t, x: -x, dim=2, score_field=lambda t, x: -x, sigma=lambda t: 0.5, sde_solver="srk", dt=0.1)
    with pytest.raises(NotImplementedError, match="constant"):
        solver.sdeint(y0, ts)
    with pytest.raises(NotImplementedError):
        sdeint(FlowScoreSDE(_drift, _score, sigma=0.5), y0, ts, method="milstein", dt=0.1)


def test_euler_with_a_noise_tensor_equals_the_seeded_torch_draws():
    y0 = torch.linspace(-1.0, 1.0, 8, dtype=torch.float64).reshape(4, 2)
    ts = torch.tensor([0.0, 0.13, 0.5, 1.0], dtype=torch.float64)
    sde = FlowScoreSDE(_drift, _score, sigma=0.6)
    a = sdeint(sde, y0, ts, dt=0.1, generator=torch.Generator().manual_seed(5), noise="torch")
    g = torch.Generator().manual_seed(5)
    xi = torch.stack([torch.randn((4, 2), dtype=torch.float64, generator=g) for _ in range(11)])
    b = sdeint(sde, y0, ts, dt=0.1, noise=xi)
    assert torch.equal(a, b)
    # and the same for srk: (2, B, d) per step
    a = sdeint(sde, y0, ts, method="srk", dt=0.1, generator=torch.Generator().manual_seed(5), noise="torch")
    g = torch.Generator().manual_seed(5)
    xi = torch.stack([torch.randn((2, 4, 2), dtype=torch.float64, generator=g) for _ in range(11)])
    assert torch.equal(a, sdeint(sde, y0, ts, method="srk", dt=0.1, noise=xi))
