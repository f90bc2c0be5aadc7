"""Noise schedules g(t) of the reference process dX = g(t) dW behind [SF]2M — the three schedules the reference's
runner is written around (``runner/src/models/components/schedule.py``: constant, linearly decreasing variance,
cosine), restated from their formulas.

A schedule is called with the time and returns the diffusion g(t); ``F(t)`` is the accumulated variance
``int_0^t g(s)^2 ds`` in closed form and ``sigma_t(t) = sqrt(F(t) - F(t)^2 / F(1))`` the standard deviation at time t of
the bridge of that process pinned at both ends.  ``t`` is a Python number, a 0-dim tensor or a ``[B]`` tensor; a
number gives a number, a tensor gives a tensor of its shape, dtype and device.
"""
import math

import torch


def _is_t(t):
    return isinstance(t, torch.Tensor)


class NoiseScheduler:
    """Base class: ``__call__(t)`` = g(t) and ``F(t)`` = int_0^t g^2 are the subclass's; ``sigma_t`` follows."""

    def __call__(self, t):
        raise NotImplementedError

    def F(self, t):
        raise NotImplementedError

    def sigma_t(self, t):
        """sqrt(F(t) - F(t)^2 / F(1)): zero at both ends (a rounding residue below zero is clamped, not a NaN)."""
        Ft = self.F(t)
        var = Ft - Ft ** 2 / self.F(1.0)
        if _is_t(var):
            return torch.sqrt(torch.clamp(var, min=0.0))
        return math.sqrt(max(var, 0.0))


class ConstantNoiseScheduler(NoiseScheduler):
    """g = sigma, F = sigma^2 t."""

    def __init__(self, sigma):
        self.sigma = sigma

    def __call__(self, t):
        return self.sigma * torch.ones_like(t) if _is_t(t) else self.sigma

    def F(self, t):
        return self.sigma ** 2 * t


class LinearDecreasingNoiseScheduler(NoiseScheduler):
    """g^2 = t sigma_min + (1 - t) sigma_max: both parameters are VARIANCES, as in the reference.
    F = sigma_max t + t^2 (sigma_min - sigma_max) / 2."""

    def __init__(self, sigma_min, sigma_max):
        self.sigma_min, self.sigma_max = sigma_min, sigma_max

    def __call__(self, t):
        g2 = t * self.sigma_min + (1 - t) * self.sigma_max
        return torch.sqrt(g2) if _is_t(g2) else math.sqrt(g2)

    def F(self, t):
        return self.sigma_max * t + t ** 2 * ((self.sigma_min - self.sigma_max) / 2)


class CosineNoiseScheduler(NoiseScheduler):
    """g = scale (1 - cos 2 pi t) + sigma_min.  With w = 2 pi, s = scale, m = sigma_min:
    F = s^2 (3 t / 2 - 2 sin(w t) / w + sin(2 w t) / (4 w)) + 2 s m (t - sin(w t) / w) + m^2 t."""

    def __init__(self, sigma_min, scale):
        self.sigma_min, self.scale = sigma_min, scale

    def __call__(self, t):
        c = torch.cos(2 * math.pi * t) if _is_t(t) else math.cos(2 * math.pi * t)
        return self.scale * (1 - c) + self.sigma_min

    def F(self, t):
        w = 2 * math.pi
        if _is_t(t):
            s1, s2 = torch.sin(w * t), torch.sin(2 * w * t)
        else:
            s1, s2 = math.sin(w * t), math.sin(2 * w * t)
        s, m = self.scale, self.sigma_min
        return s ** 2 * (1.5 * t - 2 * s1 / w + s2 / (4 * w)) + 2 * s * m * (t - s1 / w) + m ** 2 * t
