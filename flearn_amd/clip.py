"""Norm clipping on the host: the radius and the per-client scales of a clipped round, from the
clients' squared update norms (Sun et al. 2019; McMahan et al. 2018; the quantile radius of Andrew et
al. 2021).  numpy only: no torch, no GPU.  The device makes the norms (ops.rownorm2_stack) and applies
the scales (ops.clip_sum_stack); everything between is float64 arithmetic here, restated by
tests/clip_ref.py.

    tau   : the given radius (a float > 0, inf allowed), or with quantile = q in (0, 1] the
            ceil(q * F)-th smallest of the F finite norms sqrt(d2_i) — an actual client's norm, so
            there is no interpolation and no tie rule;
    s_i   : 0 for a non-finite d2_i (the upload is replaced by the centre), 1 for sqrt(d2_i) <= tau,
            else fl32(tau / sqrt(d2_i)), and a ratio that rounds to >= 1 is 1.
    sigma : fl32(noise_multiplier * tau), the Gaussian noise a DP-FedAvg round adds to the clipped
            sum (check_noise: what such a round refuses).
"""
from __future__ import annotations

import math

import numpy as np


def _is_real(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def check_radius(tau, quantile):
    """(tau, None) or (None, quantile) as Python floats; ValueError unless exactly one is given, tau is
    a number > 0 (inf allowed, NaN not) and quantile a number in (0, 1]."""
    if (tau is None) == (quantile is None):
        raise ValueError("exactly one of tau and quantile must be given")
    if tau is not None:
        if not _is_real(tau) or not float(tau) > 0.0:  # NaN fails the comparison
            raise ValueError(f"tau must be a number > 0 (inf allowed), got {tau!r}")
        return float(tau), None
    if not _is_real(quantile) or not 0.0 < float(quantile) <= 1.0:
        raise ValueError(f"quantile must be a number in (0, 1], got {quantile!r}")
    return None, float(quantile)


def _is_u64(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 0 <= int(v) < 2 ** 64


def check_noise(noise_multiplier, seed, sequence, tau, quantile, centered: bool):
    """The Gaussian noise of a DP-FedAvg round (McMahan et al. 2018) on the clipped sum: None when
    none is asked for (noise_multiplier None or 0), else (noise_multiplier, sigma, seed, sequence) with
    sigma = fl32(noise_multiplier * tau), the standard deviation added to every column of the SUM (the
    mean's is sigma / N).  ValueError for a multiplier that is no finite number >= 0, and for noise
    without the sensitivity bound it is calibrated to: with quantile= (the radius is then a function
    of the private norms themselves), with tau = inf, and without a centre (an unclipped round);
    for a seed or a sequence that is no integer in [0, 2^64); and for a sigma that leaves fp32's
    range (inf, or 0 from a positive multiplier)."""
    if noise_multiplier is None:
        return None
    if not _is_real(noise_multiplier) or not 0.0 <= float(noise_multiplier) < math.inf:  # NaN fails the comparison
        raise ValueError(f"noise_multiplier must be a finite number >= 0, got {noise_multiplier!r}")
    if float(noise_multiplier) == 0.0:
        return None
    if quantile is not None:
        raise ValueError("noise with quantile= is not supported: the radius would itself depend on the private norms")
    if tau is None or not math.isfinite(float(tau)):
        raise ValueError("noise needs a finite tau: an infinite radius bounds no client's influence")
    if not centered:
        raise ValueError("noise needs a centre: an unclipped round has no sensitivity bound")
    if not _is_u64(seed):
        raise ValueError(f"a noised round needs a seed, an integer in [0, 2^64), got {seed!r}")
    if not _is_u64(sequence):
        raise ValueError(f"sequence must be an integer in [0, 2^64), got {sequence!r}")
    with np.errstate(over="ignore", under="ignore"):
        sigma = float(np.float32(float(noise_multiplier) * float(tau)))
    if not 0.0 < sigma < math.inf:
        raise ValueError(f"sigma = fl32(noise_multiplier * tau) = {sigma!r} leaves fp32's range")
    return float(noise_multiplier), sigma, int(seed), int(sequence)


def _norm2(norm2) -> np.ndarray:
    d2 = np.asarray(norm2, dtype=np.float64)
    if d2.ndim != 1:
        raise ValueError(f"norm2 must be one squared norm per client, got shape {d2.shape}")
    return d2


def clip_radius(norm2, tau, quantile) -> float:
    """The round's radius: tau itself, or the ceil(quantile * F)-th smallest of the F finite norms
    (ValueError for F = 0)."""
    tau, q = check_radius(tau, quantile)
    if tau is not None:
        return tau
    d2 = _norm2(norm2)
    norms = np.sort(np.sqrt(d2[np.isfinite(d2)]))
    if norms.size == 0:
        raise ValueError("no upload has a finite norm: the quantile radius is undefined")
    k = min(max(math.ceil(q * norms.size), 1), norms.size)
    return float(norms[k - 1])


def clip_scales(norm2, tau) -> np.ndarray:
    """fp32 [N]: the factor each client's update is multiplied by (0: replaced by the centre)."""
    d2 = _norm2(norm2)
    tau = float(tau)
    if not tau > 0.0:
        raise ValueError(f"tau must be > 0, got {tau!r}")
    scale = np.zeros(d2.shape, dtype=np.float32)
    finite = np.isfinite(d2)
    norms = np.sqrt(np.where(finite, d2, 0.0))
    inside = finite & (norms <= tau)
    scale[inside] = 1.0
    outside = finite & ~inside  # norms > tau > 0
    ratio = (tau / norms[outside]).astype(np.float32)
    scale[outside] = np.where(ratio >= 1.0, np.float32(1.0), ratio)
    return scale
