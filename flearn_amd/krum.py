"""Krum / multi-Krum selection (Blanchard et al., NeurIPS 2017) from a client Gram matrix, on the
host: numpy only, no torch, no GPU.  The engine's Gram kernel (ops.gram_stack) makes the matrix;
Aggregator.ensemble_krum averages the uploads this module selects.

With N uploads of which up to f may be bad, upload i's score is the sum of its squared distances to
its N - f - 2 nearest other uploads; multi-Krum keeps the m uploads of lowest score (Krum: m = 1).
An upload far from the others — scaled, sign-flipped, noise — has a high score and is left out
whole; a non-finite upload has score +inf.
"""
from __future__ import annotations

import numpy as np


def _check_counts(n: int, f, m) -> tuple:
    for name, v in (("f", f), ("m", m)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an int, got {type(v).__name__}")
    f, m = int(f), int(m)
    if f < 0:
        raise ValueError(f"f must be >= 0, got {f}")
    if n < 2 * f + 3:
        raise ValueError(f"Krum needs N >= 2 f + 3 uploads: N = {n}, f = {f}")
    if not 1 <= m <= n - f:
        raise ValueError(f"m must satisfy 1 <= m <= N - f = {n - f}, got {m}")
    return f, m


def check_counts(n_clients: int, f, m) -> tuple:
    """(f, m) as ints, or ValueError: ints only (no bools), f >= 0, N >= 2 f + 3, 1 <= m <= N - f."""
    return _check_counts(int(n_clients), f, m)


def distances(gram) -> np.ndarray:
    """d[i, j] = G[i, i] + G[j, j] - 2 G[i, j] in float64: negative values (rounding) clamped to 0,
    non-finite ones +inf."""
    g = np.asarray(gram, dtype=np.float64)
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise ValueError(f"gram must be a square matrix, got shape {g.shape}")
    diag = np.diagonal(g)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (diag[:, None] + diag[None, :]) - 2.0 * g
        d = np.where(np.isfinite(d), np.maximum(d, 0.0), np.inf)
    return d


def scores(gram, f: int) -> np.ndarray:
    """score[i]: the float64 sum, in ascending order, of the N - f - 2 smallest d[i, j], j != i;
    +inf when it is not finite."""
    d = distances(gram)
    n = d.shape[0]
    keep = n - int(f) - 2
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        row = np.sort(np.delete(d[i], i))[:keep]
        s = np.float64(0.0)
        with np.errstate(over="ignore"):
            for v in row:  # ascending, sequential: the same bits on every host
                s = s + v
        out[i] = s if np.isfinite(s) else np.inf
    return out


def krum_select(gram, f: int, m: int):
    """(selected, scores): the m indices of lowest score — ties go to the lower index — returned in
    upload order (ascending), and every upload's score.  ValueError for bad f / m (check_counts) and
    when a selected upload's score is +inf: more than f uploads were non-finite."""
    g = np.asarray(gram, dtype=np.float64)
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise ValueError(f"gram must be a square matrix, got shape {g.shape}")
    f, m = _check_counts(g.shape[0], f, m)
    sc = scores(g, f)
    order = np.argsort(sc, kind="stable")[:m]  # stable: equal scores keep index order
    if not np.isfinite(sc[order]).all():
        raise ValueError(f"Krum: a selected upload has no finite score: more than f = {f} uploads are non-finite "
                         "(or the centre is)")
    return np.sort(order).astype(np.int64), sc
