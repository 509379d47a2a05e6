"""Brute-force numpy restatement of Krum / multi-Krum selection (flearn_amd/krum.py states the rules;
this file restates them independently, with Python loops and sorted() instead of array operations).

  d[i][j]  = G[i][i] + G[j][j] - 2 G[i][j], negative -> 0, non-finite -> +inf
  score[i] = the float64 sum, ascending, of the N - f - 2 smallest d[i][j], j != i; non-finite -> +inf
  selected = the m indices of lowest score, ties to the lower index, in upload order
"""
import math

import numpy as np


def distance(g, i, j):
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float64(g[i][i]) + np.float64(g[j][j]) - np.float64(2.0) * np.float64(g[i][j])
    if not math.isfinite(d):
        return math.inf
    return max(float(d), 0.0)


def scores(g, f):
    n = len(g)
    out = []
    for i in range(n):
        ds = sorted(distance(g, i, j) for j in range(n) if j != i)[: n - f - 2]
        s = np.float64(0.0)
        with np.errstate(over="ignore"):
            for d in ds:
                s = s + np.float64(d)
        out.append(float(s) if math.isfinite(s) else math.inf)
    return out


def select(g, f, m):
    """(sorted indices, scores) or ValueError when a selected score is +inf."""
    sc = scores(g, f)
    ranked = sorted(range(len(g)), key=lambda i: (sc[i], i))[:m]
    if any(math.isinf(sc[i]) for i in ranked):
        raise ValueError("more than f non-finite uploads")
    return sorted(ranked), sc


def score_error(tol, f):
    """Bound on |score_i - exact score_i| when every G entry is within tol[i][j] of the exact Gram:
    each d[i][j] moves by at most tol_ii + tol_jj + 2 tol_ij, and a sum of the k smallest of a set of
    numbers moves by at most the sum of the k largest moves."""
    tol = np.asarray(tol, dtype=np.float64)
    n = tol.shape[0]
    dd = np.diagonal(tol)[:, None] + np.diagonal(tol)[None, :] + 2.0 * tol
    out = np.empty(n)
    for i in range(n):
        out[i] = np.sort(np.delete(dd[i], i))[::-1][: n - f - 2].sum()
    return out
