"""The Gram kernel's numpy reference, its derived error bound, and plan_gram_window restated in Python
(tests/test_gram_host.py pins the restatement to flearn_amd/csrc/fa_geometry.hpp through
tests/gram_geometry_probe.cpp; the GPU tests take `chain` and `grid` of a launch from it)."""
from typing import NamedTuple

import numpy as np

MAX_CLIENTS = 128
LC = 1024
GRID_CAP = 512  # fa_gram_f32: the most blocks of a launch, what fa_gram_workspace sizes for
U = 2.0 ** -24


class GramPlan(NamedTuple):
    np_: int
    kc: int
    lc: int
    chunks: int
    grid: int
    share: int
    chain: int
    workspace_bytes: int


def gram_np(n):
    return 0 if n < 1 or n > MAX_CLIENTS else -(-n // 32) * 32


def gram_kc(np_):
    return 512 if np_ <= 32 else 256 if np_ <= 64 else 128


def plan(n_clients, n_cols, cus, forced=0):
    np_ = gram_np(n_clients)
    side = np_ or 32
    kc = gram_kc(side)
    chunks = -(-max(n_cols, 1) // kc)
    grid = max(1, min(forced if forced > 0 else cus, chunks))
    share = -(-chunks // grid) * kc
    return GramPlan(np_, kc, LC, chunks, grid, share, LC + -(-share // LC), grid * side * side * 4)


def launch_plan(n_clients, n_cols, cus, forced=0):
    """The plan fa_gram_f32 launches with on a device of `cus` CUs under fa_set_reduce_grid(forced)."""
    return plan(n_clients, n_cols, min(cus, GRID_CAP), min(forced, GRID_CAP))


def workspace_bytes(n_clients, n_cols):
    return plan(n_clients, n_cols, GRID_CAP, 0).workspace_bytes


def centred(x, c=None):
    """y = fl32(x - c): one float32 subtract."""
    x = np.asarray(x, dtype=np.float32)
    return x if c is None else (x - np.asarray(c, dtype=np.float32)[None, :]).astype(np.float32)


def gram(x, c=None):
    """G_ref = y64 @ y64.T with y64 the float64 image of the float32 y."""
    y = centred(x, c).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return y @ y.T


def gamma(n):
    return n * U / (1.0 - n * U)


def bound(x, c, p):
    """|G - G_ref| <= gamma(chain) * S + grid * 2^-52 * S, S = |y64| @ |y64|.T: every entry of a
    block's partial is behind at most `chain` fp32 roundings, and the float64 sum of the `grid`
    partials adds one 2^-53 rounding each (2^-52 bounds gamma_grid in float64 with room)."""
    y = np.abs(centred(x, c).astype(np.float64))
    s = y @ y.T
    return gamma(p.chain) * s + p.grid * 2.0 ** -52 * s
