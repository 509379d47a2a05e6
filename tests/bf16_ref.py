"""bfloat16 uploads restated in numpy, for the bf16 tests: the exact widening, fa_fold_bf16's sum row
by row with one fp32 rounding per operation, and plan_bf16_window
(flearn_amd/csrc/fa_bf16_geometry.hpp) with fa_last_launch's spelling of the shipped instantiations.
No torch, no flearn_amd."""
import numpy as np

CHUNK, W, MAX_V, IN_FLIGHT = 512, 4, 4, 64
VS = (1, 2, 4)


def depth(v):
    return IN_FLIGHT // (v * W)


def instance(v):  # fa_last_launch's spelling
    return f"widen_fold_kernel<{v},{depth(v)},{W},true>"


def plan_v(ncols, cus, forced=0):
    """(V, grid) of plan_bf16_window: plan_q8_window's rule on 512-column chunks, pieces of <= 16."""
    chunks = -(-ncols // CHUNK)
    grid = forced if forced > 0 else int(cus * 0.75 + 0.5)
    if forced <= 0 and grid * W * MAX_V < chunks <= (cus * 13 // 16) * W * MAX_V:
        grid = -(-chunks // (W * MAX_V))
    grid = max(1, min(grid, chunks))
    share, v = -(-chunks // grid), 1
    while v < MAX_V and share > v * W:
        v *= 2
    return v, grid


def widen(u16):
    return (np.asarray(u16).astype(np.uint32) << 16).view(np.float32)


def fold(acc, rows_u16, weights):
    """fp32 [cols]: acc None opens the round with row 0's product; one fp32 rounding per operation, in list order."""
    w = np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i, row in enumerate(rows_u16):
            t = w[i] * widen(row)
            acc = t if acc is None else acc + t
    return acc


def same_bits(a, b):
    """Bit for bit where b (the reference) is not NaN, NaN where it is."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(b)
    return bool(a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.isnan(a[nan]).all()
                and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all())
