"""The norm-clipped round restated in numpy and plain Python, for the clip tests: the plan of the
norm kernel (plan_rownorm_window of flearn_amd/csrc/fa_geometry.hpp, checked against the C++ by
tests/test_clip_host.py), the derived error bound of the norms, the radius and the scales
(flearn_amd/clip.py's rules, written element by element), and the clipped sum and mean.  No torch,
no flearn_amd."""
import math
from collections import namedtuple

import numpy as np

MAX_CLIENTS = 128
GRID_CAP = 512
PIECE_CHUNKS = 64
W = 4
WAVE_ADDS = 7
U = 2.0 ** -24

Plan = namedtuple("Plan", "V W D chunks pc pieces grid per_block chain workspace_bytes")


def ceil_div(a, b):
    return -(-a // b)


def row_chunks(ncols):
    return ceil_div(ceil_div(ncols, 4), 64)


def natural_grid(cus):
    return int(cus * 0.75 + 0.5)


def plan(n, ncols, cus, forced=0):
    ok = 1 <= n <= MAX_CLIENTS
    chunks = row_chunks(max(ncols, 1))
    grid = forced if forced > 0 else natural_grid(cus)
    if forced <= 0 and grid * PIECE_CHUNKS < chunks <= (cus * 13 // 16) * PIECE_CHUNKS:
        grid = ceil_div(chunks, PIECE_CHUNKS)
    grid = max(1, min(grid, GRID_CAP, chunks))
    share = ceil_div(chunks, grid)
    v = 1
    while v < PIECE_CHUNKS // W and share > v * W:
        v *= 2
    k = ceil_div(chunks, grid * W * v)
    pc = ceil_div(chunks, grid * k)
    pieces = ceil_div(chunks, pc)
    grid = min(grid, pieces)
    per_block = ceil_div(pieces, grid)
    chain = v + 2 + WAVE_ADDS + per_block + W - 1
    return Plan(v if ok else 0, W, PIECE_CHUNKS // (v * W), chunks, pc, pieces, grid, per_block, chain,
                grid * (n if ok else 0) * 4)


def launch_plan(n, ncols, cus, forced=0):
    """What fa_rownorm2_f32 plans on a device of `cus` CUs under fa_set_reduce_grid(forced)."""
    return plan(n, ncols, cus, min(forced, GRID_CAP))


def workspace_bytes(n, ncols):
    return min(GRID_CAP, row_chunks(max(ncols, 1))) * n * 4


def piece_cols(v):
    """The columns of one full piece of the instantiation with V = v."""
    return 256 * v * W


def gamma(k):
    return k * U / (1.0 - k * U)


def norm_bound(p):
    """The relative error bound of a norm under plan p: all terms are squares (non-negative), `chain`
    fp32 roundings lie behind a block's partial and the grid's partials are added in float64."""
    return gamma(p.chain) + p.grid * 2.0 ** -52


def norm2(stack, center=None):
    """float64 [N]: the exact-in-float64 sum of the squares of the fp32 differences fl32(x - g)."""
    x = np.asarray(stack, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x if center is None else (x - np.asarray(center, dtype=np.float32)[None, :]).astype(np.float32)
        d = d.astype(np.float64)
        return (d * d).sum(axis=1)


def radius(norm2_, tau=None, quantile=None):
    if tau is not None:
        return float(tau)
    norms = sorted(math.sqrt(v) for v in norm2_ if math.isfinite(v))
    if not norms:
        raise ValueError("no finite norm")
    return norms[min(max(math.ceil(quantile * len(norms)), 1), len(norms)) - 1]


def scales(norm2_, tau):
    out = []
    for v in norm2_:
        v = float(v)
        if not math.isfinite(v):
            out.append(np.float32(0.0))
        elif math.sqrt(v) <= tau:
            out.append(np.float32(1.0))
        else:
            r = np.float32(tau / math.sqrt(v))
            out.append(np.float32(1.0) if r >= 1 else r)
    return np.array(out, dtype=np.float32)


def clipped_upload(x, g, s):
    """fp32 row: the kernel's three-way rule for scale s (any float, NaN included)."""
    x = np.asarray(x, dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    s = np.float32(s)
    if s >= 1:
        return x.copy()
    if s > 0:
        with np.errstate(invalid="ignore", over="ignore"):
            d = (x - g).astype(np.float32)
            return (g + (s * d).astype(np.float32)).astype(np.float32)
    return g.copy()


def clipped_sum(stack, g, scale):
    """fp32 [cols]: acc = yhat_0; acc = fl32(acc + yhat_i) in list order."""
    acc = clipped_upload(stack[0], g, scale[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, len(stack)):
            acc = (acc + clipped_upload(stack[i], g, scale[i])).astype(np.float32)
    return acc


def clipped_mean(stack, g, scale):
    """float64 [cols]: fl64(acc) / N, the divide of FA_MODE_W32_DIV64."""
    return clipped_sum(stack, g, scale).astype(np.float64) / float(len(stack))


# The shipped instantiations, and a shape that reaches each under fa_set_reduce_grid(1) (one block:
# the share is the window's chunks, V the narrowest piece of W * V chunks that covers it).  The GPU
# tests launch every one and check fa_last_launch; tests/test_clip_inventory.py holds the library's
# symbols to this table.
VS = (1, 2, 4, 8, 16)
COVER = {v: (1000 * v, 1) for v in VS}  # V -> (columns, forced grid)


def instance(family, v):
    return f"{family}<{v},{PIECE_CHUNKS // (v * W)},{W},true>"


TARGETS = {instance(f, v) for f in ("rownorm_kernel", "clip_sum_kernel") for v in VS}
UNRECORDED = {"rownorm_finish_kernel"}  # runs behind rownorm_kernel: launches == 2
