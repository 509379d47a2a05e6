"""Int8 block-quantized uploads restated in numpy and plain Python, for the quant tests: the client's
quantizer and dequantizer (flearn_amd/quant.py's rules, written block by block), the
dequantize-and-sum of fa_deq_fold_q8 row by row with a rounding to fp32 after every operation, the
kernel's launch plan (plan_q8_window of flearn_amd/csrc/fa_quant_geometry.hpp, checked against the
C++ by tests/test_quant_host.py), and the table of shipped fa::quant instantiations as
fa_last_launch spells them with the shapes that reach each.  No torch, no flearn_amd."""
from collections import namedtuple

import numpy as np

BLOCK = 1024
W = 4
MAX_V = 2
IN_FLIGHT = 64  # KiB of code rows per block: D = IN_FLIGHT / (V * W)
PIECE_CHUNKS = W * MAX_V
FAMILY = "deq_fold_kernel"
VS = (1, 2)

Plan = namedtuple("Plan", "V W D grid")


def ceil_div(a, b):
    return -(-a // b)


def natural_grid(cus):
    return int(cus * 0.75 + 0.5)


def plan(ncols, cus, forced=0):
    """plan_q8_window: plan_fold_window's rule on 1024-column chunks with pieces of <= 8 chunks."""
    chunks = ceil_div(ncols, BLOCK)
    grid = forced if forced > 0 else natural_grid(cus)
    if forced <= 0 and grid * PIECE_CHUNKS < chunks <= (cus * 13 // 16) * PIECE_CHUNKS:
        grid = ceil_div(chunks, PIECE_CHUNKS)
    grid = max(1, min(grid, chunks))
    share = ceil_div(chunks, grid)
    v = 1
    while v < MAX_V and share > v * W:
        v *= 2
    return Plan(v, W, IN_FLIGHT // (v * W), grid)


def depth(v):
    return IN_FLIGHT // (v * W)


def instance(v):
    """fa_last_launch's spelling of the instantiation with V = v."""
    return f"{FAMILY}<{v},{depth(v)},{W},true>"


TARGETS = {instance(v) for v in VS}
# V -> (columns, forced grid) that reach it on any device: one block whose share is 1 / 5 chunks
COVER = {1: (1 * BLOCK + 1, 2), 2: (4 * BLOCK + 3, 1)}


def n_blocks(numel):
    return ceil_div(int(numel), BLOCK)


# -- the client's side -----------------------------------------------------------------------------
def quantize(x, center=None, stochastic=False, rng=None):
    """(codes int8 of x's shape, scales fp32 [blocks]) of an fp32 array, block by block."""
    x = np.asarray(x, dtype=np.float32)
    flat = x.reshape(-1)
    if center is not None:
        flat = (flat - np.asarray(center, dtype=np.float32).reshape(-1)).astype(np.float32)
    if not np.isfinite(flat).all():
        raise ValueError("non-finite input")
    codes = np.zeros(flat.size, dtype=np.int8)
    scales = np.zeros(n_blocks(flat.size), dtype=np.float32)
    for b in range(len(scales)):
        blk = flat[b * BLOCK : (b + 1) * BLOCK]
        s = np.float32(np.abs(blk).max() / np.float32(127))
        if s == 0:
            continue
        r = (blk / s).astype(np.float32)
        if stochastic:
            lo = np.floor(r)
            q = lo + (rng.random(r.shape) < (r - lo))
        else:
            q = np.rint(r)
        codes[b * BLOCK : (b + 1) * BLOCK] = np.clip(q, -127, 127).astype(np.int8)
        scales[b] = s
    return codes.reshape(x.shape), scales


def col_scales(scales, ncols, col_begin=0):
    """The per-column scale of columns [col_begin, col_begin + ncols) of rows of per-block scales [..., blocks]."""
    cols = np.arange(col_begin, col_begin + ncols) // BLOCK
    return np.asarray(scales, dtype=np.float32)[..., cols]


def dequantize(codes, scales, center=None):
    """fl32(scale * float(q)), and fl32(center + that) with a centre."""
    codes = np.asarray(codes)
    flat = codes.reshape(-1).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (col_scales(scales, flat.size) * flat).astype(np.float32)
        if center is not None:
            x = (np.asarray(center, dtype=np.float32).reshape(-1) + x).astype(np.float32)
    return x.reshape(codes.shape)


# -- fa_deq_fold_q8 -------------------------------------------------------------------------------------
def deq_fold(acc, codes, scales, weights, center=None, col_begin=0):
    """fp32 [cols]: one chunk.  codes int8 [N, cols] (the window's columns), scales fp32 [N, blocks] of
    the whole rows (block b covers the rows' columns [1024 b, 1024 b + 1024); the window starts at
    col_begin), weights fp32 [N], center fp32 [cols] or None.  acc None: the chunk opens the round
    (row 0's product is the sum); else every row's product is added to acc, in list order.  A
    rounding to fp32 after every operation."""
    codes = np.asarray(codes)
    n, cols = codes.shape
    sc = col_scales(scales, cols, col_begin)
    w = np.asarray(weights, dtype=np.float32)
    g = None if center is None else np.asarray(center, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(n):
            x = (sc[i] * codes[i].astype(np.float32)).astype(np.float32)
            if g is not None:
                x = (g + x).astype(np.float32)
            t = (w[i] * x).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
    return acc


def same_bits(a, b):
    """Bit for bit where b (the reference) is not NaN, NaN where it is."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(b)
    iv = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.isnan(a[nan]).all() and (a[~nan].view(iv) == b[~nan].view(iv)).all())
