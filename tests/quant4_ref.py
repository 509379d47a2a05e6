"""Int4 block-quantized uploads restated in numpy and plain Python: the nibble pack and unpack, the
quantizer block by block, fa_deq_fold_q4 row by row with a rounding to fp32 after every operation, and
plan_q4_window with the shipped instantiations' spelling.  No torch, no flearn_amd."""
from collections import namedtuple

import numpy as np

from quant_ref import same_bits  # noqa: F401  (the comparison the quant4 tests use)

BLOCK = 128
CHUNK = 2048
MIN_SCALE = np.float32(2.0 ** -100)
W, VS = 4, (1,)  # waves per block, the shipped chunks per wave
PIECE_CHUNKS = W * max(VS)
Plan = namedtuple("Plan", "V W D grid")


def depth(v):
    return 64 // (v * W)  # 64 KiB of code rows in flight per block


def instance(v):  # fa_last_launch's spelling
    return f"deq_fold4_kernel<{v},{depth(v)},{W},true>"


TARGETS = {instance(v) for v in VS}


def plan(ncols, cus, forced=0):
    """plan_q4_window: two blocks per CU on 2048-column chunks, the narrowest shipped piece for the share."""
    chunks = -(-ncols // CHUNK)
    grid = max(1, min(forced if forced > 0 else 2 * cus, chunks))
    v = min([v for v in VS if -(-chunks // grid) <= v * W] or [max(VS)])
    return Plan(v, W, depth(v), grid)


def pack(codes):
    """int8 codes in [-8, 7] (flat) as bytes: element e in byte e >> 1, even e in the low nibble."""
    codes = np.asarray(codes, dtype=np.int8).reshape(-1)
    out = np.zeros((codes.size + 1) // 2, dtype=np.uint8)
    for e, q in enumerate(codes.tolist()):
        out[e >> 1] |= (q & 0xF) << (4 * (e & 1))
    return out


def unpack(q4, numel):
    """The first `numel` nibbles of `q4` [..., bytes], sign-extended, as int8 [..., numel]."""
    q4 = np.asarray(q4, dtype=np.uint8)
    nib = np.stack([q4 & 0xF, q4 >> 4], axis=-1).reshape(*q4.shape[:-1], -1).astype(np.int16)
    return np.where(nib >= 8, nib - 16, nib).astype(np.int8)[..., :numel]


def quantize(x, center=None, stochastic=False, rng=None):
    """(packed codes uint8 [ceil(numel / 2)], scales fp32 [blocks]) of an fp32 array, block by block."""
    flat = np.asarray(x, dtype=np.float32).reshape(-1)
    if center is not None:
        flat = (flat - np.asarray(center, dtype=np.float32).reshape(-1)).astype(np.float32)
    if not np.isfinite(flat).all():
        raise ValueError("non-finite input")
    codes = np.zeros(flat.size, dtype=np.int8)
    scales = np.zeros(-(-flat.size // BLOCK), dtype=np.float32)
    for b in range(len(scales)):
        blk = flat[b * BLOCK : (b + 1) * BLOCK]
        s = np.float32(np.abs(blk).max() / np.float32(7))
        if s < MIN_SCALE:
            continue
        r = (blk / s).astype(np.float32)
        if stochastic:
            lo = np.floor(r)
            q = lo + (rng.random(r.shape) < (r - lo))
        else:
            q = np.rint(r)
        codes[b * BLOCK : (b + 1) * BLOCK] = np.clip(q, -7, 7).astype(np.int8)
        scales[b] = s
    return pack(codes), scales


def col_scales(scales, ncols, col_begin=0):
    """The per-column scale of columns [col_begin, col_begin + ncols) of rows of per-block scales [..., blocks]."""
    return np.asarray(scales, dtype=np.float32)[..., np.arange(col_begin, col_begin + ncols) // BLOCK]


def deq_fold4(acc, q4, scales, weights, ncols, center=None, col_begin=0):
    """fp32 [ncols]: one chunk of fa_deq_fold_q4 over columns [col_begin, col_begin + ncols) of whole rows
    q4 uint8 [N, bytes] with scales fp32 [N, blocks]; center is the window's.  acc None opens the round (row
    0's product is the sum); else every product is added, in list order, each operation rounded to fp32."""
    q4 = np.asarray(q4)
    codes = unpack(q4, 2 * q4.shape[1])[:, col_begin : col_begin + ncols]
    sc = col_scales(scales, ncols, col_begin)
    w = np.asarray(weights, dtype=np.float32)
    g = None if center is None else np.asarray(center, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(codes.shape[0]):
            x = (sc[i] * codes[i].astype(np.float32)).astype(np.float32)
            if g is not None:
                x = (g + x).astype(np.float32)
            t = (w[i] * x).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
    return acc


def dequantize(q4, numel, scales, center=None):
    """fl32(scale * float(q)), and fl32(center + that) with a centre, flat: one row under weight 1."""
    g = None if center is None else np.asarray(center, dtype=np.float32).reshape(-1)
    return deq_fold4(None, np.asarray(q4)[None], np.asarray(scales)[None], [1.0], numel, g)
