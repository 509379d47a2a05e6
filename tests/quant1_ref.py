"""1-bit sign uploads restated in numpy and plain Python: the bit pack and unpack, the scale rule block by
block, fa_deq_fold_q1 row by row with a rounding to fp32 after every operation, and plan_q1_window with
the shipped instantiation's spelling.  No torch, no flearn_amd."""
import numpy as np

from quant_ref import same_bits  # noqa: F401  (the comparison the quant1 tests use)

BLOCK = 128
CHUNK = 2048
W, V, D = 4, 1, 8  # waves per block, chunks per wave, rows in flight
PIECE_CHUNKS = W * V
INSTANCE = f"sign_fold_kernel<{V},{D},{W},true>"  # fa_last_launch's spelling


def grid(ncols, cus, forced=0):
    """plan_q1_window's grid: three blocks per CU on 2048-column chunks, never more blocks than chunks."""
    return max(1, min(forced if forced > 0 else 3 * cus, -(-ncols // CHUNK)))


def pack(neg):
    """Flat bools (True = negative) as bytes: element e in bit e % 8 of byte e >> 3."""
    out = np.zeros((len(neg) + 7) // 8, dtype=np.uint8)
    for e, b in enumerate(neg):
        out[e >> 3] |= int(bool(b)) << (e & 7)
    return out


def unpack(q1, numel):
    """The first `numel` bits of `q1` [..., bytes] as bool [..., numel]."""
    q1 = np.asarray(q1, dtype=np.uint8)
    bits = (q1[..., None] >> np.arange(8, dtype=np.uint8)) & 1
    return bits.reshape(*q1.shape[:-1], -1)[..., :numel].astype(bool)


def quantize(x, center=None):
    """(packed signs uint8 [ceil(numel / 8)], scales fp32 [blocks]): bit = x < 0, scale = the float64 mean
    of |x| over the block's real elements, rounded once."""
    flat = np.asarray(x, dtype=np.float32).reshape(-1)
    if center is not None:
        flat = (flat - np.asarray(center, dtype=np.float32).reshape(-1)).astype(np.float32)
    scales = np.zeros(-(-flat.size // BLOCK), dtype=np.float32)
    for b in range(len(scales)):
        blk = np.abs(flat[b * BLOCK : (b + 1) * BLOCK]).astype(np.float64)
        scales[b] = np.float32(blk.sum() / blk.size)
    return pack(flat < 0), scales


def deq_fold1(acc, q1, scales, weights, ncols, center=None, col_begin=0):
    """fp32 [ncols]: one chunk of fa_deq_fold_q1 over columns [col_begin, col_begin + ncols) of whole rows
    q1 uint8 [N, bytes] with scales fp32 [N, blocks]; center is the window's.  acc None opens the round (row
    0's product is the sum); else every product is added, in list order, each operation rounded to fp32."""
    q1 = np.asarray(q1)
    neg = unpack(q1, 8 * q1.shape[1])[:, col_begin : col_begin + ncols]
    sc = np.asarray(scales, dtype=np.float32)[:, np.arange(col_begin, col_begin + ncols) // BLOCK]
    w = np.asarray(weights, dtype=np.float32)
    g = None if center is None else np.asarray(center, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(neg.shape[0]):
            x = np.copysign(sc[i], np.where(neg[i], np.float32(-1), np.float32(1))).astype(np.float32)
            if g is not None:
                x = (g + x).astype(np.float32)
            t = (w[i] * x).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
    return acc


def dequantize(q1, numel, scales, center=None):
    """The scale with the code's sign, and fl32(center + that) with a centre, flat: one row under weight 1."""
    return deq_fold1(None, np.asarray(q1)[None], np.asarray(scales)[None], [1.0], numel, center)
