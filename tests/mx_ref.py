"""OCP Microscaling uploads restated in numpy: the E2M1 and E4M3 tables built in float64 from the
format's definition, the quantizer's rule element by element, and fa_deq_fold_mx row by row with a
rounding to fp32 after every operation.  No torch, no flearn_amd."""
import math

import numpy as np

from quant_ref import same_bits  # noqa: F401  (bit equality, NaN where the reference has NaN)

BLOCK, CHUNK = 32, 2048
MIN_EXP, MAX_EXP = 27, 227
W, V = 4, 1  # waves per block, chunks per wave
D = {4: 8, 8: 8}  # rows in flight, per element type: the shipped depths


def _table(ebits, mbits, bias, nan_code=None):
    out = np.zeros(1 << (1 + ebits + mbits))
    for c in range(out.size):
        ex, man = (c >> mbits) & ((1 << ebits) - 1), c & ((1 << mbits) - 1)
        mag = man * 2.0 ** (1 - bias - mbits) if ex == 0 else (1 + man / (1 << mbits)) * 2.0 ** (ex - bias)
        if nan_code is not None and c & nan_code == nan_code:
            mag = math.nan
        out[c] = -mag if c >> (ebits + mbits) else mag
    return out


TABLE = {4: _table(2, 1, 1), 8: _table(4, 3, 7, nan_code=0x7F)}  # 16 and 256 entries
EMAX = {4: 2, 8: 8}


def codes_of(stack, elem):
    """uint8 [N, bytes] -> the codes [N, columns]: FP4's low nibble is the even column."""
    stack = np.asarray(stack, dtype=np.uint8)
    if elem == 8:
        return stack
    return np.stack([stack & 0xF, stack >> 4], axis=-1).reshape(stack.shape[0], -1)


def deq_fold(acc, stack, scales, weights, ncols, elem, center=None, col_begin=0):
    """fp32 [ncols]: one chunk of fa_deq_fold_mx over columns [col_begin, col_begin + ncols) of whole
    rows `stack` uint8 [N, bytes] with scale bytes uint8 [N, blocks]; center is the window's.  acc None
    opens the round (row 0's product is the sum); else every product is added, in list order."""
    cols = np.arange(col_begin, col_begin + ncols)
    codes = codes_of(stack, elem)[:, cols]
    two = 2.0 ** (np.asarray(scales)[:, cols // BLOCK].astype(np.float64) - 127)
    w = np.asarray(weights, dtype=np.float32)
    g = None if center is None else np.asarray(center, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(codes.shape[0]):
            x64 = TABLE[elem][codes[i]] * two[i]
            x = x64.astype(np.float32)
            assert (np.isnan(x64) | (x.astype(np.float64) == x64)).all()  # exact
            if g is not None:
                x = (g + x).astype(np.float32)
            t = (w[i] * x).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
    return acc


def quantize(x, elem):
    """(codes uint8 [numel], scale bytes): the rule in float64, one element at a time — e = floor(log2
    (absmax)) - emax + 127 clamped (an all-zero block: MIN_EXP); the code is the nearest table value to
    x / 2^(e - 127), ties to the even code, saturated at the largest finite one."""
    flat = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    mags = [v for v in TABLE[elem][: TABLE[elem].size // 2] if not math.isnan(v)]
    codes, scales = np.zeros(flat.size, dtype=np.uint8), []
    for b in range(0, flat.size, BLOCK):
        amax = np.abs(flat[b : b + BLOCK]).max()
        e = MIN_EXP if amax == 0 else min(MAX_EXP, max(MIN_EXP, math.frexp(amax)[1] - 1 - EMAX[elem] + 127))
        scales.append(e)
        for j in range(b, min(b + BLOCK, flat.size)):
            r = abs(flat[j]) / 2.0 ** (e - 127)
            best = min(range(len(mags)), key=lambda c: (abs(mags[c] - r), c & 1))  # even code: even mantissa
            codes[j] = best | (int(np.signbit(flat[j])) << (3 if elem == 4 else 7))
    return codes, np.array(scales, dtype=np.uint8)
