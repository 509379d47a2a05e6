"""Int8, int4, 1-bit sign and Microscaling block-quantized uploads (DESIGN.md sections 17, 18, 21 and 22): the formats,
their checks, and the client's quantizer and dequantizer.  Host-side numpy only, no device code.

A quantized entry of upload["params"] replaces an fp32 tensor of shape S by a plain dict

    {"q8": int8 ndarray of shape S, "scale": float32 ndarray [ceil(numel / 1024)], "block": 1024, "delta": bool}

Block b covers elements [1024 b, 1024 b + 1024) of the tensor flattened in C order, and the value is
fl32(scale[b] * float(q)), one fp32 rounding; all 256 codes are legal.  delta=True: the codes encode
x - g, g the server's previous global model in fp32, and the client's value is
fl32(g + fl32(scale * q)).  In a quantized upload every fp32 tensor is quantized, tensors of other
dtypes (int64 BN counters, float64) are sent plain, float16 is refused.

The 4-bit entry (bits=4) packs two codes into a byte and scales blocks of 128:

    {"q4": uint8 ndarray [ceil(numel / 2)], "shape": tuple S, "scale": float32 ndarray [ceil(numel / 128)],
     "block": 128, "delta": bool}

Element e (C order) is a nibble of byte e >> 1, the low one for even e; codes are two's complement,
-8 ... 7, all 16 legal; block b covers elements [128 b, 128 b + 128); the value and `delta` are q8's.
A scale is finite and either zero or >= Q4_MIN_SCALE = 2^-100: scale / 16 is then exact, which the
device kernel relies on (it converts a nibble in place as 16 q and multiplies by scale / 16).  The
quantizer leaves an odd tensor's spare high nibble 0; on receipt that nibble is ignored, whatever it
holds (it is no element: dequantize_entry drops it, and on the device it lands in a padding column
nobody reads).  One round's uploads are all of one width.

The 1-bit entry (bits=1) is a sign per element and a magnitude per block of 128 (scaled signSGD;
EF-signSGD, Karimireddy et al., ICML 2019):

    {"q1": uint8 ndarray [ceil(numel / 8)], "shape": tuple S, "scale": float32 ndarray [ceil(numel / 128)],
     "block": 128, "delta": bool}

Element e (C order) is bit e % 8 of byte e >> 3; 1 is negative, 0 non-negative (exact zeros, -0.0 and
the last byte's spare bits are 0).  scale[b] is the mean of |x| over the block's real elements,
accumulated in float64 and rounded once to fp32; a legal scale is finite and >= 0.  The value is
copysign(scale[b], -1 if bit else +1) — a bit pattern, not a product — plus the centre for a delta
entry.  A sign code has no zero: the quantizer is biased, and a client keeps the residual
(QuantizedAVG's error_feedback).  Spare bits are ignored on receipt, as q4's spare nibble is.

The Microscaling entries (format="mx"; OCP Microscaling Formats v1.0) scale blocks of 32 by a power of two:

    {"mx4": uint8 ndarray [ceil(numel / 2)], "shape": tuple S, "scale": uint8 ndarray [ceil(numel / 32)],
     "block": 32, "delta": bool}            MXFP4: E2M1 codes, two per byte, the low nibble the even element
    {"mx8": uint8 ndarray [numel], ...}     MXFP8: E4M3 "fn" codes, one per byte

A scale byte e is E8M0 and stands for 2^(e - 127); legal bytes are MX_MIN_EXP = 27 ... MX_MAX_EXP = 227
(2^-100 ... 2^100; 255, E8M0's NaN, is refused with the rest), where every decoded value of both element
types is zero or an fp32 normal, and exact.  An E2M1 code is sign, two exponent bits and a mantissa bit:
+-0, 0.5, 1, 1.5, 2, 3, 4, 6, no inf, no NaN, -0 legal and -0.0.  An E4M3 code has bias 7, maximum 448,
subnormals down to 2^-9, no inf; S.1111.111 is NaN: legal on receipt (the sums are NaN), never emitted.
The value is decode(code) * 2^(e - 127), an exact fp32, plus the centre for a delta entry.  One round's
uploads are all of one format and element type.

Block-wise absmax scaling as in Dettmers et al. (ICLR 2022); quantized client updates as in FedPAQ
(Reisizadeh et al., AISTATS 2020); the stochastic rounding is QSGD's (Alistarh et al., NeurIPS 2017).
"""
from __future__ import annotations

import math

import numpy as np
import torch

BLOCK = 1024  # FA_Q8_BLOCK: one wave-chunk of fa_deq_fold_q8
Q4_BLOCK = 128  # FA_Q4_BLOCK: a sixteenth of fa_deq_fold_q4's wave-chunk
Q4_MIN_SCALE = np.float32(2.0 ** -100)  # FA_Q4_MIN_SCALE: the smallest non-zero scale of a 4-bit entry
Q1_BLOCK = 128  # FA_Q1_BLOCK: a sixteenth of fa_deq_fold_q1's wave-chunk
_F32 = np.dtype(np.float32)
_BLOCK_OF = {8: BLOCK, 4: Q4_BLOCK, 1: Q1_BLOCK}
_LEVELS = {8: 127, 4: 7, 1: 1}
_PACKED = {4: ("q4", 2), 1: ("q1", 8)}  # the widths whose codes are packed bytes: (field, codes per byte)
_BITS_MSG = "bits must be 8, 4 or 1"
MX_BLOCK = 32  # FA_MX_BLOCK: one lane of fa_deq_fold_mx's wave-chunk
MX_MIN_EXP, MX_MAX_EXP = 27, 227  # FA_MX_MIN_EXP, FA_MX_MAX_EXP: the legal E8M0 scale bytes
_MX = {"mx4": 2, "mx8": 1}  # the Microscaling tags: codes per byte
_MX_EMAX = {"mx4": 2, "mx8": 8}  # the exponent of the element format's largest binade (6 = 1.5 * 2^2, 448 = 1.75 * 2^8)
_TAGS = ("q8", "q4", "q1", "mx4", "mx8")


def _mx_table(tag: str) -> np.ndarray:
    """decode(code) for every code of an element type, in float64 from the format's definition."""
    ebits, mbits, bias = (2, 1, 1) if tag == "mx4" else (4, 3, 7)
    c = np.arange(1 << (1 + ebits + mbits))
    ex, man = (c >> mbits) & ((1 << ebits) - 1), c & ((1 << mbits) - 1)
    mag = np.where(ex == 0, man * 2.0 ** (1 - bias - mbits), (1 + man * 2.0 ** -mbits) * 2.0 ** (ex - bias))
    if tag == "mx8":
        mag[(c & 0x7F) == 0x7F] = np.nan
    return np.copysign(mag, np.where(c >> (ebits + mbits), -1.0, 1.0))


MX_TABLE = {tag: _mx_table(tag) for tag in _MX}


def _check_format(bits, format) -> str | None:
    """The Microscaling tag of (bits, format), None for format="int"; ValueError for what is neither."""
    if isinstance(bits, bool) or bits not in _BLOCK_OF:
        raise ValueError(f"{_BITS_MSG}, got {bits!r}")
    if format == "int":
        return None
    if format != "mx":
        raise ValueError(f'format must be "int" or "mx", got {format!r}')
    if bits == 1:
        raise ValueError('format="mx" has 4-bit (MXFP4) and 8-bit (MXFP8) elements: bits=1 is not a Microscaling format')
    return f"mx{bits}"


def width_of(e):
    """What a round's entries must agree on: 8, 4 or 1 for the integer codes, "mx4" / "mx8"."""
    return "mx4" if "mx4" in e else "mx8" if "mx8" in e else bits_of(e)


def n_blocks(numel: int, block: int = BLOCK) -> int:
    return -(-int(numel) // block)


def is_entry(v) -> bool:
    """v is (shaped like) a quantized entry: a dict with a "q8", a "q4", a "q1", an "mx4" or an "mx8"."""
    return isinstance(v, dict) and ("q8" in v or "q4" in v or "q1" in v or "mx4" in v or "mx8" in v)


def bits_of(e) -> int:
    """The code width of a quantized entry."""
    return 4 if "q4" in e or "mx4" in e else 1 if "q1" in e else 8


def entry_shape(e) -> tuple:
    """The shape of the tensor an entry stands for."""
    return tuple(e["q8"].shape) if "q8" in e and "shape" not in e else tuple(e["shape"])


def pack_nibbles(codes: np.ndarray) -> np.ndarray:
    """int8 codes in [-8, 7], flat, as uint8 [ceil(n / 2)]: even elements in the low nibbles, an odd
    count's spare high nibble 0."""
    u = codes.astype(np.uint8) & np.uint8(0xF)
    if u.size & 1:
        u = np.append(u, np.uint8(0))
    return u[0::2] | (u[1::2] << 4)


def unpack_nibbles(q4: np.ndarray, numel: int) -> np.ndarray:
    """pack_nibbles' inverse: the first `numel` sign-extended nibbles of a uint8 array, as int8."""
    out = np.empty(2 * q4.size, dtype=np.int8)
    out[0::2] = (q4 << 4).view(np.int8) >> 4
    out[1::2] = q4.view(np.int8) >> 4
    return out[:numel]


def pack_signs(neg: np.ndarray) -> np.ndarray:
    """A flat bool array (True = negative) as uint8 [ceil(n / 8)]: element e in bit e % 8 of byte e >> 3,
    the last byte's spare bits 0."""
    return np.packbits(neg, bitorder="little")


def unpack_signs(q1: np.ndarray, numel: int) -> np.ndarray:
    """pack_signs' inverse: the first `numel` bits of a uint8 array, as bool."""
    return np.unpackbits(q1, count=numel, bitorder="little").astype(bool)


def is_quantized(params) -> bool:
    """The upload's params carry at least one quantized entry."""
    return hasattr(params, "values") and any(is_entry(v) for v in params.values())


def _host_array(v, what: str) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        if v.device.type != "cpu":
            raise TypeError(f"{what}: device-resident tensors are not taken (host numpy arrays or CPU tensors only)")
        return v.detach().numpy()
    if isinstance(v, (np.ndarray, np.generic)):
        return np.asarray(v)
    raise TypeError(f"{what}: unsupported value type {type(v).__name__} (expected ndarray or Tensor)")


def check_entry(key, e, client=None):
    """(q8, scale, delta) of one quantized entry, as C-contiguous host arrays; client-data errors
    otherwise: ValueError for a block other than 1024, a wrong scale count, a scale that is negative,
    NaN or inf, and a missing field; TypeError for a q8 that is no int8 array (a device-resident one
    included) and a scale that is no float32 array."""
    where = f"key {key!r}" if client is None else f"client {client} key {key!r}"
    if "mx4" in e or "mx8" in e:
        return _check_entry_mx(where, e)
    if "q4" in e:
        return _check_entry4(where, e)
    if "q1" in e:
        return _check_entry4(where, e, 1)
    for f in ("q8", "scale", "block", "delta"):
        if f not in e:
            raise ValueError(f"{where}: quantized entry lacks {f!r}")
    if isinstance(e["block"], bool) or not isinstance(e["block"], (int, np.integer)) or int(e["block"]) != BLOCK:
        raise ValueError(f"{where}: block must be {BLOCK}, got {e['block']!r}")
    if not isinstance(e["delta"], (bool, np.bool_)):
        raise ValueError(f"{where}: delta must be a bool, got {e['delta']!r}")
    q8 = _host_array(e["q8"], f"{where} q8")
    if q8.dtype != np.int8:
        raise TypeError(f"{where}: q8 must be int8, got {q8.dtype}")
    scale = _host_array(e["scale"], f"{where} scale")
    if scale.dtype != _F32:
        raise TypeError(f"{where}: scale must be float32, got {scale.dtype}")
    if scale.ndim != 1 or scale.shape[0] != n_blocks(q8.size):
        raise ValueError(f"{where}: {q8.size} codes need {n_blocks(q8.size)} scales, got shape {tuple(scale.shape)}")
    if not _scales_ok(scale, 8):
        raise ValueError(f"{where}: scales must be finite and >= 0")
    return np.ascontiguousarray(q8), np.ascontiguousarray(scale), bool(e["delta"])


def _check_entry4(where: str, e, bits: int = 4):
    """check_entry for an entry of packed codes, 4-bit or (bits=1) 1-bit: (the code bytes as a
    C-contiguous uint8 array, scale, delta).  Beyond q8's refusals: a missing or malformed shape and a
    code count other than ceil(numel / 2) — 1-bit: ceil(numel / 8) — (ValueError), codes that are no
    uint8 array (TypeError), codes of two widths in one entry, and for 4 bits a scale in
    (0, Q4_MIN_SCALE) (ValueError).  A last byte's spare nibble or bits are not looked at."""
    tag, per = _PACKED[bits]
    for f in (tag, "shape", "scale", "block", "delta"):
        if f not in e:
            raise ValueError(f"{where}: quantized entry lacks {f!r}")
    if sum(t in e for t in ("q8", "q4", "q1")) > 1:
        raise ValueError(f"{where}: an entry carries q4 or q8 codes, not both" if "q1" not in e else
                         f"{where}: an entry carries codes of one width, not both q1 and another")
    if isinstance(e["block"], bool) or not isinstance(e["block"], (int, np.integer)) or int(e["block"]) != _BLOCK_OF[bits]:
        raise ValueError(f"{where}: block must be {_BLOCK_OF[bits]} for {bits}-bit codes, got {e['block']!r}")
    if not isinstance(e["delta"], (bool, np.bool_)):
        raise ValueError(f"{where}: delta must be a bool, got {e['delta']!r}")
    shape = e["shape"]
    if not isinstance(shape, (tuple, list)) or not all(
            isinstance(d, (int, np.integer)) and not isinstance(d, bool) and d >= 0 for d in shape):
        raise ValueError(f"{where}: shape must be a tuple of non-negative ints, got {shape!r}")
    numel = int(np.prod(shape, dtype=np.int64))
    q4 = _host_array(e[tag], f"{where} {tag}")
    if q4.dtype != np.uint8:
        raise TypeError(f"{where}: {tag} must be uint8 ({'two' if bits == 4 else 'eight'} codes per byte), got {q4.dtype}")
    if q4.ndim != 1 or q4.shape[0] != (numel + per - 1) // per:
        raise ValueError(f"{where}: {numel} elements need {(numel + per - 1) // per} code bytes, got shape {tuple(q4.shape)}")
    scale = _host_array(e["scale"], f"{where} scale")
    if scale.dtype != _F32:
        raise TypeError(f"{where}: scale must be float32, got {scale.dtype}")
    if scale.ndim != 1 or scale.shape[0] != n_blocks(numel, Q4_BLOCK):
        raise ValueError(f"{where}: {numel} elements need {n_blocks(numel, Q4_BLOCK)} scales, got shape {tuple(scale.shape)}")
    if not _scales_ok(scale, bits):
        raise ValueError(f"{where}: 4-bit scales must be finite and either 0 or >= 2^-100" if bits == 4 else
                         f"{where}: 1-bit scales must be finite and >= 0")
    return np.ascontiguousarray(q4), np.ascontiguousarray(scale), bool(e["delta"])


def _check_entry_mx(where: str, e):
    """check_entry for a Microscaling entry: (the code bytes as a C-contiguous uint8 array, the scale bytes,
    delta).  ValueError: a missing field, codes of two kinds, a block other than 32, a malformed shape, a
    code or scale count that does not fit it, a scale byte outside MX_MIN_EXP ... MX_MAX_EXP; TypeError:
    codes or scales that are no uint8 array (device-resident ones included).  Every code is legal, E4M3's
    NaNs too; an odd MXFP4 tensor's spare nibble is not looked at."""
    tag = "mx4" if "mx4" in e else "mx8"
    per = _MX[tag]
    for f in (tag, "shape", "scale", "block", "delta"):
        if f not in e:
            raise ValueError(f"{where}: quantized entry lacks {f!r}")
    if sum(t in e for t in _TAGS) > 1:
        raise ValueError(f"{where}: an entry carries codes of one format, not {tag} and another")
    if isinstance(e["block"], bool) or not isinstance(e["block"], (int, np.integer)) or int(e["block"]) != MX_BLOCK:
        raise ValueError(f"{where}: block must be {MX_BLOCK} for Microscaling codes, got {e['block']!r}")
    if not isinstance(e["delta"], (bool, np.bool_)):
        raise ValueError(f"{where}: delta must be a bool, got {e['delta']!r}")
    shape = e["shape"]
    if not isinstance(shape, (tuple, list)) or not all(
            isinstance(d, (int, np.integer)) and not isinstance(d, bool) and d >= 0 for d in shape):
        raise ValueError(f"{where}: shape must be a tuple of non-negative ints, got {shape!r}")
    numel = int(np.prod(shape, dtype=np.int64))
    codes = _host_array(e[tag], f"{where} {tag}")
    if codes.dtype != np.uint8:
        raise TypeError(f"{where}: {tag} must be uint8, got {codes.dtype}")
    if codes.ndim != 1 or codes.shape[0] != (numel + per - 1) // per:
        raise ValueError(f"{where}: {numel} elements need {(numel + per - 1) // per} code bytes, got shape {tuple(codes.shape)}")
    scale = _host_array(e["scale"], f"{where} scale")
    if scale.dtype != np.uint8:
        raise TypeError(f"{where}: Microscaling scales must be uint8 (E8M0), got {scale.dtype}")
    if scale.ndim != 1 or scale.shape[0] != n_blocks(numel, MX_BLOCK):
        raise ValueError(f"{where}: {numel} elements need {n_blocks(numel, MX_BLOCK)} scales, got shape {tuple(scale.shape)}")
    if not _scales_ok(scale, tag):
        raise ValueError(f"{where}: Microscaling scale bytes must be {MX_MIN_EXP} ... {MX_MAX_EXP} (2^-100 ... 2^100)")
    return np.ascontiguousarray(codes), np.ascontiguousarray(scale), bool(e["delta"])


def _scales_ok(scale: np.ndarray, bits) -> bool:
    """Finite and >= 0 (-0.0 passes: it is a zero); 4-bit: and none in (0, Q4_MIN_SCALE); Microscaling
    ("mx4" / "mx8"): bytes in MX_MIN_EXP ... MX_MAX_EXP."""
    if bits in _MX:
        return bool(((scale >= MX_MIN_EXP) & (scale <= MX_MAX_EXP)).all())
    ok = np.isfinite(scale).all() and (scale >= 0).all()
    return bool(ok and (bits != 4 or ((scale == 0) | (scale >= Q4_MIN_SCALE)).all()))


# -- the client's side -----------------------------------------------------------------------------
def _blocks(flat: np.ndarray, block: int = BLOCK) -> np.ndarray:
    """flat padded with zeros to whole blocks, as [blocks, block]"""
    nb = n_blocks(flat.size, block)
    if flat.size == nb * block:
        return flat.reshape(nb, block)
    out = np.zeros(nb * block, dtype=flat.dtype)
    out[: flat.size] = flat
    return out.reshape(nb, block)


def _floor_log2(a: np.ndarray) -> np.ndarray:
    """floor(log2(a)) of positive floats, exactly (frexp: a = m * 2^e with 0.5 <= m < 1)."""
    return np.frexp(a)[1].astype(np.int64) - 1


def _quantize_mx(flat: np.ndarray, shape, tag: str, delta: bool) -> dict:
    """quantize_array's Microscaling rule on the flat fp32 values (centre already subtracted, finite): per
    block of 32, e = floor(log2(absmax)) - emax + 127 clamped into MX_MIN_EXP ... MX_MAX_EXP (an all-zero
    block: MX_MIN_EXP); a code is x / 2^(e - 127) — exact in float64 — rounded to nearest even in the
    element format and saturated at the format's maximum, found in the table of magnitudes."""
    b = _blocks(flat.astype(np.float64), MX_BLOCK)
    amax = np.abs(b).max(axis=1, initial=0.0)
    e = np.full(amax.shape, MX_MIN_EXP, dtype=np.int64)
    live = amax > 0
    e[live] = np.clip(_floor_log2(amax[live]) - _MX_EMAX[tag] + 127, MX_MIN_EXP, MX_MAX_EXP)
    r = np.ldexp(b, (127 - e)[:, None])
    mbits, emin = (1, 0) if tag == "mx4" else (3, -6)  # mantissa bits, the smallest normal binade
    mags = np.abs(MX_TABLE[tag][: 8 if tag == "mx4" else 127])  # the non-negative codes' values, ascending
    a = np.abs(r)
    ex = np.maximum(_floor_log2(np.where(a > 0, a, 1.0)), emin)
    quantum = np.ldexp(1.0, ex - mbits)
    q = np.minimum(np.rint(a / quantum) * quantum, mags[-1])  # rint: ties to the even mantissa
    codes = np.searchsorted(mags, q).astype(np.uint8) | (np.signbit(r).astype(np.uint8) << (3 if tag == "mx4" else 7))
    codes = codes.reshape(-1)[: flat.size]
    if tag == "mx4":
        if codes.size & 1:
            codes = np.append(codes, np.uint8(0))
        codes = codes[0::2] | (codes[1::2] << 4)
    return {tag: codes, "shape": tuple(shape), "scale": e.astype(np.uint8), "block": MX_BLOCK, "delta": delta}


def quantize_array(x: np.ndarray, center=None, stochastic: bool = False, rng=None, bits: int = 8, format: str = "int") -> dict:
    """One fp32 array as a quantized entry.  bits=4: blocks of 128, s = fl32(amax / 7), codes clipped
    to -7 ... 7 and packed two per byte, a block with s < 2^-100 gets scale 0 and codes 0, and
    |dequantized - x| <= s * (0.5 + 2^-20).  bits=8, per block: amax = max|x|, s = fl32(amax / 127), codes
    clip(rint(fl32(x / s)), -127, 127) (round half to even); s == 0 (an all-zero block, or amax / 127
    underflowing) gives codes 0 and scale 0.  stochastic: x / s is rounded up with probability equal
    to its fractional part (unbiased), with `rng` (a numpy.random.Generator).  center: x - center is
    quantized, in fp32, and the entry is marked delta.  Non-finite input: ValueError.  bits=1: blocks of
    128, the code is x < 0 and s = fl32(the float64 mean of |x| over the block's real elements), the
    minimiser of the block's squared error for sign codes; stochastic=True is refused (the unbiased 1-bit
    rule needs s = max|x|: another scale).  format="mx": bits=4 is MXFP4 and bits=8 MXFP8 (_quantize_mx has
    the rule); stochastic=True is refused for it."""
    tag = _check_format(bits, format)
    if tag and stochastic:
        raise ValueError('stochastic rounding is not implemented for format="mx"')
    if bits == 1 and stochastic:
        raise ValueError("stochastic rounding is not defined for bits=1 (the scale is the mean magnitude)")
    block, top = _BLOCK_OF[bits], _LEVELS[bits]
    x = np.asarray(x)
    if x.dtype != _F32:
        raise TypeError(f"only float32 arrays are quantized, got {x.dtype}")
    shape = x.shape
    flat = np.ascontiguousarray(x).reshape(-1)
    if center is not None:
        c = np.asarray(center)
        if c.size != flat.size:
            raise ValueError(f"center has {c.size} elements, the array has {flat.size}")
        with np.errstate(over="ignore", invalid="ignore"):  # an overflowing difference is refused below
            flat = flat - np.ascontiguousarray(c, dtype=np.float32).reshape(-1)
    if not np.isfinite(flat).all():
        raise ValueError("non-finite values cannot be quantized")
    if tag:
        return _quantize_mx(flat, shape, tag, center is not None)
    if bits == 1:
        b = _blocks(np.abs(flat).astype(np.float64), block)
        real = np.minimum(block, flat.size - block * np.arange(b.shape[0]))  # the last block's real elements
        scale = (b.sum(axis=1) / real).astype(np.float32)
        return {"q1": pack_signs(flat < 0), "shape": tuple(shape), "scale": scale, "block": block,
                "delta": center is not None}
    b = _blocks(flat, block)
    s = (np.abs(b).max(axis=1, initial=np.float32(0)) / np.float32(top)).astype(np.float32)
    live = s > 0 if bits == 8 else s >= Q4_MIN_SCALE
    r = np.zeros_like(b)
    np.divide(b, s[:, None], out=r, where=live[:, None])
    if stochastic:
        if rng is None:
            raise ValueError("stochastic rounding needs rng (a numpy.random.Generator)")
        lo = np.floor(r)
        q = lo + (rng.random(r.shape) < (r - lo))
    else:
        q = np.rint(r)
    codes = np.clip(q, -top, top).astype(np.int8).reshape(-1)[: flat.size]
    scale = np.where(live, s, np.float32(0)).astype(np.float32)
    if bits == 4:
        return {"q4": pack_nibbles(codes), "shape": tuple(shape), "scale": scale, "block": block,
                "delta": center is not None}
    return {"q8": codes.reshape(shape), "scale": scale, "block": block, "delta": center is not None}


def dequantize_entry(e, center=None, key=None) -> np.ndarray:
    """fl32(scale[b] * float(q)) — 1-bit: scale[b] with the code's sign — and fl32(center + that) for a
    delta entry: the client's values."""
    codes, scale, delta = check_entry(key, e)
    shape = entry_shape(e)
    numel = int(np.prod(shape, dtype=np.int64))
    if "q4" in e:
        codes = unpack_nibbles(codes, numel)
    block = MX_BLOCK if width_of(e) in _MX else _BLOCK_OF[bits_of(e)]
    if width_of(e) in _MX:
        if "mx4" in e:
            codes = np.stack([codes & 0xF, codes >> 4], axis=1).reshape(-1)
        two = np.ldexp(1.0, scale.astype(np.int64) - 127)
        x = (MX_TABLE[width_of(e)][codes[:numel]] * np.repeat(two, block)[:numel]).astype(np.float32)  # exact
    elif "q1" in e:
        x = np.copysign(np.repeat(scale, block)[:numel], np.where(unpack_signs(codes, numel), np.float32(-1), np.float32(1)))
    else:
        with np.errstate(over="ignore"):  # a scale near the top of the range: the product is +-inf, as on the device
            x = (_blocks(codes.reshape(-1).astype(np.float32), block) * scale[:, None]).astype(np.float32).reshape(-1)[: codes.size]
    if delta:
        if center is None:
            raise ValueError(f"key {key!r}: a delta entry needs the centre it was taken against")
        c = np.ascontiguousarray(_host_array(center, f"center[{key!r}]"), dtype=np.float32).reshape(-1)
        if c.size != x.size:
            raise ValueError(f"center[{key!r}] has {c.size} elements, the entry has {x.size}")
        x = (c + x).astype(np.float32)
    return x.reshape(shape)


def quantize_state_dict(sd, center=None, stochastic: bool = False, rng=None, bits: int = 8, format: str = "int") -> dict:
    """A state dict (numpy arrays or host torch tensors) as a quantized upload's params: every fp32
    tensor becomes a quantized entry (quantize_array), tensors of other dtypes are passed on as numpy
    arrays, float16 raises TypeError.  center: a w_glob-like dict; its values, cast to fp32, are
    subtracted before quantizing and the entries are marked delta=True.  bits: 8, 4 or 1 (1: no
    stochastic rounding).  format: "int" or "mx" (Microscaling: bits 4 or 8, no stochastic rounding)."""
    if _check_format(bits, format) and stochastic:
        raise ValueError('stochastic rounding is not implemented for format="mx"')
    if bits == 1 and stochastic:
        raise ValueError("stochastic rounding is not defined for bits=1 (the scale is the mean magnitude)")
    if stochastic and rng is None:
        raise ValueError("stochastic rounding needs rng (a numpy.random.Generator)")
    out = {}
    for k, v in sd.items():
        a = _host_array(v, f"key {k!r}")
        if a.dtype == np.float16:
            raise TypeError(f"key {k!r}: float16 tensors are not quantized (quantize the fp32 model)")
        if a.dtype != _F32:
            out[k] = a
            continue
        c = None
        if center is not None:
            if k not in center:
                raise ValueError(f"center has no key {k!r}")
            c = np.asarray(_host_array(center[k], f"center[{k!r}]"), dtype=np.float32)
        out[k] = quantize_array(a, c, stochastic, rng, bits, format)
    return out


def dequantize_state_dict(qsd, center=None) -> dict:
    """quantize_state_dict's inverse up to the quantization: fp32 arrays for the quantized entries
    (delta entries added to `center` cast to fp32), everything else as it is."""
    out = {}
    for k, v in qsd.items():
        if is_entry(v):
            c = None
            if v.get("delta"):
                if center is None or k not in center:
                    raise ValueError(f"key {k!r}: a delta entry needs the centre it was taken against")
                c = center[k]
            out[k] = dequantize_entry(v, c, k)
        else:
            out[k] = v
    return out


# -- the server's side: one round's uploads ----------------------------------------------------------
def _dtype_name(v) -> str:
    return str(getattr(v, "dtype", "")).replace("torch.", "")


def check_round(w_local_lst, keys):
    """(qkeys, delta, entries, scales, bits) of a round of quantized uploads over the selected `keys`,
    or client-data errors.  qkeys: the selected keys that are quantized, in order; delta: the round's
    flag; entries[i][key] = (codes, scale) as checked host arrays (q8: int8 of the tensor's shape, q4:
    and q1: the packed uint8 bytes); scales[i]: client i's scales of all qkeys in order, one array; bits:
    the round's code width, 8, 4 or 1, or its Microscaling tag, "mx4" / "mx8" (scales are then E8M0 bytes).  ValueError: entries of two widths in one round (across clients or keys),
    a key quantized by some clients and plain in others, a
    plain fp32 tensor, mixed delta flags, codes of different shapes, and check_entry's; TypeError:
    float16 tensors, and check_entry's.  A well-formed numpy entry costs a few attribute reads; a
    client's scales are looked at once, together."""
    qkeys = [k for k in keys if is_entry(w_local_lst[0][k])]
    qset = set(qkeys)
    delta = bits = None
    entries, scales = [], []
    shapes = {}
    for i, w in enumerate(w_local_lst):
        mine = {}
        for k in keys:
            v = w[k]
            if is_entry(v) != (k in qset):
                raise ValueError(f"client {i} key {k!r}: quantized in some uploads and plain fp32 in others")
            if k not in qset:
                if _dtype_name(v) == "float16":
                    raise TypeError(f"client {i} key {k!r}: float16 tensors in a quantized upload are not supported")
                if _dtype_name(v) == "float32":
                    raise ValueError(f"client {i} key {k!r}: a plain fp32 tensor in a quantized upload "
                                     "(every fp32 tensor is quantized)")
                continue
            if bits is None:
                bits = width_of(v)
            elif width_of(v) != bits and (bits in _MX or width_of(v) in _MX):
                raise ValueError(f"client {i} key {k!r}: {width_of(v)} codes in a round of {bits} uploads (a round's "
                                 "uploads are all of one format: integer codes of one width, mx4 or mx8)")
            elif width_of(v) != bits:
                raise ValueError(f"client {i} key {k!r}: {bits_of(v)}-bit codes in a round of {bits}-bit uploads "
                                 + ("(a round's uploads are all q8 or all q4)" if {bits, bits_of(v)} == {8, 4} else
                                    "(a round's uploads are all of one width: q8, q4 or q1)"))
            if bits in _PACKED or bits in _MX:
                tag, per, blk, sdt = (bits, _MX[bits], MX_BLOCK, np.uint8) if bits in _MX else (*_PACKED[bits], Q4_BLOCK, _F32)
                q8, sc, d, shape = v.get(tag), v.get("scale"), v.get("delta"), v.get("shape")
                if not (type(q8) is np.ndarray and type(sc) is np.ndarray and q8.dtype == np.uint8 and sc.dtype == sdt
                        and type(shape) is tuple and all(type(n) is int and n >= 0 for n in shape)
                        and sum(t in v for t in _TAGS) == 1
                        and q8.ndim == 1 and q8.shape[0] == (math.prod(shape) + per - 1) // per and sc.ndim == 1
                        and sc.shape[0] == n_blocks(math.prod(shape), blk) and type(v.get("block")) is int
                        and v["block"] == blk and type(d) is bool and q8.flags.c_contiguous and sc.flags.c_contiguous):
                    q8, sc, d = check_entry(k, v, i)  # raises what is wrong, or hands back the packed bytes as host arrays
                    shape = entry_shape(v)
            else:
                q8, sc, d = v.get("q8"), v.get("scale"), v.get("delta")
                if not (type(q8) is np.ndarray and type(sc) is np.ndarray and q8.dtype == np.int8 and sc.dtype == _F32
                        and sc.ndim == 1 and sc.shape[0] == n_blocks(q8.size) and type(v.get("block")) is int
                        and v["block"] == BLOCK and type(d) is bool and q8.flags.c_contiguous and sc.flags.c_contiguous):
                    q8, sc, d = check_entry(k, v, i)  # raises what is wrong, or hands back the entry as host arrays
                shape = q8.shape
            if delta is None:
                delta = d
            elif d != delta:
                raise ValueError(f"client {i} key {k!r}: delta={d} in a round of delta={delta} uploads")
            if shape != shapes.setdefault(k, shape):
                raise ValueError(f"client {i} key {k!r}: codes of shape {shape} do not match client 0's {shapes[k]}")
            mine[k] = (q8, sc)
        cat = np.concatenate([mine[k][1] for k in qkeys]) if qkeys else np.zeros(0, np.float32)
        if not _scales_ok(cat, bits or 8):
            for k in qkeys:
                check_entry(k, w[k], i)  # names the key
        entries.append(mine)
        scales.append(cat)
    return qkeys, bool(delta), entries, scales, bits or 8
