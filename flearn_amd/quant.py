"""Int8 block-quantized uploads: the format, its checks, and the client's
quantizer and dequantizer.  Host-side numpy only, no device code.

A quantized entry of upload["params"] replaces an fp32 tensor of shape S by a plain dict

    {"q8": int8 ndarray of shape S, "scale": float32 ndarray [ceil(numel / 1024)], "block": 1024, "delta": bool}

Block b covers elements [1024 b, 1024 b + 1024) of the tensor flattened in C order, and the value is
fl32(scale[b] * float(q)), one fp32 rounding; all 256 codes are legal.  delta=True: the codes encode
x - g, g the server's previous global model in fp32, and the client's value is
fl32(g + fl32(scale * q)).  In a quantized upload every fp32 tensor is quantized, tensors of other
dtypes (int64 BN counters, float64) are sent plain, float16 is refused.

Block-wise absmax scaling as in Dettmers et al. (ICLR 2022); quantized client updates as in FedPAQ
(Reisizadeh et al., AISTATS 2020); the stochastic rounding is QSGD's (Alistarh et al., NeurIPS 2017).
"""
from __future__ import annotations

import numpy as np
import torch

BLOCK = 1024  # FA_Q8_BLOCK: one wave-chunk of fa_deq_fold_q8
_F32 = np.dtype(np.float32)


def n_blocks(numel: int) -> int:
    return -(-int(numel) // BLOCK)


def is_entry(v) -> bool:
    """v is (shaped like) a quantized entry: a dict with a "q8"."""
    return isinstance(v, dict) and "q8" in v


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
    if not (np.isfinite(scale).all() and (scale >= 0).all()):  # -0.0 passes: it is a zero
        raise ValueError(f"{where}: scales must be finite and >= 0")
    return np.ascontiguousarray(q8), np.ascontiguousarray(scale), bool(e["delta"])


# -- the client's side -----------------------------------------------------------------------------
def _blocks(flat: np.ndarray) -> np.ndarray:
    """flat padded with zeros to whole blocks, as [blocks, 1024]"""
    nb = n_blocks(flat.size)
    if flat.size == nb * BLOCK:
        return flat.reshape(nb, BLOCK)
    out = np.zeros(nb * BLOCK, dtype=flat.dtype)
    out[: flat.size] = flat
    return out.reshape(nb, BLOCK)


def quantize_array(x: np.ndarray, center=None, stochastic: bool = False, rng=None) -> dict:
    """One fp32 array as a quantized entry.  Per block: amax = max|x|, s = fl32(amax / 127), codes
    clip(rint(fl32(x / s)), -127, 127) (round half to even); s == 0 (an all-zero block, or amax / 127
    underflowing) gives codes 0 and scale 0.  stochastic: x / s is rounded up with probability equal
    to its fractional part (unbiased), with `rng` (a numpy.random.Generator).  center: x - center is
    quantized, in fp32, and the entry is marked delta.  Non-finite input: ValueError."""
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
    b = _blocks(flat)
    s = (np.abs(b).max(axis=1, initial=np.float32(0)) / np.float32(127)).astype(np.float32)
    live = s > 0
    r = np.zeros_like(b)
    np.divide(b, s[:, None], out=r, where=live[:, None])
    if stochastic:
        if rng is None:
            raise ValueError("stochastic rounding needs rng (a numpy.random.Generator)")
        lo = np.floor(r)
        q = lo + (rng.random(r.shape) < (r - lo))
    else:
        q = np.rint(r)
    q8 = np.clip(q, -127, 127).astype(np.int8).reshape(-1)[: flat.size].reshape(shape)
    return {"q8": q8, "scale": np.where(live, s, np.float32(0)).astype(np.float32), "block": BLOCK,
            "delta": center is not None}


def dequantize_entry(e, center=None, key=None) -> np.ndarray:
    """fl32(scale[b] * float(q)), and fl32(center + that) for a delta entry: the client's values."""
    q8, scale, delta = check_entry(key, e)
    x = (_blocks(q8.reshape(-1).astype(np.float32)) * scale[:, None]).astype(np.float32).reshape(-1)[: q8.size]
    if delta:
        if center is None:
            raise ValueError(f"key {key!r}: a delta entry needs the centre it was taken against")
        c = np.ascontiguousarray(_host_array(center, f"center[{key!r}]"), dtype=np.float32).reshape(-1)
        if c.size != x.size:
            raise ValueError(f"center[{key!r}] has {c.size} elements, the entry has {x.size}")
        x = (c + x).astype(np.float32)
    return x.reshape(q8.shape)


def quantize_state_dict(sd, center=None, stochastic: bool = False, rng=None) -> dict:
    """A state dict (numpy arrays or host torch tensors) as a quantized upload's params: every fp32
    tensor becomes a quantized entry (quantize_array), tensors of other dtypes are passed on as numpy
    arrays, float16 raises TypeError.  center: a w_glob-like dict; its values, cast to fp32, are
    subtracted before quantizing and the entries are marked delta=True."""
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
        out[k] = quantize_array(a, c, stochastic, rng)
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
    """(qkeys, delta, entries, scales) of a round of quantized uploads over the selected `keys`, or
    client-data errors.  qkeys: the selected keys that are quantized, in order; delta: the round's
    flag; entries[i][key] = (q8, scale) as checked host arrays; scales[i]: client i's scales of all
    qkeys in order, one array.  ValueError: a key quantized by some clients and plain in others, a
    plain fp32 tensor, mixed delta flags, codes of different shapes, and check_entry's; TypeError:
    float16 tensors, and check_entry's.  A well-formed numpy entry costs a few attribute reads; a
    client's scales are looked at once, together."""
    qkeys = [k for k in keys if is_entry(w_local_lst[0][k])]
    qset = set(qkeys)
    delta = None
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
            q8, sc, d = v.get("q8"), v.get("scale"), v.get("delta")
            if not (type(q8) is np.ndarray and type(sc) is np.ndarray and q8.dtype == np.int8 and sc.dtype == _F32
                    and sc.ndim == 1 and sc.shape[0] == n_blocks(q8.size) and type(v.get("block")) is int
                    and v["block"] == BLOCK and type(d) is bool and q8.flags.c_contiguous and sc.flags.c_contiguous):
                q8, sc, d = check_entry(k, v, i)  # raises what is wrong, or hands back the entry as host arrays
            if delta is None:
                delta = d
            elif d != delta:
                raise ValueError(f"client {i} key {k!r}: delta={d} in a round of delta={delta} uploads")
            if q8.shape != shapes.setdefault(k, q8.shape):
                raise ValueError(f"client {i} key {k!r}: codes of shape {q8.shape} do not match client 0's {shapes[k]}")
            mine[k] = (q8, sc)
        cat = np.concatenate([mine[k][1] for k in qkeys]) if qkeys else np.zeros(0, np.float32)
        if not (np.isfinite(cat).all() and (cat >= 0).all()):
            for k in qkeys:
                check_entry(k, w[k], i)  # names the key
        entries.append(mine)
        scales.append(cat)
    return qkeys, bool(delta), entries, scales
