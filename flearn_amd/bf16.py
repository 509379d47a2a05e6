"""bfloat16 uploads: the wire entry, its checks, and the client's encoder and
decoder.  Host-side numpy and torch only, no device code.

numpy has no bfloat16, so on the wire a bfloat16 tensor of shape S is a plain dict

    {"bf16": uint16 ndarray of shape S, "shape": tuple S}

whose uint16 values are the tensors' bit patterns: the high halves of the fp32 of the same values, so
that widening, (u16 << 16) viewed as float32, is exact.  In a bfloat16 upload every floating tensor
of 4 bytes or fewer is bfloat16 (an entry, or a torch.bfloat16 tensor on the host or on the device);
tensors of other dtypes (int64 BN counters, float64) are sent plain.

Rounding fp32 to bfloat16 is to nearest, ties to even (what torch's .to(torch.bfloat16) does), or
stochastic: up with probability equal to the dropped fraction, which is unbiased (Gupta et al.,
ICML 2015).
"""
from __future__ import annotations

import numpy as np
import torch

MARK = "bf16"
_U16 = np.dtype(np.uint16)


def is_entry(v) -> bool:
    """v is (shaped like) a bfloat16 wire entry: a dict with a "bf16"."""
    return isinstance(v, dict) and MARK in v


def is_bf16(v) -> bool:
    """v is a bfloat16 upload value: a wire entry or a torch.bfloat16 tensor."""
    return is_entry(v) or (isinstance(v, torch.Tensor) and v.dtype == torch.bfloat16)


def is_bf16_upload(params) -> bool:
    """The upload's params carry at least one bfloat16 value."""
    return hasattr(params, "values") and any(is_bf16(v) for v in params.values())


def round_f32(x: np.ndarray, stochastic: bool = False, rng=None) -> np.ndarray:
    """The bfloat16 bit patterns (uint16, x's shape) of an fp32 array.  Nearest, ties to even: add
    0x7FFF and the kept half's last bit, drop the low half (a carry out of the mantissa moves to the
    next binade, past the largest finite value to inf).  stochastic: add a uniform 16-bit integer from
    `rng` (a numpy.random.Generator) instead — up with probability low half / 2^16 — which leaves inf and
    every representable value where it is.  NaN stays NaN: its high half with the quiet bit set."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    if stochastic:
        if rng is None:
            raise ValueError("stochastic rounding needs rng (a numpy.random.Generator)")
        bump = rng.integers(0, 1 << 16, size=u.shape, dtype=np.uint64)
    else:
        bump = np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))
    out = ((u + bump) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x)
    if nan.any():
        out[nan] = ((u[nan] >> np.uint64(16)) | np.uint64(0x0040)).astype(np.uint16)
    return out


def widen(u16: np.ndarray) -> np.ndarray:
    """The fp32 values of bfloat16 bit patterns: exact."""
    return (np.asarray(u16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def encode_tensor(v, stochastic: bool = False, rng=None) -> dict:
    """One floating tensor (host numpy array or CPU torch tensor) as a wire entry: torch.bfloat16
    losslessly by an int16 view, float16 and fp32 through fp32 and round_f32."""
    if isinstance(v, torch.Tensor):
        if v.device.type != "cpu":
            raise TypeError("device-resident tensors are not encoded (upload them as they are)")
        v = v.detach()
        if v.dtype == torch.bfloat16:
            return {MARK: v.contiguous().view(torch.int16).numpy().view(np.uint16).copy(), "shape": tuple(v.shape)}
        v = v.to(torch.float32).numpy()
    a = np.asarray(v)
    return {MARK: round_f32(a.astype(np.float32, copy=False), stochastic, rng).reshape(a.shape), "shape": tuple(a.shape)}


def encode_state_dict(sd, stochastic: bool = False, rng=None) -> dict:
    """A state dict (numpy arrays or host torch tensors) as a bfloat16 upload's params: float16, fp32
    and torch.bfloat16 tensors become wire entries, everything else (int64, float64) is passed on as a
    numpy array."""
    if stochastic and rng is None:
        raise ValueError("stochastic rounding needs rng (a numpy.random.Generator)")
    out = {}
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            narrow = v.is_floating_point() and v.element_size() <= 4
        else:
            v = np.asarray(v)
            narrow = v.dtype.kind == "f" and v.dtype.itemsize <= 4
        if narrow:
            out[k] = encode_tensor(v, stochastic, rng)
        else:
            out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v
    return out


def check_entry(key, e, client=None) -> np.ndarray:
    """The C-contiguous uint16 array of one wire entry; client-data errors otherwise: ValueError for a
    missing or malformed shape and an element count that does not match it, TypeError for a "bf16"
    that is no uint16 host array."""
    where = f"key {key!r}" if client is None else f"client {client} key {key!r}"
    shape = e.get("shape")
    if not isinstance(shape, (tuple, list)) or not all(
            isinstance(d, (int, np.integer)) and not isinstance(d, bool) and d >= 0 for d in shape):
        raise ValueError(f"{where}: shape must be a tuple of non-negative ints, got {shape!r}")
    u = e[MARK]
    if isinstance(u, torch.Tensor):
        raise TypeError(f"{where}: bf16 must be a uint16 ndarray (send a torch.bfloat16 tensor as it is), got a Tensor")
    if not isinstance(u, np.ndarray) or u.dtype != _U16:
        raise TypeError(f"{where}: bf16 must be a uint16 ndarray, got {getattr(u, 'dtype', type(u).__name__)}")
    if u.size != int(np.prod(shape, dtype=np.int64)):
        raise ValueError(f"{where}: shape {tuple(shape)} does not hold {u.size} elements")
    return np.ascontiguousarray(u)


def entry_shape(v) -> tuple:
    """The shape of the tensor a bfloat16 upload value stands for."""
    return tuple(v["shape"]) if is_entry(v) else tuple(v.shape)


def decode(e, key=None) -> np.ndarray:
    """A wire entry (or a torch.bfloat16 tensor) widened to an fp32 array of its shape."""
    if isinstance(e, torch.Tensor):
        return e.detach().cpu().to(torch.float32).numpy()
    return widen(check_entry(key, e)).reshape(tuple(e["shape"]))


def decode_state_dict(params) -> dict:
    """encode_state_dict's inverse up to the rounding: fp32 arrays for the bfloat16 values."""
    return {k: decode(v, k) if is_bf16(v) else v for k, v in params.items()}


def _dtype_name(v) -> str:
    return str(getattr(v, "dtype", "")).replace("torch.", "")


def check_round(w_local_lst, keys):
    """(bkeys, rows) of a round of bfloat16 uploads over the selected `keys`, or client-data errors.
    bkeys: the selected keys that are bfloat16 for client 0, in order; rows[i][key]: client i's value
    as a flat C-contiguous uint16 host array, or the torch.bfloat16 tensor itself (host or device).
    ValueError: a key that is bfloat16 for some clients only, shapes that differ between clients, a
    plain fp32 floating tensor beside bfloat16 keys, and check_entry's; TypeError: a float16 tensor
    beside bfloat16 keys, and check_entry's."""
    bkeys = [k for k in keys if is_bf16(w_local_lst[0][k])]
    bset = set(bkeys)
    rows, shapes = [], {}
    for i, w in enumerate(w_local_lst):
        mine = {}
        for k in keys:
            v = w[k]
            if is_bf16(v) != (k in bset):
                raise ValueError(f"client {i} key {k!r}: bfloat16 in some uploads and not in others")
            if k not in bset:
                if bset and _dtype_name(v) == "float16":
                    raise TypeError(f"client {i} key {k!r}: float16 tensors in a bfloat16 upload are not supported")
                if bset and _dtype_name(v) == "float32":
                    raise ValueError(f"client {i} key {k!r}: a plain fp32 tensor in a bfloat16 upload "
                                     "(every fp32 tensor is sent as bfloat16)")
                continue
            mine[k] = check_entry(k, v, i).reshape(-1) if is_entry(v) else v
            shape = entry_shape(v)
            if shape != shapes.setdefault(k, shape):
                raise ValueError(f"client {i} key {k!r}: shape {shape} does not match client 0's {shapes[k]}")
        rows.append(mine)
    return bkeys, rows
