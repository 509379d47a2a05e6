"""Top-k sparse uploads: the format, the client's sparsifier and the server's
checks.  sparseround.py sums a round of them; strategy/sparse.py is TopKAVG.

A sparse entry stands for one fp32 tensor of an upload:

    {"idx": uint32[k], "val": float32[k], "shape": tuple, "delta": bool}

idx holds flat indices into the tensor, strictly ascending, every one < numel; 0 <= k <= numel; val the
values there, every other element being 0.  delta=True: the values are an update, to be added to the
centre (the last global model, cast to fp32) the client took them against.  Tensors of other dtypes
(int64 BN counters, float64) are sent plain.  The client keeps the k entries of largest magnitude
(Aji & Heafield 2017; Lin et al. 2018) and, with error feedback, the rest as a residual it adds to
its next upload (Stich et al. 2018).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import bf16, quant
from .quant import _host_array

_F32 = np.dtype(np.float32)
_U32 = np.dtype(np.uint32)


def is_entry(v) -> bool:
    """v is (shaped like) a sparse entry: a dict with an "idx" and a "val"."""
    return isinstance(v, dict) and "idx" in v and "val" in v


def is_sparse(params) -> bool:
    """The upload's params carry at least one sparse entry."""
    return hasattr(params, "values") and any(is_entry(v) for v in params.values())


def entry_shape(e) -> tuple:
    """The shape of the tensor an entry stands for."""
    return tuple(e["shape"])


def top_k_count(numel: int, ratio: float = 0.01, k=None) -> int:
    """How many entries of a tensor are kept: min(numel, max(1, ceil(ratio * numel))), or `k` clamped
    to [0, numel]."""
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an int >= 0 or None, got {k!r}")
        return min(int(numel), int(k))
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.floating)) or not 0 < ratio <= 1:
        raise ValueError(f"ratio must be in (0, 1], got {ratio!r}")
    return min(int(numel), max(1, math.ceil(float(ratio) * int(numel))))


def sparsify_array(x: np.ndarray, center=None, ratio: float = 0.01, k=None) -> dict:
    """The sparse entry of an fp32 array: u = x - center (fp32) or x itself, the top_k_count entries of
    largest |u|, ties going to the lower index.  Non-finite input is refused (ValueError)."""
    shape = tuple(int(d) for d in x.shape)
    u = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if center is not None:
        c = np.asarray(center, dtype=np.float32).reshape(-1)
        if c.size != u.size:
            raise ValueError(f"center has {c.size} elements, the tensor has {u.size}")
        u = u - c
    if not np.isfinite(u).all():
        raise ValueError("non-finite values are not sparsified (inf or NaN in the tensor or its update)")
    kk = top_k_count(u.size, ratio, k)
    if kk >= u.size:
        idx = np.arange(u.size, dtype=np.uint32)
    elif kk == 0:
        idx = np.zeros(0, dtype=np.uint32)
    else:
        mag = np.abs(u)
        t = np.partition(mag, u.size - kk)[u.size - kk]  # the k-th largest magnitude
        above = np.flatnonzero(mag > t)
        ties = np.flatnonzero(mag == t)[: kk - above.size]  # ascending: the lower indices win
        idx = np.sort(np.concatenate([above, ties])).astype(np.uint32)
    return {"idx": idx, "val": u[idx.astype(np.int64)].copy(), "shape": shape, "delta": center is not None}


def sparsify_state_dict(sd, center=None, ratio: float = 0.01, k=None) -> dict:
    """A state dict (numpy arrays or host torch tensors) as a sparse upload's params: every fp32 tensor
    becomes a sparse entry (sparsify_array), tensors of other dtypes are passed on as numpy arrays,
    float16 raises TypeError.  center: a w_glob-like dict; its values, cast to fp32, are subtracted
    first and the entries are marked delta=True."""
    out = {}
    for key, v in sd.items():
        a = _host_array(v, f"key {key!r}")
        if a.dtype == np.float16:
            raise TypeError(f"key {key!r}: float16 tensors are not sparsified (sparsify the fp32 model)")
        if a.dtype != _F32:
            out[key] = a
            continue
        c = None
        if center is not None:
            if key not in center:
                raise ValueError(f"center has no key {key!r}")
            c = np.asarray(_host_array(center[key], f"center[{key!r}]"), dtype=np.float32)
        try:
            out[key] = sparsify_array(a, c, ratio, k)
        except ValueError as e:
            raise ValueError(f"key {key!r}: {e}") from None
    return out


def densify_entry(e, center=None, key=None) -> np.ndarray:
    """The fp32 tensor an entry stands for: zeros with val at idx; a delta entry is added to `center`
    (its fp32 cast), one fp32 add per element."""
    shape = entry_shape(e)
    x = np.zeros(math.prod(shape), dtype=np.float32)
    x[np.asarray(e["idx"]).astype(np.int64)] = np.asarray(e["val"], dtype=np.float32)
    if e.get("delta"):
        if center is None:
            raise ValueError(f"key {key!r}: a delta entry needs the centre it was taken against")
        c = np.asarray(_host_array(center, f"center[{key!r}]"), dtype=np.float32).reshape(-1)
        if c.size != x.size:
            raise ValueError(f"center[{key!r}] has {c.size} elements, the entry has {x.size}")
        x = (c + x).astype(np.float32)
    return x.reshape(shape)


def densify_state_dict(ssd, center=None) -> dict:
    """sparsify_state_dict's inverse up to the dropped entries."""
    return {key: densify_entry(v, center[key] if v.get("delta") and center is not None and key in center else None, key)
            if is_entry(v) else v for key, v in ssd.items()}


def check_entry(key, e, client=None):
    """(idx, val, delta, shape) of one sparse entry as C-contiguous host arrays, or client-data errors:
    TypeError for an idx that is no uint32 array or a val that is no float32 array (device-resident ones
    included); ValueError for a missing field, lengths that differ, an index >= numel and indices that are
    not strictly ascending."""
    where = f"key {key!r}" if client is None else f"client {client} key {key!r}"
    for f in ("idx", "val", "shape", "delta"):
        if f not in e:
            raise ValueError(f"{where}: a sparse entry needs {f!r}")
    idx = _host_array(e["idx"], f"{where} idx")
    val = _host_array(e["val"], f"{where} val")
    if idx.dtype != _U32:
        raise TypeError(f"{where}: idx must be uint32, got {idx.dtype}")
    if val.dtype != _F32:
        raise TypeError(f"{where}: val must be float32, got {val.dtype}")
    shape = e["shape"]
    if not isinstance(shape, (tuple, list)) or not all(isinstance(d, (int, np.integer)) and d >= 0 for d in shape):
        raise ValueError(f"{where}: shape must be a tuple of ints >= 0, got {shape!r}")
    shape = tuple(int(d) for d in shape)
    if type(e["delta"]) is not bool:
        raise ValueError(f"{where}: delta must be a bool, got {e['delta']!r}")
    if idx.ndim != 1 or val.ndim != 1 or idx.shape[0] != val.shape[0]:
        raise ValueError(f"{where}: idx and val must be 1-D of one length, got {idx.shape} and {val.shape}")
    numel = math.prod(shape)
    if idx.size:
        if int(idx[-1]) >= numel or int(idx.max()) >= numel:
            raise ValueError(f"{where}: an index is >= the tensor's {numel} elements")
        if idx.size > 1 and not (idx[1:] > idx[:-1]).all():
            raise ValueError(f"{where}: indices must be strictly ascending")
    return np.ascontiguousarray(idx), np.ascontiguousarray(val), e["delta"], shape


def check_round(w_local_lst, keys):
    """(skeys, delta, entries) of a round of sparse uploads over the selected `keys`, or client-data
    errors.  skeys: the selected keys that are sparse, in order; delta: the round's flag;
    entries[i][key] = (idx, val) as checked host arrays.  ValueError: a key sparse for some clients and
    plain for others, a plain fp32 tensor, quantized or bfloat16 entries in the round, mixed delta flags,
    shapes that differ, and check_entry's; TypeError: float16 tensors, and check_entry's."""
    skeys = [k for k in keys if is_entry(w_local_lst[0][k])]
    sset = set(skeys)
    delta = None
    shapes = {}
    entries = []
    for i, w in enumerate(w_local_lst):
        mine = {}
        for k in keys:
            v = w[k]
            if quant.is_entry(v) or bf16.is_entry(v):
                raise ValueError(f"client {i} key {k!r}: a quantized or bfloat16 entry in a round of sparse uploads "
                                 "(a round's uploads are all of one format)")
            if is_entry(v) != (k in sset):
                raise ValueError(f"client {i} key {k!r}: sparse in some uploads and plain in others")
            if k not in sset:
                name = quant._dtype_name(v)
                if name == "float16":
                    raise TypeError(f"client {i} key {k!r}: float16 tensors in a sparse upload are not supported")
                if name == "float32":
                    raise ValueError(f"client {i} key {k!r}: a plain fp32 tensor in a sparse upload "
                                     "(every fp32 tensor is sparsified)")
                continue
            idx, val, d, shape = check_entry(k, v, i)
            if delta is None:
                delta = d
            elif d != delta:
                raise ValueError(f"client {i} key {k!r}: delta={d} in a round of delta={delta} uploads")
            if shape != shapes.setdefault(k, shape):
                raise ValueError(f"client {i} key {k!r}: shape {shape} does not match client 0's {shapes[k]}")
            mine[k] = (idx, val)
        entries.append(mine)
    return skeys, bool(delta), entries
