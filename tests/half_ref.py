"""numpy restatement of what the reference computes on float16 uploads (strategy.py:123-129):

    w = a0 * x0;  w += a_n * x_n;  w = np.divide(w, np.sum(agg_weight_lst))

numpy's own float16 `*`, `+` and `/` ARE the reference's arithmetic for numpy uploads, so those rows
are the literal expression; torch uploads (TensorIterator: float product stored as half, half sum)
are restated with explicit casts.  tests/test_half_host.py holds this module to the fixtures
captured from the reference (tests/golden/half_*.npz) bit for bit; the GPU tests compare the
kernels with it.
"""
from __future__ import annotations

import numpy as np

from flearn_amd import _native as na

F16, F32, F64 = np.float16, np.float32, np.float64


def reduce_rows(mode: int, x: np.ndarray, weights: np.ndarray, denom: float) -> np.ndarray:
    """The result array in the dtype it is born in (float64 / float32 / float16) for an [N, P] float16
    stack, weights as semantics.resolve_half casts them and denom = float(np.sum(agg_weight_lst))."""
    assert x.dtype == F16 and x.ndim == 2
    with np.errstate(all="ignore"):
        if mode in (na.MODE_H16_NUMPY, na.MODE_H16_NP16):
            w = weights.astype(F16)
            acc = w[0] * x[0]
            for i in range(1, len(x)):
                acc = acc + w[i] * x[i]
            assert acc.dtype == F16
            return acc / F16(denom) if mode == na.MODE_H16_NP16 else acc / F64(denom)
        if mode == na.MODE_H16_TORCH:
            w = weights.astype(F32)
            acc = (w[0] * x[0].astype(F32)).astype(F16)
            for i in range(1, len(x)):
                acc = acc + (w[i] * x[i].astype(F32)).astype(F16)
            return acc / F64(denom)
        if mode == na.MODE_H16_W32:
            w = weights.astype(F32)
            acc = w[0] * x[0]
            for i in range(1, len(x)):
                acc = acc + w[i] * x[i]
            assert acc.dtype == F32
            return acc / F32(denom)
        if mode == na.MODE_H16_W64:
            w = weights.astype(F64)
            acc = w[0] * x[0]
            for i in range(1, len(x)):
                acc = acc + w[i] * x[i]
            assert acc.dtype == F64
            return acc / F64(denom)
    raise ValueError(mode)


def outputs(q: np.ndarray):
    """(out64, out32, out16) of fa_reduce_f16 for the result q: widenings are exact, and a float64
    result reaches float16 through float32 (what load_state_dict into a half module does)."""
    with np.errstate(all="ignore"):
        o32 = q.astype(F32)
        return q.astype(F64), o32, (q if q.dtype == F16 else o32.astype(F16))


def loaded_half(q: np.ndarray) -> np.ndarray:
    """What a half module holds after load_state_dict of q: fl16(fl32(q))."""
    return outputs(np.asarray(q))[2]


def server_ensemble(agg_weight_lst, w_local_lst, key_lst=None, torch_inputs=False):
    """strategy.py:102-130 on numpy arrays, literally (numpy uploads); for torch uploads the float16
    keys go through the MODE_H16_TORCH restatement (other keys: the literal expression)."""
    if key_lst is None:
        key_lst = set(w_local_lst[0])
        for w in w_local_lst[1:]:
            key_lst &= set(w)
    molecular = np.sum(agg_weight_lst)
    out = {}
    with np.errstate(all="ignore"):
        for k in key_lst:
            xs = [np.asarray(w[k]) for w in w_local_lst]
            if torch_inputs and xs[0].dtype == F16:
                stack = np.stack([x.reshape(-1) for x in xs])
                q = reduce_rows(na.MODE_H16_TORCH, stack, np.array([F32(a) for a in agg_weight_lst]), float(molecular))
                out[k] = q.reshape(xs[0].shape)
                continue
            acc = agg_weight_lst[0] * xs[0]
            for a, x in zip(agg_weight_lst[1:], xs[1:]):
                acc = acc + a * x
            out[k] = np.divide(acc, molecular)
    return out


def same_bits(got, want) -> bool:
    """Finite values and infinities bit for bit (the sign of zero included), NaNs by position."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(got.view(u)[~gn], want.view(u)[~wn])
