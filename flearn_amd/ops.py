"""Device entry points on torch CUDA tensors: what bench.py, the multi-GPU path, the tools and the
engine (aggregator.py, streaming.py, serverstate.py) call.

`reduce_stack*` sum, divide and update a client stack in one launch; `fold_stack` adds a chunk of
clients to a typed accumulator and `fold_finish` divides and updates a finished one; `trim_sum_stack`
makes the accumulator of a robust round (per column, the sorted clients' middle values), `gram_stack`
the clients' Gram matrix, `rownorm2_stack` their squared update norms and `clip_sum_stack` the
accumulator of a norm-clipped round, to which `gauss_add` adds a DP-FedAvg round's noise;
`deq_fold_stack` adds a chunk of int8 block-quantized client rows to an fp32 accumulator.  `StackSum`
and `FoldedSum` carry what differs between those two ways to a round's weighted sum behind one
`mean(...)` with reduce_stack's keyword names, so the engine's server step is written once.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _native as na
from .rowtable import RowTable
from .semantics import KIND_F32, KIND_F64, KIND_I64

_ACC_TORCH = {na.ACC_F32: torch.float32, na.ACC_F32_W64: torch.float64, na.ACC_F64: torch.float64,
              na.ACC_I64: torch.int64}


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _check_cuda(t: torch.Tensor, name: str, dtype: torch.dtype, ndim: int | None = None):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise TypeError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {tuple(t.shape)}")


def _check_window(shape, col_begin, n_cols, n_clients):
    """(n, ncols) of the window [col_begin, +n_cols) over the first n_clients rows of a stack."""
    n = shape[0] if n_clients is None else n_clients
    if not 1 <= n <= shape[0]:
        raise ValueError("n_clients out of range")
    ncols = shape[1] - col_begin if n_cols is None else n_cols
    if col_begin < 0 or ncols < 0 or col_begin + ncols > shape[1]:
        raise ValueError("column window out of range")
    return n, ncols


def _check_stack(stack, dtype, col_begin, n_cols, n_clients):
    _check_cuda(stack, "stack", dtype, 2)
    if stack.stride(1) != 1:
        raise ValueError("stack rows must be contiguous")
    return _check_window(stack.shape, col_begin, n_cols, n_clients)


def _check_weights(weights, dtype, n):
    _check_cuda(weights, "weights", dtype)
    if weights.numel() < n:
        raise ValueError("fewer weights than clients")


def _check_arrays(ncols, *arrays, optional=True):
    """Every (name, tensor, dtype) the launch reads or writes ncols elements of: CUDA, dtype,
    contiguous, long enough.  optional: None is allowed (that output is not wanted)."""
    for name, t, dt in arrays:
        if t is None and optional:
            continue
        _check_cuda(t, name, dt)
        if t.numel() < ncols or not t.is_contiguous():
            raise ValueError(f"{name} too small or not contiguous")


def _epilogue(op: int, prev, v, beta=0.9, eta=1e-1, tau=1e-9, beta2=0.99, h=None, alpha=0.0, n_dyn=0, v_out=None):
    return na.Epilogue(op, 0, _ptr(prev), _ptr(v), beta, eta, tau, beta2, _ptr(h), alpha, float(n_dyn), _ptr(v_out))


def _byte_range(t: torch.Tensor, ncols: int):
    return t.data_ptr(), t.data_ptr() + ncols * t.element_size()


def _check_v_out(v_out, v, ncols, others=()):
    """v_out (the updated v / theta) must not share a byte with v, nor with the other operands
    the epilogue reads (prev, h): the kernel's stores would race its loads."""
    if v_out is None:
        return
    _check_arrays(ncols, ("v_out", v_out, v.dtype))
    if v_out.data_ptr() == v.data_ptr():
        raise ValueError("v_out must be None (in place) or another buffer")
    o0, o1 = _byte_range(v_out, ncols)
    for name, t in (("v", v),) + tuple(others):
        if t is None or ncols == 0:
            continue
        a0, a1 = _byte_range(t, ncols)
        if o0 < a1 and a0 < o1:
            raise ValueError(f"v_out overlaps {name}")


# ---------------------------------------------------------------------------------------------
# one launch over a client stack
# ---------------------------------------------------------------------------------------------


def reduce_stack(
    stack: torch.Tensor,
    weights: torch.Tensor,
    mode: int,
    denom: float,
    *,
    col_begin: int = 0,
    n_cols: int | None = None,
    n_clients: int | None = None,
    out32: torch.Tensor | None = None,
    out64: torch.Tensor | None = None,
    op: int = na.OP_MEAN,
    prev: torch.Tensor | None = None,
    v: torch.Tensor | None = None,
    beta: float = 0.9,
    eta: float = 1e-1,
    tau: float = 1e-9,
    beta2: float = 0.99,
    h: torch.Tensor | None = None,
    alpha: float = 0.01,
    reorder: bool = False,
    v_out: torch.Tensor | None = None,
) -> None:
    """Weighted mean of the fp32 client stack [N, stride] over columns [col_begin, +n_cols)
    (+ fused update), queued on torch's current stream.  out32/out64/prev/v/h are indexed from
    col_begin.  weights: fp32 for MODE_W32_*, f64 for MODE_W64 (device tensors).
    op=OP_DYN: FedDyn with h (fp32, in place) and v = theta; prev unused.
    v_out: where the updated v / theta goes (None: back into v).  The fast form of a fused step
    is double-buffered — out32 not prev, v_out not v, the caller swapping the pairs — because
    stores onto the lines the epilogue has just loaded cost 1-3% (DESIGN.md §4 finding 20).
    reorder=True: allow fa_reduce_f32_splitn (client splits + a fixed tree: deterministic, within
    1e-6 normwise of the reference, not bit-exact) where it is faster — narrow windows, many
    clients; stack input only."""
    L = na.lib()
    rows = isinstance(stack, RowTable)  # device uploads read in place (fa_reduce_f32_rows)
    if rows:
        if stack.elem_size != 4 or not stack.aligned:
            raise ValueError("row table is not an aligned fp32 bucket")
        if col_begin != 0 or (n_cols is not None and n_cols != stack.shape[1]):
            raise ValueError("a row table is reduced over its whole bucket")
        if n_clients is not None and n_clients != stack.shape[0]:
            raise ValueError("a row table is reduced over all of its clients")
        n, ncols = _check_window(stack.shape, col_begin, n_cols, n_clients)
    else:
        n, ncols = _check_stack(stack, torch.float32, col_begin, n_cols, n_clients)
    _check_weights(weights, torch.float64 if mode == na.MODE_W64 else torch.float32, n)
    _check_arrays(ncols, ("out32", out32, torch.float32), ("out64", out64, torch.float64))
    vdt = torch.float32 if mode == na.MODE_W32_DIV32 else torch.float64
    epi = None
    if op == na.OP_DYN:
        _check_arrays(ncols, ("h", h, torch.float32), ("theta", v, vdt), optional=False)
        _check_v_out(v_out, v, ncols, (("h", h),))
        epi = _epilogue(op, None, v, h=h, alpha=alpha, n_dyn=n, v_out=v_out)
    elif op != na.OP_MEAN:
        _check_arrays(ncols, ("prev", prev, torch.float32), ("v", v, vdt), optional=False)
        _check_v_out(v_out, v, ncols, (("prev", prev),))
        epi = _epilogue(op, prev, v, beta, eta, tau, beta2, v_out=v_out)
    if rows:
        pieces, npieces, grid = stack.piece_table(op)
        rc = L.fa_reduce_f32_rows(
            stack.ptrs.data_ptr(), n, mode, weights.data_ptr(), float(denom), pieces.data_ptr(), npieces, grid,
            stack.work.data_ptr(),
            ctypes.byref(epi) if epi is not None else None, _ptr(out32), _ptr(out64),
            na.stream_handle(stack.device),
        )
        na.check(rc, "fa_reduce_f32_rows")
        stack.release()
        return
    fn = L.fa_reduce_f32_splitn if reorder else L.fa_reduce_f32
    rc = fn(
        stack.data_ptr(), stack.stride(0), n, mode, weights.data_ptr(), float(denom), col_begin, ncols,
        ctypes.byref(epi) if epi is not None else None, _ptr(out32), _ptr(out64),
        na.stream_handle(stack.device),
    )
    na.check(rc, "fa_reduce_f32_splitn" if reorder else "fa_reduce_f32")


def _reduce_stack8(dtype, entry, stack, weights, denom, out64, n_clients, col_begin, n_cols):
    """The 8-byte kernels' shared body: entry = fa_reduce_f64 / fa_reduce_i64, stack and weights in dtype."""
    n, ncols = _check_stack(stack, dtype, col_begin, n_cols, n_clients)
    _check_weights(weights, dtype, n)
    _check_arrays(ncols, ("out64", out64, torch.float64), optional=False)
    rc = getattr(na.lib(), entry)(stack.data_ptr(), stack.stride(0), n, weights.data_ptr(), float(denom), col_begin,
                                  ncols, out64.data_ptr(), na.stream_handle(stack.device))
    na.check(rc, entry)


def reduce_stack_f64(stack, weights, denom, out64, n_clients=None, *, col_begin=0, n_cols=None):
    """Weighted mean of the float64 client stack over columns [col_begin, +n_cols) (default: all);
    out64 is indexed from col_begin."""
    _reduce_stack8(torch.float64, "fa_reduce_f64", stack, weights, denom, out64, n_clients, col_begin, n_cols)


def reduce_stack_i64(stack, weights, denom, out64, n_clients=None, *, col_begin=0, n_cols=None):
    """Wrapping int64 weighted sum of the int64 client stack over columns [col_begin, +n_cols)
    (default: all), then the float64 divide; out64 is indexed from col_begin."""
    _reduce_stack8(torch.int64, "fa_reduce_i64", stack, weights, denom, out64, n_clients, col_begin, n_cols)


def reduce_stack_f16(stack, weights, mode, denom, *, out16=None, out32=None, out64=None, col_begin=0, n_cols=None,
                     n_clients=None) -> None:
    """Weighted mean of the float16 client stack [N, stride] over columns [col_begin, +n_cols), queued on
    torch's current stream (fa_reduce_f16; mode: na.MODE_H16_*, see semantics.resolve_half).
    weights: device float32 (float64 for MODE_H16_W64) — for MODE_H16_NUMPY / _NP16 the float16
    weights widened.  out64 / out32 / out16 (float64 / float32 / float16 device tensors, any subset):
    the result in the dtype it is born in, widened exactly, or narrowed through float32 — out16 of a
    float64 result is fl16(fl32(q)), what load_state_dict into a half module stores."""
    L = na.lib()
    n, ncols = _check_stack(stack, torch.float16, col_begin, n_cols, n_clients)
    _check_weights(weights, torch.float64 if mode == na.MODE_H16_W64 else torch.float32, n)
    _check_arrays(ncols, ("out16", out16, torch.float16), ("out32", out32, torch.float32),
                  ("out64", out64, torch.float64))
    rc = L.fa_reduce_f16(stack.data_ptr(), stack.stride(0), n, mode, weights.data_ptr(), float(denom), col_begin, ncols,
                         _ptr(out16), _ptr(out32), _ptr(out64), na.stream_handle(stack.device))
    na.check(rc, "fa_reduce_f16")


# ---------------------------------------------------------------------------------------------
# a round in chunks of clients: fold, then finish
# ---------------------------------------------------------------------------------------------


def acc_kind_of(kind: str, mode: int) -> int:
    """FA_ACC_* of a bucket kind under its numerics' mode (the sum type np.result_type gives)."""
    if kind == KIND_F32:
        return na.ACC_F32_W64 if mode == na.MODE_W64 else na.ACC_F32
    return {KIND_F64: na.ACC_F64, KIND_I64: na.ACC_I64}[kind]


def fold_stack(acc_kind: int, stack: torch.Tensor, weights: torch.Tensor, acc_in, acc_out: torch.Tensor, *,
               col_begin: int = 0, n_cols: int | None = None, n_clients: int | None = None) -> None:
    """acc_out = acc_in + sum_i weights[i] * stack[i] over the chunk's rows in list order (fa_fold),
    queued on torch's current stream.  acc_in None: the chunk opens the round (its first product
    initialises the sum).  acc_out may be acc_in."""
    n = stack.shape[0] if n_clients is None else n_clients
    ncols = stack.shape[1] - col_begin if n_cols is None else n_cols
    if stack.dim() != 2 or stack.stride(1) != 1 or not stack.is_cuda:
        raise ValueError("stack must be a 2-D device tensor with contiguous rows")
    adt = _ACC_TORCH[acc_kind]
    for name, t in (("acc_in", acc_in), ("acc_out", acc_out)):
        if t is not None and (t.dtype != adt or not t.is_cuda or t.numel() < ncols or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {adt} device tensor of at least {ncols} elements")
    if weights.numel() < n or not 1 <= n <= stack.shape[0]:
        raise ValueError("fewer weights or rows than clients")
    rc = na.lib().fa_fold(acc_kind, stack.data_ptr(), stack.stride(0), n, weights.data_ptr(), _ptr(acc_in),
                          acc_out.data_ptr(), col_begin, ncols, na.stream_handle(stack.device))
    na.check(rc, "fa_fold")


def fold_finish(acc_kind: int, mode: int, acc: torch.Tensor, denom: float, n_cols: int, *, out32=None, out64=None,
                epi: na.Epilogue | None = None) -> None:
    """The divide by `denom` and the optional server update over a finished accumulator
    (fa_fold_finish), queued on torch's current stream."""
    rc = na.lib().fa_fold_finish(acc_kind, mode, acc.data_ptr(), float(denom), n_cols,
                                 ctypes.byref(epi) if epi is not None else None, _ptr(out32), _ptr(out64),
                                 na.stream_handle(acc.device))
    na.check(rc, "fa_fold_finish")


def trim_sum_stack(acc_kind: int, stack: torch.Tensor, trim: int, acc_out: torch.Tensor, *, n_clients: int | None = None,
                   col_begin: int = 0, n_cols: int | None = None) -> None:
    """acc_out[c] = the sum, in ascending IEEE totalOrder, of column col_begin + c's n_clients values
    without its `trim` smallest and `trim` largest (fa_trim_sum), queued on torch's current stream.
    acc_kind: na.ACC_F32 (fp32 stack, fp32 sums), na.ACC_F64 or na.ACC_I64; the accumulator is what
    fold_finish takes, with denom = n_clients - 2 * trim for the trimmed mean.  At most
    na.TRIM_MAX_CLIENTS clients; the result does not depend on the order of the rows."""
    if acc_kind not in (na.ACC_F32, na.ACC_F64, na.ACC_I64):
        raise ValueError("trimmed sums take ACC_F32, ACC_F64 or ACC_I64")
    if not isinstance(stack, torch.Tensor) or stack.dim() != 2 or stack.stride(1) != 1 or not stack.is_cuda:
        raise ValueError("stack must be a 2-D device tensor with contiguous rows")
    adt = _ACC_TORCH[acc_kind]
    if stack.dtype != adt:
        raise TypeError(f"stack must be {adt} for this accumulator kind, got {stack.dtype}")
    n, ncols = _check_window(stack.shape, col_begin, n_cols, n_clients)
    if n > na.TRIM_MAX_CLIENTS:
        raise ValueError(f"at most {na.TRIM_MAX_CLIENTS} clients, got {n}")
    if isinstance(trim, bool) or not isinstance(trim, (int, np.integer)) or trim < 0 or 2 * trim >= n:
        raise ValueError(f"trim must be an integer with 0 <= 2 * trim < n_clients, got {trim!r} for {n} clients")
    if (not isinstance(acc_out, torch.Tensor) or acc_out.dtype != adt or not acc_out.is_cuda or acc_out.numel() < ncols
            or not acc_out.is_contiguous() or acc_out.device != stack.device):
        raise ValueError(f"acc_out must be a contiguous {adt} tensor of at least {ncols} elements on the stack's device")
    rc = na.lib().fa_trim_sum(acc_kind, stack.data_ptr(), stack.stride(0), n, int(trim), acc_out.data_ptr(), col_begin,
                              ncols, na.stream_handle(stack.device))
    na.check(rc, "fa_trim_sum")


def gram_workspace(n_clients: int, n_cols: int) -> int:
    """Bytes of workspace gram_stack needs for this shape (fa_gram_workspace): enough on any device
    and under any set_reduce_grid."""
    need = na.load().fa_gram_workspace(int(n_clients), int(n_cols))
    if need < 0:
        na.check(int(need), "fa_gram_workspace")
    return int(need)


def gram_stack(stack: torch.Tensor, *, center: torch.Tensor | None = None, n_clients: int | None = None,
               col_begin: int = 0, n_cols: int | None = None, out: torch.Tensor | None = None,
               workspace: torch.Tensor | None = None) -> torch.Tensor:
    """The clients' Gram matrix over the window [col_begin, +n_cols) of an fp32 stack (fa_gram_f32),
    queued on torch's current stream: G[i, j] = sum_k y_i[k] * y_j[k] with y_i = fl32(x_i - center),
    a float64 [N, N] device tensor, symmetric bit for bit.  center: an fp32 device row laid out like
    a stack row (indexed by the stack's columns, at least col_begin + n_cols long), or None.  At most
    na.GRAM_MAX_CLIENTS clients.  out: a contiguous float64 tensor of at least N * N elements to
    write (else a fresh one); workspace: a 16-B aligned device buffer of at least
    gram_workspace(N, n_cols) bytes (else a fresh one)."""
    if not isinstance(stack, torch.Tensor) or stack.dim() != 2 or stack.stride(1) != 1 or not stack.is_cuda:
        raise ValueError("stack must be a 2-D device tensor with contiguous rows")
    if stack.dtype != torch.float32:
        raise TypeError(f"stack must be torch.float32, got {stack.dtype}")
    n, ncols = _check_window(stack.shape, col_begin, n_cols, n_clients)
    if n > na.GRAM_MAX_CLIENTS:
        raise ValueError(f"at most {na.GRAM_MAX_CLIENTS} clients, got {n}")
    if ncols < 1:
        raise ValueError("the column window is empty")
    if center is not None:
        if (not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or center.device != stack.device
                or center.dim() != 1 or not center.is_contiguous() or center.numel() < col_begin + ncols):
            raise ValueError(f"center must be a contiguous 1-D torch.float32 tensor of at least {col_begin + ncols} "
                             "elements on the stack's device")
    if out is None:
        out = torch.empty((n, n), dtype=torch.float64, device=stack.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != stack.device
          or not out.is_contiguous() or out.numel() < n * n):
        raise ValueError(f"out must be a contiguous torch.float64 tensor of at least {n * n} elements on the stack's device")
    need = gram_workspace(n, ncols)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=stack.device)
    elif (not isinstance(workspace, torch.Tensor) or workspace.device != stack.device or not workspace.is_contiguous()
          or workspace.numel() * workspace.element_size() < need):
        raise ValueError(f"workspace must be a contiguous tensor of at least {need} bytes on the stack's device")
    rc = na.lib().fa_gram_f32(stack.data_ptr(), stack.stride(0), n, _ptr(center), col_begin, ncols, workspace.data_ptr(),
                              workspace.numel() * workspace.element_size(), out.data_ptr(),
                              na.stream_handle(stack.device))
    na.check(rc, "fa_gram_f32")
    return out.reshape(-1)[: n * n].view(n, n)


def rownorm_workspace(n_clients: int, n_cols: int) -> int:
    """Bytes of workspace rownorm2_stack needs for this shape (fa_rownorm_workspace): enough on any
    device and under any set_reduce_grid."""
    need = na.load().fa_rownorm_workspace(int(n_clients), int(n_cols))
    if need < 0:
        na.check(int(need), "fa_rownorm_workspace")
    return int(need)


def _check_f32_stack(stack, col_begin, n_cols, n_clients, max_clients):
    if not isinstance(stack, torch.Tensor) or stack.dim() != 2 or stack.stride(1) != 1 or not stack.is_cuda:
        raise ValueError("stack must be a 2-D device tensor with contiguous rows")
    if stack.dtype != torch.float32:
        raise TypeError(f"stack must be torch.float32, got {stack.dtype}")
    n, ncols = _check_window(stack.shape, col_begin, n_cols, n_clients)
    if n > max_clients:
        raise ValueError(f"at most {max_clients} clients, got {n}")
    return n, ncols


def _check_center_row(center, stack, need):
    if (not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or center.device != stack.device
            or center.dim() != 1 or not center.is_contiguous() or center.numel() < need):
        raise ValueError(f"center must be a contiguous 1-D torch.float32 tensor of at least {need} "
                         "elements on the stack's device")


def rownorm2_stack(stack: torch.Tensor, *, center: torch.Tensor | None = None, n_clients: int | None = None,
                   col_begin: int = 0, n_cols: int | None = None, out: torch.Tensor | None = None,
                   workspace: torch.Tensor | None = None) -> torch.Tensor:
    """The clients' squared update norms over the window [col_begin, +n_cols) of an fp32 stack
    (fa_rownorm2_f32), queued on torch's current stream: out[i] = sum_k fl32(x_i[k] - center[k])^2, a
    float64 [N] device tensor, summed in a fixed order (the same bits for the same inputs, device and
    grid).  center: an fp32 device row laid out like a stack row (at least col_begin + n_cols long),
    or None.  At most na.CLIP_MAX_CLIENTS clients.  out: a contiguous float64 tensor of at least N
    elements to write (else a fresh one); workspace: a 16-B aligned device buffer of at least
    rownorm_workspace(N, n_cols) bytes (else a fresh one)."""
    n, ncols = _check_f32_stack(stack, col_begin, n_cols, n_clients, na.CLIP_MAX_CLIENTS)
    if ncols < 1:
        raise ValueError("the column window is empty")
    if center is not None:
        _check_center_row(center, stack, col_begin + ncols)
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=stack.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != stack.device
          or not out.is_contiguous() or out.numel() < n):
        raise ValueError(f"out must be a contiguous torch.float64 tensor of at least {n} elements on the stack's device")
    need = rownorm_workspace(n, ncols)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=stack.device)
    elif (not isinstance(workspace, torch.Tensor) or workspace.device != stack.device or not workspace.is_contiguous()
          or workspace.numel() * workspace.element_size() < need):
        raise ValueError(f"workspace must be a contiguous tensor of at least {need} bytes on the stack's device")
    rc = na.lib().fa_rownorm2_f32(stack.data_ptr(), stack.stride(0), n, _ptr(center), col_begin, ncols,
                                  workspace.data_ptr(), workspace.numel() * workspace.element_size(), out.data_ptr(),
                                  na.stream_handle(stack.device))
    na.check(rc, "fa_rownorm2_f32")
    return out.reshape(-1)[:n]


def clip_sum_stack(stack: torch.Tensor, center: torch.Tensor, scale: torch.Tensor, acc_out: torch.Tensor, *,
                   n_clients: int | None = None, col_begin: int = 0, n_cols: int | None = None) -> None:
    """acc_out[c] = the running fp32 sum, in list order, of the clients' clipped uploads of column
    col_begin + c (fa_clip_sum_f32), queued on torch's current stream: row i as it is for
    scale[i] >= 1, fl32(g + fl32(scale[i] * fl32(x - g))) for 0 < scale[i] < 1, and the centre g, the
    row unread, otherwise.  center: an fp32 device row laid out like a stack row; scale: fp32 [N] on
    the device.  The accumulator is na.ACC_F32's: fold_finish divides it.  At most
    na.CLIP_MAX_CLIENTS clients."""
    n, ncols = _check_f32_stack(stack, col_begin, n_cols, n_clients, na.CLIP_MAX_CLIENTS)
    _check_center_row(center, stack, col_begin + ncols)
    if (not isinstance(scale, torch.Tensor) or scale.dtype != torch.float32 or scale.device != stack.device
            or not scale.is_contiguous() or scale.numel() < n):
        raise ValueError(f"scale must be a contiguous torch.float32 tensor of at least {n} elements on the stack's device")
    if (not isinstance(acc_out, torch.Tensor) or acc_out.dtype != torch.float32 or not acc_out.is_cuda
            or acc_out.numel() < ncols or not acc_out.is_contiguous() or acc_out.device != stack.device):
        raise ValueError(f"acc_out must be a contiguous torch.float32 tensor of at least {ncols} elements on the "
                         "stack's device")
    rc = na.lib().fa_clip_sum_f32(stack.data_ptr(), stack.stride(0), n, center.data_ptr(), scale.data_ptr(),
                                  acc_out.data_ptr(), col_begin, ncols, na.stream_handle(stack.device))
    na.check(rc, "fa_clip_sum_f32")


def clip_fold_stack(stack: torch.Tensor, center: torch.Tensor, scale: torch.Tensor, acc_in, acc_out: torch.Tensor, *,
                    n_clients: int | None = None, col_begin: int = 0, n_cols: int | None = None) -> None:
    """One chunk of a streamed clipped round (fa_clip_fold_f32), queued on torch's current stream:
    acc_out[c] = acc_in[c] + the chunk's clipped uploads of column col_begin + c, added in list order
    under clip_sum_stack's three-way rule.  acc_in None: the chunk opens the round and the call is
    clip_sum_stack's (the first clipped upload initialises the sum).  Chunks chained through the
    accumulator leave the bits of one clip_sum_stack over all their rows.  acc_out may be acc_in.
    At most na.CLIP_MAX_CLIENTS clients per chunk."""
    n, ncols = _check_f32_stack(stack, col_begin, n_cols, n_clients, na.CLIP_MAX_CLIENTS)
    _check_center_row(center, stack, col_begin + ncols)
    if (not isinstance(scale, torch.Tensor) or scale.dtype != torch.float32 or scale.device != stack.device
            or not scale.is_contiguous() or scale.numel() < n):
        raise ValueError(f"scale must be a contiguous torch.float32 tensor of at least {n} elements on the stack's device")
    for name, t in (("acc_in", acc_in), ("acc_out", acc_out)):
        if name == "acc_in" and t is None:
            continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.numel() < ncols
                or not t.is_contiguous() or t.device != stack.device):
            raise ValueError(f"{name} must be a contiguous torch.float32 tensor of at least {ncols} elements on the "
                             "stack's device")
    rc = na.lib().fa_clip_fold_f32(stack.data_ptr(), stack.stride(0), n, center.data_ptr(), scale.data_ptr(),
                                   _ptr(acc_in), acc_out.data_ptr(), col_begin, ncols, na.stream_handle(stack.device))
    na.check(rc, "fa_clip_fold_f32")


def deq_fold_stack(stack_i8: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor, acc_in, acc_out: torch.Tensor, *,
                   center: torch.Tensor | None = None, col_begin: int = 0, n_cols: int | None = None,
                   n_clients: int | None = None) -> None:
    """One chunk of int8 block-quantized client rows added to an fp32 accumulator (fa_deq_fold_q8;
    DESIGN.md section 17, restated by tests/quant_ref.py), queued on torch's current stream.  Per
    column c of the window and row i in list order, every operation rounded to fp32:
    x = scales[i, (col_begin + c) // 1024] * float(stack_i8[i, col_begin + c]); with `center` (an fp32
    device row laid out like a stack row: delta uploads) x = center[col_begin + c] + x;
    acc_out[c] = acc + weights[i] * x, acc starting from acc_in[c] — or, acc_in None, from row 0's
    product: the chunk opens the round.  The bits are fold_stack's (na.ACC_F32) on the dequantized
    rows, and fold_finish divides the accumulator.  stack_i8: int8 [N, stride], stride a multiple of
    16; scales: fp32 [N, >= ceil((col_begin + n_cols) / 1024)]; weights: fp32 [>= N]; col_begin a
    multiple of 1024.  acc_out may be acc_in.  No client cap."""
    if (not isinstance(stack_i8, torch.Tensor) or stack_i8.dim() != 2 or stack_i8.stride(1) != 1
            or not stack_i8.is_cuda):
        raise ValueError("stack_i8 must be a 2-D device tensor with contiguous rows")
    if stack_i8.dtype != torch.int8:
        raise TypeError(f"stack_i8 must be torch.int8, got {stack_i8.dtype}")
    n, ncols = _check_window(stack_i8.shape, col_begin, n_cols, n_clients)
    dev = stack_i8.device
    blocks = -(-(col_begin + ncols) // na.Q8_BLOCK)
    if (not isinstance(scales, torch.Tensor) or scales.dtype != torch.float32 or scales.device != dev
            or scales.dim() != 2 or scales.stride(1) != 1 or scales.shape[0] < n or scales.shape[1] < blocks):
        raise ValueError(f"scales must be a torch.float32 [>= {n}, >= {blocks}] tensor with contiguous rows on the "
                         "stack's device")
    if (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.device != dev
            or not weights.is_contiguous() or weights.numel() < n):
        raise ValueError(f"weights must be a contiguous torch.float32 tensor of at least {n} elements on the stack's device")
    if center is not None:
        _check_center_row(center, stack_i8, col_begin + ncols)
    for name, t in (("acc_in", acc_in), ("acc_out", acc_out)):
        if name == "acc_in" and t is None:
            continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.numel() < ncols
                or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous torch.float32 tensor of at least {ncols} elements on the "
                             "stack's device")
    rc = na.lib().fa_deq_fold_q8(stack_i8.data_ptr(), stack_i8.stride(0), n, scales.data_ptr(), scales.stride(0),
                                 weights.data_ptr(), _ptr(center), _ptr(acc_in), acc_out.data_ptr(), col_begin, ncols,
                                 na.stream_handle(dev))
    na.check(rc, "fa_deq_fold_q8")


def gauss_add(acc: torch.Tensor, sigma: float, seed: int, sequence: int, *, col_begin: int = 0,
              n_cols: int | None = None) -> None:
    """acc[c] = fl32(acc[c] + fl32(sigma * z)) for c < n_cols (default: all of acc), z the standard
    normal of the absolute column col_begin + c under (seed, sequence) (fa_gauss_add_f32; DESIGN.md
    section 15, restated by tests/noise_ref.py), queued on torch's current stream.  acc: a contiguous
    1-D fp32 device tensor, the window itself; col_begin (a multiple of 4, any size up to 2^63) only
    enters the generator's counter.  seed and sequence are integers in [0, 2^64); the caller advances
    sequence once per noised round, and the same (seed, sequence) repeats the noise.  sigma = 0 or an
    empty window launches nothing."""
    if (not isinstance(acc, torch.Tensor) or acc.dtype != torch.float32 or not acc.is_cuda or acc.dim() != 1
            or not acc.is_contiguous()):
        raise ValueError("acc must be a contiguous 1-D torch.float32 device tensor")
    ncols = acc.numel() if n_cols is None else n_cols
    for name, v in (("col_begin", col_begin), ("n_cols", ncols)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
    if ncols > acc.numel() or col_begin + ncols >= 2 ** 63:
        raise ValueError("column window out of range")
    for name, v in (("seed", seed), ("sequence", sequence)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 64:
            raise ValueError(f"{name} must be an integer in [0, 2^64), got {v!r}")
    with np.errstate(over="ignore"):
        s32 = np.float32(sigma)
    if not np.isfinite(s32) or s32 < 0:  # an fp32 argument: a finite double past fp32's range is refused too
        raise ValueError(f"sigma must be finite in fp32 and >= 0, got {sigma!r}")
    rc = na.lib().fa_gauss_add_f32(acc.data_ptr(), int(col_begin), int(ncols), float(s32), int(seed), int(sequence),
                                   na.stream_handle(acc.device))
    na.check(rc, "fa_gauss_add_f32")


# ---------------------------------------------------------------------------------------------
# a round's weighted sum, either way: what the engine's server step divides and updates
# ---------------------------------------------------------------------------------------------
# mean(nm, denom, **reduce_stack's output and epilogue keywords) queues the divide by denom under
# the bucket's Numerics nm, and the update.  Both look their launch up in this module at the call,
# so a test that refuses a launch replaces reduce_stack / fold_finish / _epilogue here.


class StackSum(NamedTuple):
    """Clients still to be summed: the one-launch reduce sums, divides and updates."""
    stack: object  # torch stack or RowTable
    weights: torch.Tensor
    reorder: bool = False  # only ever True for a torch fp32 stack

    @property
    def n_clients(self) -> int:
        return self.stack.shape[0]

    def mean(self, nm, denom, *, out32=None, out64=None, **epilogue) -> None:
        if nm.kind == KIND_F32:
            reduce_stack(self.stack, self.weights, nm.mode, denom, out32=out32, out64=out64, reorder=self.reorder,
                         **epilogue)
        else:
            (reduce_stack_f64 if nm.kind == KIND_F64 else reduce_stack_i64)(self.stack, self.weights, denom, out64)


class FoldedSum(NamedTuple):
    """The sum fa_fold already made: fa_fold_finish divides and updates."""
    acc: torch.Tensor
    acc_kind: int
    n_clients: int  # the whole round's, FedDyn's N
    n_cols: int

    def mean(self, nm, denom, *, out32=None, out64=None, op=na.OP_MEAN, prev=None, v=None, v_out=None, h=None,
             alpha=0.0, beta=0.9, eta=1e-1, tau=1e-9, beta2=0.99) -> None:
        epi = None
        if op == na.OP_DYN:
            epi = _epilogue(op, None, v, h=h, alpha=alpha, n_dyn=self.n_clients, v_out=v_out)
        elif op != na.OP_MEAN:
            epi = _epilogue(op, prev, v, beta, eta, tau, beta2, v_out=v_out)
        fold_finish(self.acc_kind, nm.mode, self.acc, denom, self.n_cols, out32=out32, out64=out64, epi=epi)


# ---------------------------------------------------------------------------------------------
# standalone updates, launch settings, synthetic data, FedDistill's mean
# ---------------------------------------------------------------------------------------------


def apply_update(op: int, local32, glob, v, *, out32=None, out64=None, beta=0.9, eta=1e-1, tau=1e-9,
                 beta2=0.99) -> None:
    """Standalone AVGM/OPT update (client_receive form): w = update(glob, local32, v)."""
    L = na.lib()
    prec = na.PREC_F64 if glob.dtype == torch.float64 else na.PREC_F32
    _check_cuda(local32, "local", torch.float32)
    _check_cuda(glob, "glob", torch.float64 if prec == na.PREC_F64 else torch.float32)
    _check_cuda(v, "v", glob.dtype)
    n = local32.numel()
    if glob.numel() != n or v.numel() != n:
        raise ValueError("local / glob / v sizes differ")
    _check_arrays(n, ("v", v, glob.dtype), ("out32", out32, torch.float32), ("out64", out64, torch.float64))
    epi = _epilogue(op, local32, v, beta, eta, tau, beta2)
    rc = L.fa_opt_apply(prec, ctypes.byref(epi), local32.data_ptr(), glob.data_ptr(), n, _ptr(out32),
                        _ptr(out64), na.stream_handle(local32.device))
    na.check(rc, "fa_opt_apply")


def apply_dyn(glob, h, theta, n_clients: int, alpha: float = 0.01, *, out32=None, out64=None) -> None:
    """Standalone FedDyn step on a computed mean (dyn.py:17-36): h and theta in place,
    w -> out32/out64 (which may alias glob / theta)."""
    L = na.lib()
    prec = na.PREC_F64 if glob.dtype == torch.float64 else na.PREC_F32
    _check_cuda(glob, "glob", torch.float64 if prec == na.PREC_F64 else torch.float32)
    _check_cuda(h, "h", torch.float32)
    _check_cuda(theta, "theta", glob.dtype)
    n = glob.numel()
    if h.numel() != n or theta.numel() != n:
        raise ValueError("glob / h / theta sizes differ")
    _check_arrays(n, ("h", h, torch.float32), ("theta", theta, glob.dtype), ("out32", out32, torch.float32),
                  ("out64", out64, torch.float64))
    epi = _epilogue(na.OP_DYN, None, theta, h=h, alpha=alpha, n_dyn=n_clients)
    rc = L.fa_opt_apply(prec, ctypes.byref(epi), None, glob.data_ptr(), n, _ptr(out32), _ptr(out64),
                        na.stream_handle(glob.device))
    na.check(rc, "fa_opt_apply")


def set_reduce_grid(grid: int) -> int:
    """Blocks of the stack reduces (fp32 and float16), the folds, the trimmed sums, the Gram
    matrix, the update norms, the clipped sum and its noise, process-wide (fa_set_reduce_grid): 0 = the library's
    choice; fewer leave CUs to kernels running beside the reduce (RCCL's gather in the multi-GPU
    pipeline).  Returns the previous setting.  Results never depend on it."""
    L = na.load()
    rc = L.fa_set_reduce_grid(int(grid))
    if rc < 0:
        na.check(rc, "fa_set_reduce_grid")
    return rc


def last_launch():
    """(kernel, grid, launches) of the calling thread's last reduce call (fa_last_launch): the name
    of the kernel instantiation launched last, its blocks, and how many launches the call made.
    kernel is None when the call launched nothing."""
    rec = na.LaunchRecord()
    na.check(na.load().fa_last_launch(ctypes.byref(rec)), "fa_last_launch")
    return (rec.kernel.decode() if rec.kernel else None), rec.grid, rec.launches


def fill_uniform(dst: torch.Tensor, seed: int, row_begin: int = 0, col_begin: int = 0,
                 n_cols: int | None = None) -> None:
    """Synthetic client data on device: dst[r, c] = U(-1,1) hash of (seed, row_begin+r,
    col_begin+c) for c < n_cols (default: all columns)."""
    L = na.lib()
    _check_cuda(dst, "dst", torch.float32)
    d2 = dst if dst.dim() == 2 else dst.view(1, -1)
    ncols = d2.shape[1] if n_cols is None else n_cols
    for r0 in range(0, d2.shape[0], 65535):
        rows = min(65535, d2.shape[0] - r0)
        rc = L.fa_fill_uniform_f32(d2[r0].data_ptr(), d2.stride(0), rows, ncols, seed & (2**64 - 1),
                                   row_begin + r0, col_begin, na.stream_handle(dst.device))
        na.check(rc, "fa_fill_uniform_f32")


def mean_tables(tables, device=None):
    """FedDistill's logits mean (distill.py:42-46) on the device: user_logits = 0, += each table
    in list order, / len(tables), in the tables' dtype (fp32 or f64), bit-identical to torch /
    numpy on the host.  One reduce launch over a [N+1, C*C] stack whose row 0 is zeros with
    weight 1 (so the sum starts from +0.0 exactly as `0 + t0` does) and weights 1 elsewhere.
    Returns the container type of tables[0] (torch tensor on its device, or ndarray)."""
    if len(tables) == 0:
        raise ZeroDivisionError("division by zero")  # 0 / len([])  distill.py:46
    first = tables[0]
    as_torch = isinstance(first, torch.Tensor)
    host = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in tables]
    dt, shape = host[0].dtype, host[0].shape
    for a in host[1:]:
        if a.dtype != dt or a.shape != shape:
            raise ValueError(f"logits tables differ: {a.dtype}{a.shape} vs {dt}{shape}")
    if dt not in (np.float32, np.float64):
        raise NotImplementedError(f"logits dtype {dt}: the device mean handles float32 / float64 tables")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n, m = len(host), int(np.prod(shape, dtype=np.int64))
    stride = max(64, -(-m // 64) * 64)
    stack = np.zeros((n + 1, stride), dtype=dt)
    for i, a in enumerate(host):
        stack[i + 1, :m] = a.reshape(-1)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    with torch.cuda.device(dev):
        sd = torch.from_numpy(stack).to(dev)
        w = torch.ones(n + 1, dtype=tdt, device=dev)
        out = torch.empty(stride, dtype=tdt, device=dev)
        if tdt == torch.float32:
            reduce_stack(sd, w, na.MODE_W32_DIV32, float(n), out32=out)  # fp32 sum, fp32 / fl32(N)
        else:
            reduce_stack_f64(sd, w, float(n), out)
        res = out[:m].view(shape)
        if as_torch:
            return res.to(first.device).clone() if first.device != dev else res.clone()
        return res.cpu().numpy()
