"""The fast path of small host rounds (Aggregator._small_round): every bucket together under
SMALL_BYTES — LeNet-sized models, flearn's config 1.  The whole round is prebuilt once per plan as
ctypes argument records (`_SmallRecord`), so a server call is a native pack, one launch per bucket
and one synchronisation, with no per-key Python.  The switches (`small_zero_copy`, `small_parts`)
and their measurements are class attributes of Aggregator.
"""
from __future__ import annotations

import itertools
from typing import NamedTuple

import numpy as np
import torch

from . import _native as na
from .bucketplan import SMALL_BYTES, TORCH_DTYPE, BucketPlan, Shard, _as_list
from .packer import AsyncPack, NativeRows, Packer, piece_columns
from .semantics import KIND_F16, KIND_F32, KIND_F64
from .wire import wire_row

_F64 = np.dtype(np.float64)


def chain_table(pieces, host_ptr: int, row_bytes: int, bounds) -> np.ndarray:
    """AsyncPack's job table of a chained small round (_small_chain): clients
    [bounds[k], bounds[k + 1]) are part k, packed as chunk k, and client i of part k goes to row
    i + k of the staging at host_ptr — each part leaves a row free for the partial sum before it."""
    part = np.repeat(np.arange(len(bounds) - 1), np.diff(bounds))[:, None]  # per client
    client = np.arange(bounds[-1])[:, None]
    source, base, pitch, off = piece_columns(pieces, ((host_ptr, row_bytes),))
    return AsyncPack.table(src=client, dst=base + (client + part) * pitch + off, chunk=part, **source)


class _SmallChain(NamedTuple):
    """The fp32 bucket of a small zero-copy round as chained launches (_small_chain)."""
    pack: AsyncPack  # native threads pack part k's clients as its chunk k
    launches: list  # the ctypes arguments of launch k
    weights: list  # launch k's device weights, kept alive


class _SmallBucket(NamedTuple):
    """One bucket kind of a small round's record (_small_record)."""
    nat: NativeRows  # the native pack table of every client into `host`
    host: torch.Tensor  # pinned staging, [clients (+ a chain's partial-sum rows), stride]
    stack: torch.Tensor  # what the kernel reads: `host` itself (zero-copy) or a device stack
    w: torch.Tensor  # device weights, kept alive
    dout: torch.Tensor  # what the kernel writes: `hout` itself (zero-copy) or a device buffer
    hout: torch.Tensor  # the pinned result ...
    hnp: np.ndarray  # ... and its numpy view
    fn: object  # the reduce entry point
    args: tuple  # its ctypes arguments, all but the stream
    out: list  # (key, offset, size, shape) of every key of the result
    chain: _SmallChain | None


class _SmallRecord(NamedTuple):
    buckets: tuple  # one _SmallBucket per bucket kind
    pack: object  # fa_py_pack_rows
    wsig: tuple | None  # the fp32 bucket's layout as wire.wire_row compares it


def _small_record(agg, plan: BucketPlan, w_local_lst):
    """The prebuilt round of a small host-upload plan (every bucket together < SMALL_BYTES:
    LeNet-sized models, flearn's config 1), cached on the plan: per bucket kind its own
    pinned staging, device stack, device weights and result buffers, the native pack table
    and the ctypes arguments of its reduce launch, and the (key, offset, size, shape) list
    of the result.  None (cached as False) when the plan does not qualify."""
    zc = bool(agg.small_zero_copy)
    key = ("small_round", id(agg.packer), str(agg.device), agg.output, zc, int(agg.small_parts))
    rec = plan.memo.get(key)
    if rec is not None:
        return rec or None
    n = plan.n_clients
    total = sum(n * g.stride * np.dtype(g.store_dtype).itemsize for g in plan.groups.values())
    # (a float16 bucket takes the general path: its result dtype depends on the output mode)
    if plan.input_kind != "numpy" or total >= SMALL_BYTES or not plan.groups or KIND_F16 in plan.groups:
        plan.memo[key] = False
        return None
    L, dev = na.lib(), agg.device
    buckets = []
    for kind, g in plan.groups.items():
        tdt = TORCH_DTYPE[g.store_dtype]
        pieces = Packer._pieces(g, [Shard(0, dev, 0, g.stride)])
        # spare rows: the chained zero-copy round's partial sums (below)
        parts = max(1, min(int(agg.small_parts), n // 2))
        host = torch.zeros((n + parts - 1, g.stride), dtype=tdt, pin_memory=True)
        if not NativeRows.usable(pieces, [host]):
            plan.memo[key] = False
            return None
        nat = NativeRows(pieces, [host], w_local_lst, [None] * n)
        nm = g.numerics
        w = agg._weights(nm, dev)
        f64 = kind != KIND_F32 or (agg.output == "reference" and nm.out_dtype == _F64)
        odt = torch.float64 if f64 else torch.float32
        hout = torch.empty(g.stride, dtype=odt, pin_memory=True)
        if zc:  # the kernel reads the pinned staging and writes the pinned result over PCIe
            stack, dout = host, hout
        else:
            stack = torch.empty((n, g.stride), dtype=tdt, device=dev)
            dout = torch.empty(g.stride, dtype=odt, device=dev)
        chain = None
        if kind == KIND_F32:
            fn = L.fa_reduce_f32
            args = (stack.data_ptr(), g.stride, n, nm.mode, w.data_ptr(), float(nm.denom), 0, g.stride, None,
                    None if f64 else dout.data_ptr(), dout.data_ptr() if f64 else None)
            if zc and parts >= 2 and nm.mode in (na.MODE_W32_DIV64, na.MODE_W32_DIV32):
                chain = _small_chain(g, pieces, host, w, nm, dout, f64, n, parts, dev)
        else:
            fn = L.fa_reduce_f64 if kind == KIND_F64 else L.fa_reduce_i64
            args = (stack.data_ptr(), g.stride, n, w.data_ptr(), float(nm.denom), 0, g.stride, dout.data_ptr())
        out = [(s.key, s.offset, s.numel, s.shape) for s in g.segments]
        buckets.append(_SmallBucket(nat, host, stack, w, dout, hout, hout.numpy(), fn, args, out, chain))
    wsig = plan.f32.row_layout if plan.f32 is not None else None
    rec = plan.memo[key] = _SmallRecord(tuple(buckets), na.load_pyhost().fa_py_pack_rows, wsig)
    return rec


def _small_chain(g, pieces, host, w, nm, dout, f64, n, parts, dev) -> _SmallChain:
    """The fp32 bucket of a small zero-copy round as `parts` chained launches.  Clients are cut
    into parts b_0 = 0 < b_1 < ... < b_K = n (the first smallest, so the GPU starts early);
    client i of part k sits in staging row i + k.  Launch 0 sums rows [0, b_1) in fp32 (mode
    W32_DIV32 with W = 1: the epilogue returns the sum itself) into row b_1; launch k sums
    rows [b_k + k - 1, b_{k+1} + k) — the previous partial with weight fl32(1.0), then part
    k's clients — into row b_{k+1} + k, the last one with the real denominator and output.
    fl32(1 * acc) = acc, so the chain of adds is the single launch's, bit for bit, and no
    launch writes a row it reads.  The parts are packed by native threads
    (AsyncPack chunk k = part k) and each launch waits only for its own part."""
    base, rem = divmod(n, parts)  # the remainder goes to the last parts
    bounds = [0, *itertools.accumulate(base + (k >= parts - rem) for k in range(parts))]
    row = g.stride * 4
    hp = host.data_ptr()
    ap = AsyncPack(tuple(p.segment.key for p in pieces) * n, chain_table(pieces, hp, row, bounds), parts)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    args, ws = [], []
    for k in range(parts):
        lo, hi = bounds[k], bounds[k + 1]
        if k == 0:
            first, cnt, wk = hp, hi, w[:hi]
        else:
            first, cnt = hp + (lo + k - 1) * row, hi - lo + 1
            wk = torch.cat([one, w[lo:hi]])
        ws.append(wk)
        if k < parts - 1:  # an fp32 partial into row hi + k
            args.append((first, g.stride, cnt, na.MODE_W32_DIV32, wk.data_ptr(), 1.0, 0, g.stride, None,
                         hp + (hi + k) * row, None))
        else:
            args.append((first, g.stride, cnt, nm.mode, wk.data_ptr(), float(nm.denom), 0, g.stride, None,
                         None if f64 else dout.data_ptr(), dout.data_ptr() if f64 else None))
    return _SmallChain(ap, args, ws)


def _small_round(agg, plan: BucketPlan, w_local_lst):
    """One small host round with no per-key Python: the uploads are packed natively into the
    record's pinned staging (every value checked against the plan: C-contiguous, dtype, byte
    size), each bucket is one reduce launch reading that staging and writing a pinned result
    over PCIe (zero-copy; with small_zero_copy False: one H2D, the launch and one D2H) on
    torch's current stream, one synchronisation, and the result is handed out as views of one fresh array per bucket
    (numpy scalars for 0-d keys) — what Packer.unpack returns.  Returns None (nothing queued)
    when a value does not fit the record; the caller then takes the general path."""
    rec = _small_record(agg, plan, w_local_lst)
    if rec is None:
        return None
    buckets = rec.buckets
    lst = _as_list(w_local_lst)
    # decoded by the wire codec into pinned rows of this layout: the general path DMAs them as is
    if rec.wsig is not None and wire_row(lst[0], rec.wsig) is not None:
        return None
    n = len(lst)
    for b in buckets:  # every bucket packed here, except a chained one (native threads)
        if b.chain is None and rec.pack(lst, b.nat.keys, len(b.nat.keys), b.nat.ptr, 0, n) != 0:
            return None
    handles = {}
    try:
        for i, b in enumerate(buckets):
            if b.chain is not None:
                h = b.chain.pack.start(lst)
                if h is None:  # a value off the plan: nothing was copied, nothing launched
                    return None
                handles[i] = h
        dev = agg.device
        if dev.index is not None and dev.index != torch.cuda.current_device():
            with torch.cuda.device(dev):  # launches go to dev's stream from dev's context
                parts = _small_launch(buckets, handles, dev)
        else:
            parts = _small_launch(buckets, handles, dev)
    finally:
        for i, h in handles.items():  # every copy done (and the values released)
            buckets[i].chain.pack.end(h)
    return {k: parts[k] for k in plan.keys}


def _small_launch(buckets, handles, dev):
    """The queued part of _small_round: launches (and copies) on dev's current stream — a
    chained bucket's launches each right after its part's copies are in — one
    synchronisation, the results as {key: value}."""
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    try:
        _small_enqueue(buckets, handles, stream, sh)
    finally:
        stream.synchronize()  # also: the staging may be rewritten by the next call
    parts = {}
    for b in buckets:
        fresh = b.hnp.copy()
        for k, off, m, shape in b.out:
            a = fresh[off : off + m].reshape(shape)
            parts[k] = a.dtype.type(a[()]) if shape == () else a
    return parts


def _small_enqueue(buckets, handles, stream, sh):
    for i, b in enumerate(buckets):
        fn = b.fn
        if b.chain is not None:  # chained zero-copy launches, each after its part is packed
            for k, a in enumerate(b.chain.launches):
                b.chain.pack.wait(handles[i], k)
                na.check(fn(*a, sh), fn.__name__)
        elif b.stack is b.host:  # zero-copy record
            na.check(fn(*b.args, sh), fn.__name__)
        else:
            b.stack.copy_(b.host[: b.stack.shape[0]], non_blocking=True)
            na.check(fn(*b.args, sh), fn.__name__)
            b.hout.copy_(b.dout, non_blocking=True)
