"""The sparse round of the engine, bound on Aggregator as `ensemble_sparse`:
uploads whose fp32 tensors are top-k sparse entries (sparse.py) are summed by ops.sparse_fold_stack
from a device stack of (column, value) pairs — eight bytes per kept entry on PCIe and in HBM, the
rows never densified — into the fp32 accumulator every folded round ends in, and the round ends in
the server step every round ends in (Aggregator._server_step).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _native as na
from . import ops, sparse
from .bucketplan import Group, make_plan, select_keys
from .semantics import KIND_F16, KIND_F32
from .serverstate import DynState, ServerOptimizer


def _refuse(agg, server_opt) -> None:
    """What the sparse round does not do, refused before the uploads are looked at."""
    if agg._dist:
        raise ValueError("a sparse round is not sharded over a process group (group=)")
    if len(agg.devices) > 1:
        raise ValueError("a sparse round runs on one device: devices=[...] with several devices is not supported")
    if isinstance(server_opt, DynState):
        raise TypeError("FedDyn state is not supported by a sparse round")
    k = agg.chunk_clients
    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1):
        raise ValueError(f"chunk_clients must be an int >= 1 or None, got {k!r}")


def weight_sum(weights: np.ndarray) -> np.float32:
    """wsum of a delta round: the float64 sum of the round's fp32 weights, rounded once to fp32."""
    return np.float32(np.sum(np.asarray(weights, dtype=np.float32).astype(np.float64)))


def _stand_ins(w_local_lst, keys, skeys):
    """The uploads with every sparse entry replaced by a zero-strided fp32 array of its shape (no
    memory behind it): what make_plan plans the round's numerics, key order and 8-byte buckets from."""
    w0 = w_local_lst[0]
    as_torch = any(isinstance(w0[k], torch.Tensor) for k in keys)
    zero_t, zero_n = torch.zeros((), dtype=torch.float32), np.float32(0)
    shapes = {k: sparse.entry_shape(w0[k]) for k in skeys}
    stand = {k: (zero_t.expand(shapes[k]) if as_torch else np.broadcast_to(zero_n, shapes[k])) for k in skeys}
    if len(skeys) == len(keys):
        return [stand] * len(w_local_lst)
    return [{k: stand[k] if k in stand else w[k] for k in keys} for w in w_local_lst]


def _pack_chunk(agg, g32: Group, entries, kstride: int, lo: int, hi: int, slot: int, device):
    """Clients [lo, hi) as one pinned int32 [K, kstride, 2] pair stack on the device: per row the keys'
    (index + the key's segment offset, bit pattern of the value) pairs in segment order — ascending
    columns of the bucket — then (na.SPARSE_PAD, 0) up to kstride.  Returns the device tensor."""
    k = hi - lo
    pk = agg.packer
    hq = pk._staging(("sp", slot), (k, kstride, 2), torch.int32)
    nq = hq.numpy().view(np.uint32)
    segs = [(s.key, s.offset) for s in g32.segments if s.numel]
    for r in range(k):
        mine, row, at = entries[lo + r], nq[r], 0
        for key, off in segs:
            idx, val = mine[key]
            m = idx.shape[0]
            row[at : at + m, 0] = idx + np.uint32(off)
            row[at : at + m, 1] = val.view(np.uint32)
            at += m
        row[at:, 0] = na.SPARSE_PAD
        row[at:, 1] = 0
    dq = pk.device_bucket(("sp", slot), (k, kstride, 2), torch.int32, device)
    dq.copy_(hq, non_blocking=True)
    pk._staging_used(("sp", slot), device)
    return dq


def ensemble_sparse(agg, agg_weight_lst, w_local_lst, key_lst=None, server_opt: ServerOptimizer | None = None,
                    center=None):
    """The weighted mean of top-k sparse uploads (sparse.py's format).  Per column c of the fp32 bucket:
    acc = init[c], then for the rows i in list order that hold an entry (c, v): acc = fl32(acc +
    fl32(a_i * v)); init is +0.0 for a non-delta round and fl32(wsum * g[c]) for a delta round, g being
    `center` (a w_glob-like dict: the server's own previous model) cast to fp32 and wsum weight_sum of
    the round's fp32 weights.  The divide, a fused AVGM / OPT update and the three output modes are the
    server step's.

    A non-delta round with finite weights >= 0 is bit-identical to ensemble(agg_weight_lst, the densified
    uploads, key_lst, server_opt) (a column whose only entries are -0.0 comes out +0.0).  A delta round is
    not: the centre enters once instead of once per row, which is what keeps the work proportional to the
    entries; its distance from the exact mean of the densified uploads is bounded in DESIGN.md section 23.

    The round is planned over zero-strided fp32 stand-ins of the sparse keys; the entries are packed into
    one pinned int32 [N, kstride, 2] pair stack (kstride: the round's largest per-row entry count, made
    even), one H2D, and one ops.sparse_fold_stack over the whole stride makes the accumulator.  Tensors of
    other dtypes (int64 BN counters, float64) are sent plain and aggregated as ever.  chunk_clients=K on
    the engine folds the round in chunks of K rows (at most na.SPARSE_MAX_CLIENTS) through the same
    kernel, with the same bits.  A round without sparse entries is `ensemble` itself.

    self.last_sparse = {"bytes_in", "bytes_fp32", "delta", "nnz", "kstride"} is the audit.  Refused before
    anything is queued: group= and several devices (ValueError); FedDyn state, float16 tensors and weights
    whose products are float64 (TypeError: the sum is fp32); a bucket whose stride does not fit uint32
    columns, delta uploads without a centre, and sparse.check_round's client-data errors."""
    _refuse(agg, server_opt)
    if len(w_local_lst) == 0 or len(agg_weight_lst) == 0 or len(agg_weight_lst) != len(w_local_lst):
        make_plan(agg_weight_lst, w_local_lst, key_lst)  # raises what `ensemble` raises
    keys = select_keys(w_local_lst, key_lst)
    skeys, delta, entries = sparse.check_round(w_local_lst, keys)
    if not skeys:
        agg.last_sparse = None
        return agg.ensemble(agg_weight_lst, w_local_lst, key_lst, server_opt)
    plan = make_plan(agg_weight_lst, _stand_ins(w_local_lst, keys, skeys), keys)
    if KIND_F16 in plan.groups:
        raise TypeError("float16 tensors in a sparse upload are not supported")
    g32 = plan.groups[KIND_F32]
    nm = g32.numerics
    if nm.mode == na.MODE_W64:
        raise TypeError("a sparse round sums in fp32: weights whose products are float64 (np.float64 / numpy "
                        "integer agg_weight) are not supported — use Python or np.float32 weights")
    if g32.stride >= na.SPARSE_PAD:
        raise ValueError(f"the fp32 bucket's {g32.stride} columns do not fit uint32 column indices")
    if delta and center is None:
        raise ValueError("delta uploads need the server's previous model: no centre was given")
    centre = agg._check_center(g32, center) if delta else None  # refused here, before anything is queued
    n = plan.n_clients
    counts = [sum(e[key][0].shape[0] for key in skeys) for e in entries]
    kstride = max(2, (max(counts) + 1) & ~1)
    agg.last_plan = plan
    agg.last_sparse = None
    packer = agg.packer
    device = agg.device
    rest = {kind: g for kind, g in plan.groups.items() if kind != KIND_F32}
    stacks8 = packer.pack(dataclasses.replace(plan, groups=rest), w_local_lst) if rest else {}
    k = min(n if agg.chunk_clients is None else int(agg.chunk_clients), n, na.SPARSE_MAX_CLIENTS)
    with torch.cuda.device(device):
        row = agg._center_row(g32, centre, device)
        weights = agg._weights(nm, device)
        wsum = float(weight_sum(nm.weights)) if delta else 0.0
        acc = packer.device_bucket(("acc", KIND_F32), (g32.stride,), torch.float32, device)
        ws = packer.device_bucket(("spws", KIND_F32), (ops.sparse_workspace(k, g32.stride),), torch.uint8, device)
        for j, lo in enumerate(range(0, n, k)):
            hi = min(n, lo + k)
            dq = _pack_chunk(agg, g32, entries, kstride, lo, hi, j % 2, device)
            # the whole stride in one launch: padding columns hold sums nobody reads
            ops.sparse_fold_stack(dq, weights[lo:hi], acc if lo else None, acc, center=None if lo else row, wsum=wsum,
                                  n_clients=hi - lo, n_cols=g32.stride, workspace=ws)
    agg.last_sparse = {"bytes_in": 8 * n * kstride, "bytes_fp32": 4 * n * g32.stride, "delta": delta,
                       "nnz": int(sum(counts)), "kstride": kstride}
    sums = {KIND_F32: [(packer.shards(plan, KIND_F32)[0], ops.FoldedSum(acc, na.ACC_F32, n, g32.stride))]}
    for kind, parts in stacks8.items():
        sums[kind] = parts
    results = agg._server_step(plan, sums, server_opt)
    for kind, parts in stacks8.items():
        packer.hold_slab(kind, [st for _, st in parts], parts[0][0].device)
    return agg._finish(plan, results)
