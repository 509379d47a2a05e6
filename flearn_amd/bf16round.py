"""The bfloat16 round of the engine, bound on Aggregator as `ensemble_bf16`:
uploads whose floating tensors are bfloat16 — wire entries (bf16.py), CPU torch.bfloat16 tensors or
device-resident ones — are summed by ops.fold_bf16_stack from a device stack of two bytes per
parameter — the rows are never widened to fp32 in memory — into the fp32 accumulator every folded
round ends in, and the round ends in the server step every round ends in (Aggregator._server_step).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _native as na
from . import bf16, ops
from .bucketplan import SMALL_BYTES, BucketPlan, Group, Segment, make_plan, padded_span, select_keys
from .semantics import KIND_F16, KIND_F32
from .serverstate import DynState, ServerOptimizer

SEG_ALIGN = 8  # elements: a key starts on a 16-B load of fa_fold_bf16
STRIDE_ALIGN = 64  # elements: rows start on 128-B lines


def _refuse(agg, server_opt) -> None:
    """What the bfloat16 round does not do, refused before the uploads are looked at."""
    if agg._dist:
        raise ValueError("a bfloat16 round is not sharded over a process group (group=)")
    if len(agg.devices) > 1:
        raise ValueError("a bfloat16 round runs on one device: devices=[...] with several devices is not supported")
    if isinstance(server_opt, DynState):
        raise TypeError("FedDyn state is not supported by a bfloat16 round")
    k = agg.chunk_clients
    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1):
        raise ValueError(f"chunk_clients must be an int >= 1 or None, got {k!r}")


def _stand_ins(w_local_lst, keys, bkeys):
    """The uploads with every bfloat16 value replaced by a zero-strided fp32 array of its shape (no
    memory behind it): what make_plan plans the round's numerics, key order and 8-byte buckets from."""
    w0 = w_local_lst[0]
    as_torch = any(isinstance(w0[k], torch.Tensor) for k in keys)
    zero_t, zero_n = torch.zeros((), dtype=torch.float32), np.float32(0)
    shapes = {k: bf16.entry_shape(w0[k]) for k in bkeys}
    stand = {k: (zero_t.expand(shapes[k]) if as_torch else np.broadcast_to(zero_n, shapes[k])) for k in bkeys}
    if len(bkeys) == len(keys):
        return [stand] * len(w_local_lst)
    return [{k: stand[k] if k in stand else w[k] for k in keys} for w in w_local_lst]


def _bf16_plan(plan: BucketPlan) -> BucketPlan:
    """`plan` with its fp32 group laid out for fa_fold_bf16: every segment starts on an 8-element
    boundary (one 16-B load never spans two keys) and the stride is a multiple of 64 elements.  Kept in
    the base plan's memo: make_plan reuses plans across rounds."""
    bp = plan.memo.get("bf16plan")
    if bp is None:
        g = plan.groups[KIND_F32]
        segs, off = [], 0
        for s in g.segments:
            segs.append(Segment(s.key, s.shape, s.numel, off, s.src_dtype))
            off += padded_span(s.numel, SEG_ALIGN)
        off = -(-off // STRIDE_ALIGN) * STRIDE_ALIGN
        groups = dict(plan.groups)
        groups[KIND_F32] = Group(KIND_F32, g.numerics, segs, off)
        key_segment = dict(plan.key_segment)
        key_segment.update({s.key: s for s in segs})
        bp = plan.memo["bf16plan"] = BucketPlan(plan.keys, groups, plan.key_group, key_segment, plan.n_clients,
                                                plan.input_kind)
    return bp


def _pack_chunk(agg, g32: Group, rows, lo: int, hi: int, slot: int, device):
    """Clients [lo, hi) as one [K, stride] stack of bfloat16 bit patterns on the device (int16; padding
    is +0.0).  Host values (wire entries, CPU torch.bfloat16 tensors through an int16 view) are packed
    into a pinned stack, in groups of rows (the packer's threads, one row range each), and every
    group's H2D is queued while the next is packed; device-resident tensors are copied into their
    rows' columns on the same stream, after that H2D.  Returns the device tensor."""
    k, stride = hi - lo, g32.stride
    pk = agg.packer
    hq = pk._staging(("bf16", slot), (k, stride), torch.int16)
    nq = hq.numpy().view(np.uint16)
    segs = [(s.key, s.offset, s.numel) for s in g32.segments]
    # a staging buffer last written under this layout keeps its padding (only key bodies are rewritten)
    sig = (tuple(segs), k, stride)
    clean = pk.__dict__.setdefault("_bf16_clean", {})
    if clean.get(slot) != sig:
        nq[...] = 0
        clean[slot] = sig
    resident = []  # (row, offset, numel, device tensor)

    def rows_of(r0, r1):
        for r in range(r0, r1):
            mine, row = rows[lo + r], nq[r]
            for key, off, numel in segs:
                v = mine[key]
                if isinstance(v, torch.Tensor):
                    v = v.detach()
                    if v.device.type != "cpu":
                        resident.append((r, off, numel, v))  # (list.append: safe from the pack threads)
                        continue
                    v = v.contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)
                row[off : off + numel] = v

    dq = pk.device_bucket(("bf16", slot), (k, stride), torch.int16, device)
    threaded = k > 1 and pk.workers > 1 and 2 * k * stride >= SMALL_BYTES
    group = 2 * pk.workers if threaded else k
    for g0 in range(0, k, group):
        g1 = min(k, g0 + group)
        if threaded:
            step = -(-(g1 - g0) // pk.workers)
            list(pk._executor().map(lambda r0: rows_of(r0, min(g1, r0 + step)), range(g0, g1, step)))
        else:
            rows_of(g0, g1)
        dq[g0:g1].copy_(hq[g0:g1], non_blocking=True)
        for r, off, numel, v in resident:
            dq[r, off : off + numel].copy_(v.contiguous().view(torch.int16).reshape(-1), non_blocking=True)
        if resident:
            pk.hold([v for _, _, _, v in resident], device)
            resident.clear()
    pk._staging_used(("bf16", slot), device)
    return dq


def ensemble_bf16(agg, agg_weight_lst, w_local_lst, key_lst=None, server_opt: ServerOptimizer | None = None):
    """The weighted mean of bfloat16 uploads, bit-identical to ensemble(agg_weight_lst, the uploads
    widened to fp32, key_lst, server_opt): the server keeps fp32 sums and fp32 master weights, the
    clients' rows stay two bytes per parameter on the wire, over PCIe and in HBM.

    The round is planned with the plan's own numerics (make_plan over zero-strided fp32 stand-ins of
    the bfloat16 keys), its fp32 group re-laid with segments on 8-element boundaries and a stride that
    is a multiple of 64; the rows are packed into one pinned [N, stride] stack of bit patterns, each
    group of rows copied to the device while the next is packed, and one ops.fold_bf16_stack over the
    whole stride makes the fp32 accumulator: per column acc = fl32(a_0 * x_0), acc = fl32(acc +
    fl32(a_i * x_i)) in list order, x the exact fp32 of the bfloat16.  The divide, a fused AVGM / OPT
    update and the three output modes are the server step's.  A value may be a wire entry
    (bf16.encode_state_dict), a CPU torch.bfloat16 tensor or a device-resident one (copied into its
    row on the engine's stream).  Tensors of other dtypes (int64 BN counters, float64) are aggregated
    as ever.  chunk_clients=K on the engine folds the round in chunks of K rows through the same
    kernel (device memory O(K x model / 2)), with the same bits.  A round without bfloat16 values is
    `ensemble` itself.

    self.last_bf16 = {"bytes_in", "bytes_fp32"} is the audit: the bytes of the bfloat16 stack, and what
    the fp32 stack would have been.  Refused before anything is queued: group= and several devices
    (ValueError); FedDyn state and weights whose products are float64 (TypeError: the sum is fp32);
    and bf16.check_round's client-data errors."""
    _refuse(agg, server_opt)
    if len(w_local_lst) == 0 or len(agg_weight_lst) == 0 or len(agg_weight_lst) != len(w_local_lst):
        make_plan(agg_weight_lst, w_local_lst, key_lst)  # raises what `ensemble` raises
    keys = select_keys(w_local_lst, key_lst)
    bkeys, rows = bf16.check_round(w_local_lst, keys)
    if not bkeys:
        agg.last_bf16 = None
        return agg.ensemble(agg_weight_lst, w_local_lst, key_lst, server_opt)
    base = make_plan(agg_weight_lst, _stand_ins(w_local_lst, keys, bkeys), keys)
    if KIND_F16 in base.groups:
        raise TypeError("float16 tensors in a bfloat16 upload are not supported")
    nm = base.groups[KIND_F32].numerics
    if nm.mode == na.MODE_W64:
        raise TypeError("a bfloat16 round sums in fp32: weights whose products are float64 (np.float64 / numpy "
                        "integer agg_weight) are not supported — use Python or np.float32 weights")
    plan = _bf16_plan(base)
    g32 = plan.groups[KIND_F32]
    n = plan.n_clients
    agg.last_plan = plan
    agg.last_bf16 = None
    packer = agg.packer
    device = agg.device
    rest = {kind: g for kind, g in plan.groups.items() if kind != KIND_F32}
    stacks8 = packer.pack(dataclasses.replace(plan, groups=rest), w_local_lst) if rest else {}
    k = n if agg.chunk_clients is None else min(int(agg.chunk_clients), n)
    with torch.cuda.device(device):
        weights = agg._weights(nm, device)
        acc = packer.device_bucket(("acc", KIND_F32), (g32.stride,), torch.float32, device)
        for j, lo in enumerate(range(0, n, k)):
            hi = min(n, lo + k)
            dq = _pack_chunk(agg, g32, rows, lo, hi, j % 2, device)
            # the whole stride in one launch: padding columns hold sums nobody reads
            ops.fold_bf16_stack(dq, weights[lo:hi], acc if lo else None, acc, n_clients=hi - lo)
    agg.last_bf16 = {"bytes_in": 2 * n * g32.stride, "bytes_fp32": 4 * n * base.groups[KIND_F32].stride}
    sums = {KIND_F32: [(packer.shards(plan, KIND_F32)[0], ops.FoldedSum(acc, na.ACC_F32, n, g32.stride))]}
    for kind, parts in stacks8.items():
        sums[kind] = parts
    results = agg._server_step(plan, sums, server_opt)
    for kind, parts in stacks8.items():
        packer.hold_slab(kind, [st for _, st in parts], parts[0][0].device)
    return agg._finish(plan, results)
