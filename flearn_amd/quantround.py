"""The quantized round of the engine, bound on Aggregator as `ensemble_quantized` (DESIGN.md
section 17): uploads whose fp32 tensors are int8 block-quantized entries (quant.py) are summed by
ops.deq_fold_stack from a 1-byte-per-parameter device stack — the codes are never expanded to fp32
in memory — and the round ends in the server step every round ends in (Aggregator._server_step).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _native as na
from . import ops, quant
from .bucketplan import SMALL_BYTES, BucketPlan, Group, Segment, make_plan, padded_span, select_keys
from .semantics import KIND_F16, KIND_F32
from .serverstate import DynState, ServerOptimizer


def _refuse(agg, server_opt) -> None:
    """What the quantized round does not do, refused before the uploads are looked at."""
    if agg._dist:
        raise ValueError("a quantized round is not sharded over a process group (group=)")
    if len(agg.devices) > 1:
        raise ValueError("a quantized round runs on one device: devices=[...] with several devices is not supported")
    if isinstance(server_opt, DynState):
        raise TypeError("FedDyn state is not supported by a quantized round")
    k = agg.chunk_clients
    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1):
        raise ValueError(f"chunk_clients must be an int >= 1 or None, got {k!r}")


def _stand_ins(w_local_lst, keys, qkeys, entries):
    """The uploads with every quantized entry replaced by a zero-strided fp32 array of its shape (no
    memory behind it): what make_plan plans the round's numerics, key order and 8-byte buckets from."""
    as_torch = any(isinstance(w_local_lst[0][k], torch.Tensor) for k in keys if k not in entries[0])
    zero_t, zero_n = torch.zeros((), dtype=torch.float32), np.float32(0)
    stand = {k: (zero_t.expand(entries[0][k][0].shape) if as_torch else np.broadcast_to(zero_n, entries[0][k][0].shape))
             for k in qkeys}
    if len(qkeys) == len(keys):
        one = {k: stand[k] for k in keys}
        return [one] * len(w_local_lst)
    return [{k: stand[k] if k in stand else w[k] for k in keys} for w in w_local_lst]


def _q8_plan(plan: BucketPlan) -> BucketPlan:
    """`plan` with its fp32 group laid out for fa_deq_fold_q8: every segment starts on a 1024-column
    boundary (one scale block never spans two keys) and the stride is a multiple of 1024.  Kept in
    the base plan's memo: make_plan reuses plans across rounds."""
    qp = plan.memo.get("q8plan")
    if qp is None:
        g = plan.groups[KIND_F32]
        segs, off = [], 0
        for s in g.segments:
            segs.append(Segment(s.key, s.shape, s.numel, off, s.src_dtype))
            off += padded_span(s.numel, quant.BLOCK)
        groups = dict(plan.groups)
        groups[KIND_F32] = Group(KIND_F32, g.numerics, segs, off)
        key_segment = dict(plan.key_segment)
        key_segment.update({s.key: s for s in segs})
        qp = plan.memo["q8plan"] = BucketPlan(plan.keys, groups, plan.key_group, key_segment, plan.n_clients,
                                                plan.input_kind)
    return qp


def _pack_chunk(agg, g32: Group, entries, scales, lo: int, hi: int, slot: int, device):
    """Clients [lo, hi) as one pinned int8 [K, stride] code stack and one fp32 [K, stride / 1024] scale
    stack on the device; padding is code 0 with scale 0.  Rows are packed in groups (the packer's
    threads, one row range each) and every group's H2D is queued while the next is packed.  Returns
    the two device tensors."""
    k, stride = hi - lo, g32.stride
    nb = stride // quant.BLOCK
    pk = agg.packer
    hq = pk._staging(("q8", slot), (k, stride), torch.int8)
    hs = pk._staging(("q8s", slot), (k, nb), torch.float32)
    nq, ns = hq.numpy(), hs.numpy()
    segs = [(s.key, s.offset, s.numel, s.offset // quant.BLOCK, quant.n_blocks(s.numel),
             s.offset + padded_span(s.numel, quant.BLOCK)) for s in g32.segments]
    dense = all(b * quant.BLOCK == end - off for _, off, _, _, b, end in segs)  # no empty key: the scales are one run
    # a staging buffer last written under this layout keeps its padding (only key bodies are rewritten)
    sig = (tuple((off, numel) for _, off, numel, _, _, _ in segs), k, stride)
    clean = pk.__dict__.setdefault("_q8_clean", {})
    if clean.get(slot) != sig:
        nq[...] = 0
        ns[...] = 0
        clean[slot] = sig

    def rows(r0, r1):
        for r in range(r0, r1):
            e, row = entries[lo + r], nq[r]
            for key, off, numel, b0, b, end in segs:
                row[off : off + numel] = e[key][0].reshape(-1)
            if dense:
                ns[r] = scales[lo + r]
            else:
                for key, off, numel, b0, b, end in segs:
                    ns[r, b0 : b0 + b] = e[key][1]

    dq = pk.device_bucket(("q8", slot), (k, stride), torch.int8, device)
    ds = pk.device_bucket(("q8s", slot), (k, nb), torch.float32, device)
    threaded = k > 1 and pk.workers > 1 and k * stride >= SMALL_BYTES
    group = 2 * pk.workers if threaded else k
    for g0 in range(0, k, group):
        g1 = min(k, g0 + group)
        if threaded:
            step = -(-(g1 - g0) // pk.workers)
            list(pk._executor().map(lambda r0: rows(r0, min(g1, r0 + step)), range(g0, g1, step)))
        else:
            rows(g0, g1)
        dq[g0:g1].copy_(hq[g0:g1], non_blocking=True)
    ds.copy_(hs, non_blocking=True)
    pk._staging_used(("q8", slot), device)
    pk._staging_used(("q8s", slot), device)
    return dq, ds


def ensemble_quantized(agg, agg_weight_lst, w_local_lst, key_lst=None, server_opt: ServerOptimizer | None = None,
                       center=None):
    """The weighted mean of int8 block-quantized uploads (quant.py's format; FedPAQ, Reisizadeh et al.
    2020), bit-identical to ensemble(agg_weight_lst, the dequantized uploads, key_lst, server_opt).

    The round is planned with the plan's own numerics (make_plan over zero-strided fp32 stand-ins of
    the quantized keys), its fp32 group re-laid with segments on 1024-column boundaries; the codes are
    packed into one pinned int8 [N, stride] stack and the scales into [N, stride / 1024], one H2D of
    each (a quarter of the fp32 bytes over PCIe and in HBM), and one ops.deq_fold_stack over the whole
    stride makes the fp32 accumulator: per column acc = fl32(a_0 * x_0), acc = fl32(acc + fl32(a_i *
    x_i)) in list order, x = fl32(scale * q), or fl32(g + fl32(scale * q)) for delta uploads, g being
    `center` (a w_glob-like dict: the server's own previous model) cast to fp32.  The divide, a fused
    AVGM / OPT update and the three output modes are the server step's.  Tensors of other dtypes
    (int64 BN counters, float64) are sent plain and aggregated as ever.  chunk_clients=K on the engine
    folds the round in chunks of K rows through the same kernel (device memory O(K x model / 4)),
    with the same bits.  A round without quantized entries is `ensemble` itself.

    self.last_quant = {"bytes_in", "bytes_fp32", "delta", "blocks"} is the audit: the bytes of codes
    and scales copied to the device, what the fp32 stack would have been, the round's delta flag and
    the scale blocks read.  Refused before anything is queued: group= and several devices
    (ValueError); FedDyn state, device-resident code tensors, float16 tensors and weights whose
    products are float64 (TypeError: the sum is fp32); and quant.check_round's client-data errors —
    a scale that is negative, NaN or inf, a wrong scale count, q8 that is not int8, shapes or delta
    flags that differ between clients, a key quantized by some clients only, a plain fp32 tensor,
    block != 1024 — and delta uploads without a centre (ValueError)."""
    _refuse(agg, server_opt)
    if len(w_local_lst) == 0 or len(agg_weight_lst) == 0 or len(agg_weight_lst) != len(w_local_lst):
        make_plan(agg_weight_lst, w_local_lst, key_lst)  # raises what `ensemble` raises
    keys = select_keys(w_local_lst, key_lst)
    qkeys, delta, entries, scales = quant.check_round(w_local_lst, keys)
    if not qkeys:
        agg.last_quant = None
        return agg.ensemble(agg_weight_lst, w_local_lst, key_lst, server_opt)
    base = make_plan(agg_weight_lst, _stand_ins(w_local_lst, keys, qkeys, entries), keys)
    if KIND_F16 in base.groups:
        raise TypeError("float16 tensors in a quantized upload are not supported")
    nm = base.groups[KIND_F32].numerics
    if nm.mode == na.MODE_W64:
        raise TypeError("a quantized round sums in fp32: weights whose products are float64 (np.float64 / numpy "
                        "integer agg_weight) are not supported — use Python or np.float32 weights")
    plan = _q8_plan(base)
    g32 = plan.groups[KIND_F32]
    if delta and center is None:
        raise ValueError("delta uploads need the server's previous model: no centre was given")
    centre = agg._check_center(g32, center) if delta else None  # refused here, before anything is queued
    n = plan.n_clients
    agg.last_plan = plan
    agg.last_quant = None
    packer = agg.packer
    device = agg.device
    rest = {kind: g for kind, g in plan.groups.items() if kind != KIND_F32}
    stacks8 = packer.pack(dataclasses.replace(plan, groups=rest), w_local_lst) if rest else {}
    k = n if agg.chunk_clients is None else min(int(agg.chunk_clients), n)
    with torch.cuda.device(device):
        row = agg._center_row(g32, centre, device)
        weights = agg._weights(nm, device)
        acc = packer.device_bucket(("acc", KIND_F32), (g32.stride,), torch.float32, device)
        for j, lo in enumerate(range(0, n, k)):
            hi = min(n, lo + k)
            dq, ds = _pack_chunk(agg, g32, entries, scales, lo, hi, j % 2, device)
            # the whole stride in one launch: padding columns hold sums nobody reads
            ops.deq_fold_stack(dq, ds, weights[lo:hi], acc if lo else None, acc, center=row, n_clients=hi - lo)
    nb = g32.stride // quant.BLOCK
    agg.last_quant = {"bytes_in": n * g32.stride + 4 * n * nb, "bytes_fp32": 4 * n * base.groups[KIND_F32].stride,
                      "delta": delta, "blocks": n * nb}
    sums = {KIND_F32: [(packer.shards(plan, KIND_F32)[0], ops.FoldedSum(acc, na.ACC_F32, n, g32.stride))]}
    for kind, parts in stacks8.items():
        sums[kind] = parts
    results = agg._server_step(plan, sums, server_opt)
    for kind, parts in stacks8.items():
        packer.hold_slab(kind, [st for _, st in parts], parts[0][0].device)
    return agg._finish(plan, results)
