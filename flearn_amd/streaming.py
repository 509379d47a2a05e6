"""A round aggregated in chunks of clients: `RoundAccumulator` (Aggregator.begin_round).

The reference's sum is a running one — w = a0*x0; w += a_n*x_n in list order
(flearn/common/strategy/strategy.py:123-126) — so the engine does not need the whole [N][stride]
client stack at once.  Uploads are buffered until `chunk_clients` are present, packed with the
existing Packer on a chunk-sized plan of the same layout, and folded into a typed accumulator
(fa_fold); `finish()` divides by np.sum over the WHOLE weight list and applies the optional server
update (fa_fold_finish, strategy.py:127-129, avgm.py / opt.py / dyn.py).  Results are bit-identical
to `Aggregator.ensemble` on the same list; device memory is O(chunk_clients * stride) whatever the
client count, and uploads are aggregated as they arrive.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .bucketplan import TORCH_DTYPE, BucketPlan, Group, _as_array_meta, make_plan
from .ops import _ACC_TORCH, FoldedSum, acc_kind_of, fold_finish, fold_stack  # noqa: F401 (re-exported)
from .packer import Packer
from .semantics import _is_weight, resolve

_F16, _F64 = np.dtype(np.float16), np.dtype(np.float64)


class RoundAccumulator:
    """One round aggregated as it arrives: `add(upload)` per {"agg_weight", "params"} dict, then
    `finish()`, which returns exactly what `Aggregator.ensemble` returns for the same uploads.

    The layout and key set come from the first upload (or key_lst): every later upload must carry
    those keys with the same shapes and dtypes; extra keys are ignored.  The sum type of each bucket
    is np.result_type(weight, dtype) as semantics.resolve decides it, fixed by the first upload; the
    divide mode, the denominator and the output dtype come from resolve() on the whole weight list at
    finish().  `reorder` does not apply: a streamed round is always bit-exact."""

    #: the device buffers device_bytes counts, by the first element of their tag
    _device_tags = ("in", "acc", "out32", "out64", "dyn_g")

    def __init__(self, agg, key_lst=None, server_opt=None, chunk_clients: int = 16):
        if agg._dist:
            raise ValueError("a streamed round is not sharded over a process group (group=): use ensemble()")
        if len(agg.devices) > 1:
            raise ValueError("a streamed round runs on one device: devices=[...] with several devices is not supported")
        if not isinstance(chunk_clients, (int, np.integer)) or isinstance(chunk_clients, bool) or chunk_clients < 1:
            raise ValueError("chunk_clients must be an integer >= 1")
        self.agg = agg
        self.chunk_clients = int(chunk_clients)
        self.server_opt = server_opt
        self._key_lst = None if key_lst is None else list(key_lst)
        self._keys = None  # fixed by the first upload
        self._meta = None  # key -> (dtype, shape)
        self._input_kind = None
        self._acc_dtype = {}  # tensor dtype -> the sum dtype np.result_type gives under the weights
        self._pending = []  # uploads of the chunk being collected
        self._weights = []  # every weight so far (the divide needs the whole list)
        self._acc = {}  # bucket kind -> the accumulator holding the sum so far
        self._layout = None  # the first chunk's plan: groups, segments, strides
        self._chunks = 0
        self._finished = False
        self.max_stack_rows = 0  # the most client rows any packed chunk had

    # -- uploads ----------------------------------------------------------------------------
    def add(self, upload) -> None:
        if self._finished:
            raise RuntimeError("add() after finish(): begin a new round")
        w, params = upload["agg_weight"], upload["params"]
        if not _is_weight(w):
            raise TypeError(f"agg_weight must be a real scalar, got {type(w).__name__}")
        if self._keys is None:
            self._first(w, params)
        else:
            self._check(w, params)
        self._weights.append(w)
        self._pending.append((w, params))
        if len(self._pending) == self.chunk_clients:
            self._fold_pending()

    def _first(self, w, params) -> None:
        keys = list(params.keys()) if self._key_lst is None else self._key_lst
        meta, kinds, acc = {}, set(), {}
        for k in keys:
            if k not in params:
                raise KeyError(k)
            dt, shape, ik = _as_array_meta(params[k], f"client 0 key {k!r}")
            if dt == _F16:  # refused before anything is queued, as Aggregator._refuse_half does
                raise TypeError("float16 uploads: a streamed round aggregates fp32 / float64 / int64 buckets only "
                                "(use ensemble() without chunk_clients for a model.half() client)")
            meta[k] = (dt, tuple(shape))
            kinds.add(ik)
            if dt not in acc:
                acc[dt] = resolve([w], dt).acc_dtype
        if len(kinds) > 1:
            raise TypeError("mixing numpy arrays and torch tensors in one aggregation is not supported")
        self._keys, self._meta, self._acc_dtype = keys, meta, acc
        self._input_kind = kinds.pop() if kinds else "numpy"

    def _check(self, w, params) -> None:
        n = len(self._weights)
        for k in self._keys:
            if k not in params:
                raise KeyError(k)
            dt, shape, ik = _as_array_meta(params[k], f"client {n} key {k!r}")
            dt0, shape0 = self._meta[k]
            if dt != dt0 or tuple(shape) != shape0:
                raise ValueError(f"client {n} key {k!r}: {dt}{list(shape)} does not match client 0's {dt0}{list(shape0)}")
            if ik != self._input_kind:
                raise TypeError("mixing numpy arrays and torch tensors in one aggregation is not supported")
        for dt, a0 in self._acc_dtype.items():
            a = np.result_type(w, dt)
            if a != a0:
                raise TypeError(
                    "agg_weight types promote differently (" + ", ".join(sorted(map(str, {a, a0}))) + "); "
                    "the reference would mix precisions per client — use one weight type")

    # -- folding ----------------------------------------------------------------------------
    def _packer(self) -> Packer:
        """Two staging and stack sets alternate: chunk c + 1 is packed into the other set's pinned
        staging while chunk c's copies and fold run; a set's staging is rewritten only after the
        copy queued from it last has completed (Packer._staging waits for that event), and its
        device stack only by copies queued, on the same stream, behind the fold that read it."""
        agg = self.agg
        if getattr(agg, "_chunk_packers", None) is None:
            agg._chunk_packers = (agg.packer, Packer(agg.devices, agg.packer.workers))
        return agg._chunk_packers[self._chunks % 2]

    def chunk_plan(self, ws, ps) -> BucketPlan:
        """The chunk-sized plan of the round's layout (host only): the existing make_plan over the
        chunk's uploads and weights — the same keys, segments, offsets and strides as a plan of the
        whole list, the chunk's weights cast as numpy casts them."""
        plan = make_plan(ws, ps, self._keys)
        if self._layout is None:
            self._layout = plan
        elif any(k not in self._layout.groups or self._layout.groups[k].stride != g.stride
                 for k, g in plan.groups.items()) or len(plan.groups) != len(self._layout.groups):
            raise TypeError("agg_weight types promote differently between chunks; use one weight type")
        return plan

    def numerics(self, x_dtype):
        """semantics.resolve on the WHOLE weight list so far: the divide mode, np.sum over the list as
        the reference computes it, and the output dtype (why the divide is not fused into a fold)."""
        return resolve(self._weights, x_dtype)

    def _fold_pending(self) -> None:
        ws = [w for w, _ in self._pending]
        ps = [p for _, p in self._pending]
        self._pending = []
        plan = self.chunk_plan(ws, ps)
        agg, packer = self.agg, self._packer()
        dev = agg.device
        if self._chunks == 0:
            # both sets' chunk stacks at their full K rows from the first chunk on: what the round holds
            # on the device does not depend on how many uploads follow (device_bytes)
            for p in agg._chunk_packers:
                for kind, g in plan.groups.items():
                    p.device_bucket(("in", kind, 0), (self.chunk_clients, g.stride), TORCH_DTYPE[g.store_dtype], dev)
        stacks = packer.pack(plan, ps)
        self.max_stack_rows = max(self.max_stack_rows, len(ps))
        with torch.cuda.device(dev):
            for kind, parts in stacks.items():
                _, stack = packer.dense_stack(plan, kind, parts, len(ps))  # the chunk stack
                self._fold_bucket(packer, plan.groups[kind], stack, len(ps))
        self._chunks += 1

    def _fold_bucket(self, packer: Packer, g: Group, stack, n: int) -> None:
        """One bucket's chunk stack (n rows, packed by `packer`) into its accumulator."""
        agg, kind = self.agg, g.kind
        dev = agg.device
        ak = acc_kind_of(kind, g.numerics.mode)
        acc = agg.packer.device_bucket(("acc", kind), (g.stride,), _ACC_TORCH[ak], dev)
        fold_stack(ak, stack, agg._weights(g.numerics, dev), self._acc.get(kind), acc, n_clients=n)
        self._acc[kind] = acc
        packer.hold_slab(kind, [stack], dev)

    # -- the end of the round -----------------------------------------------------------------
    def _final_plan(self) -> BucketPlan:
        """The round's plan: the layout of the chunks, the numerics of the WHOLE weight list."""
        lay = self._layout
        groups = {}
        for kind, g in lay.groups.items():
            nm = self.numerics(g.segments[0].src_dtype)
            if nm.kind != kind or acc_kind_of(kind, nm.mode) != acc_kind_of(kind, g.numerics.mode):
                raise TypeError("agg_weight types promote differently over the round; use one weight type")
            groups[kind] = Group(kind, nm, g.segments, g.stride)
        return dataclasses.replace(lay, groups=groups, n_clients=len(self._weights), memo={})

    def finish(self):
        if self._finished:
            raise RuntimeError("finish() was already called: begin a new round")
        self._finished = True
        if not self._weights:
            make_plan([], [], self._key_lst)  # raises what ensemble([], []) raises
        if self._pending:
            self._fold_pending()
        agg = self.agg
        plan = self._final_plan()
        agg.last_plan = plan
        sums = {}  # the server step Aggregator.ensemble runs, over the sums already made
        for kind, g in plan.groups.items():
            (sh,) = agg.packer.shards(plan, kind)
            ak = acc_kind_of(kind, g.numerics.mode)
            sums[kind] = [(sh, FoldedSum(self._acc[kind], ak, len(self._weights), sh.width))]
        return agg._finish(plan, agg._server_step(plan, sums, self.server_opt))

    # -- memory -------------------------------------------------------------------------------
    @property
    def device_bytes(self) -> int:
        """Bytes of chunk stacks, accumulators and outputs this round holds on the device: it does
        not depend on how many uploads were added."""
        agg = self.agg
        total = 0
        packers = getattr(agg, "_chunk_packers", None) or (agg.packer,)
        seen = set()
        for p in packers:
            for (tag, _dev), t in p._dev.items():
                name = tag[0] if isinstance(tag, tuple) else tag
                if name in self._device_tags and id(t) not in seen:
                    seen.add(id(t))
                    total += t.numel() * t.element_size()
        return total
