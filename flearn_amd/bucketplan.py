"""Bucket planning of client state_dicts (packer.py copies them in; rowtable.py: device uploads).

The reference reduces key by key, N x K numpy calls over many small tensors
(flearn/common/strategy/strategy.py:123-126; ResNet-18 has 102 fp32 tensors, median 256
elements).  Here every selected key of every client is flattened into ONE row of a device
matrix per arithmetic kind ("bucket"), so a whole aggregation is one kernel launch:

    f32 bucket  [N, stride]  fp32 tensors (weights, biases, BN running stats)
    f16 bucket  [N, stride]  float16 tensors (a model.half() client's uploads): 2-byte elements,
                             segments on 8-element (16-B) boundaries
    f64 bucket  [N, stride]  float64 tensors, and int64 buffers numpy promotes to float64
    i64 bucket  [N, stride]  int64 buffers under integer weights (stay int64 in numpy)

Each key occupies a segment [offset, offset+numel) of its bucket row; segments start on
ALIGN-element (256-byte) boundaries and the row stride is a multiple of ALIGN, so every row of
every segment is 16-byte aligned for the dwordx4 loads, and rows never share a cache line.
Padding elements are zero and never read back.
"""
from __future__ import annotations

import collections
import math
import threading
from dataclasses import dataclass, field
from functools import cached_property, reduce
from typing import NamedTuple

import numpy as np
import torch

from . import _native as na
from .semantics import KIND_F16, KIND_F32, KIND_F64, KIND_I64, Numerics, resolve, resolve_half

ALIGN = 64  # elements: 256 B for fp32, 512 B for 8-byte kinds
ALIGN_F16 = 8  # elements: float16 segments start on 16 B (one buffer load of fa_reduce_f16)
STRIDE_ALIGN_F16 = 128  # elements: the float16 row stride is a multiple of 256 B
SMALL_BYTES = 4 << 20  # below this, host packing / unpacking runs on the calling thread

_STORE = {KIND_F32: np.float32, KIND_F64: np.float64, KIND_I64: np.int64, KIND_F16: np.float16}
TORCH_DTYPE = {np.float32: torch.float32, np.float64: torch.float64, np.int64: torch.int64, np.float16: torch.float16}
_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64, torch.float16: np.float16}
FMT = {np.dtype(np.float32): ord("f"), np.dtype(np.float64): ord("d"), np.dtype(np.int64): ord("i"),
        np.dtype(np.float16): ord("e")}


def padded_span(numel: int, align: int = ALIGN) -> int:
    """Elements a key takes of its row: at least one, rounded up to `align`.  The bucket plan, the
    wire decoder's pinned rows and the client update's flat layout agree because all use this."""
    return -(-max(numel, 1) // align) * align


def row_layout(slots, stride: int) -> tuple:
    """The layout of one fp32 row as wire.wire_row compares it: ((key, shape, offset), ..., stride)."""
    return tuple(slots) + (stride,)


def layout_slots(layout: tuple) -> tuple:
    """The (key, shape, offset) of every key of a row_layout."""
    return layout[:-1]


def layout_stride(layout: tuple) -> int:
    return layout[-1]


def _as_list(w_local_lst) -> list:
    """The uploads as a list (the native walks take nothing else), the caller's own when it is one."""
    return w_local_lst if type(w_local_lst) is list else list(w_local_lst)


@dataclass
class Segment:
    key: str
    shape: tuple
    numel: int
    offset: int
    src_dtype: np.dtype


@dataclass
class Group:
    kind: str
    numerics: Numerics
    segments: list = field(default_factory=list)
    stride: int = 0

    @property
    def store_dtype(self):
        return _STORE[self.kind]

    @cached_property
    def row_layout(self) -> tuple:
        """This (finished) group's row as a row_layout: what the wire codec's rows are matched against."""
        return row_layout(((s.key, s.shape, s.offset) for s in self.segments), self.stride)


def key_runs(g: Group) -> list:
    """The column ranges [c0, c1) of a bucket that hold keys and nothing else: consecutive keys with
    no padding between them form one run.  What a Gram is taken over: a stack's padding columns are
    never written by a pack and may hold another layout's values."""
    runs = []
    for s in g.segments:
        if s.numel == 0:
            continue
        if runs and runs[-1][1] == s.offset:
            runs[-1][1] = s.offset + s.numel
        else:
            runs.append([s.offset, s.offset + s.numel])
    return [tuple(r) for r in runs]


@dataclass
class BucketPlan:
    keys: list  # output key order
    groups: dict  # kind -> Group
    key_group: dict  # key -> kind
    key_segment: dict  # key -> Segment
    n_clients: int
    input_kind: str  # "numpy" | "torch"
    # derived per-plan data of the packer (pieces, native pack tables); plans are reused across
    # rounds (make_plan's cache), so this is computed once per model layout and staging buffer
    memo: dict = field(default_factory=dict, compare=False, repr=False)

    @property
    def f32(self):
        return self.groups.get(KIND_F32)


def _as_array_meta(v, where):
    """(dtype, shape, kind) of one uploaded value without copying it."""
    if isinstance(v, (np.ndarray, np.generic)):
        return v.dtype, v.shape, "numpy"
    if isinstance(v, torch.Tensor):
        if v.layout != torch.strided:
            # sparse / mkldnn / nested uploads: client data the engine does not take (TypeError ->
            # the server_exception route), never a torch error from deep inside the pack
            raise TypeError(f"{where}: {v.layout} tensor uploads are not supported (dense tensors only)")
        return np.dtype(str(v.dtype).replace("torch.", "")), tuple(v.shape), "torch"
    raise TypeError(f"{where}: unsupported value type {type(v).__name__} (expected ndarray or Tensor)")


def _raw_signature(w, keys):
    """(type, dtype, shape, layout) of every selected value, as the objects report them (no
    normalisation): equal signatures mean equal metadata, so only the first client needs the
    per-key checks (10,200 of them for 100 ResNet-18 uploads)."""
    try:
        return tuple((type(v), v.dtype, v.shape, getattr(v, "layout", None)) for v in map(w.__getitem__, keys))
    except (AttributeError, KeyError):
        return None


def _plain_dicts(w_local_lst) -> bool:
    """Every upload is a dict / OrderedDict, whose item lookup the native walks reproduce."""
    return all(type(w) in (dict, collections.OrderedDict) for w in w_local_lst)


def _same_signature_native(w_local_lst, keys, sig0=None) -> bool:
    """True when every client's (type, dtype, shape, layout) per key equals client 0's, read
    natively: numpy uploads through the buffer protocol (csrc/fa_pyhost.c fa_py_same_signature:
    type, format, itemsize, shape — numpy arrays are always strided), torch uploads from the
    tensors' TensorImpl (csrc/fa_torchmeta.cpp) — the same comparisons as _raw_signature without
    the per-attribute interpreter work; False when it differs or cannot tell (the caller then
    compares in Python)."""
    if len(w_local_lst) < 2 or not _plain_dicts(w_local_lst):
        return False
    lst = _as_list(w_local_lst)
    if sig0 is not None and sig0 and all(t[0] is np.ndarray for t in sig0):
        return na.load_pyhost().fa_py_same_signature(lst, tuple(keys)) == 1
    L = na.load_torchmeta()
    return L is not None and L.fa_tm_same_signature(lst, tuple(keys)) == 1


def select_keys(w_local_lst, key_lst=None):
    """strategy.py:119-121: the keys common to every client when key_lst is None, else key_lst.
    Ordered by the first client's insertion order (the reference's order is set-hash order,
    so any fixed order is equally faithful; this one is deterministic)."""
    if key_lst is not None:
        keys = list(key_lst)
        for n, w in enumerate(w_local_lst):
            for k in keys:
                if k not in w:
                    raise KeyError(k)
        return keys
    k0 = w_local_lst[0].keys()
    if all(w.keys() == k0 for w in w_local_lst[1:]):  # the usual case: one model, same keys (C-level set compare)
        return list(k0)
    common = reduce(lambda a, b: a & b, [set(w.keys()) for w in w_local_lst])
    return [k for k in w_local_lst[0].keys() if k in common]


_PLANS: collections.OrderedDict = collections.OrderedDict()  # recent plans (read-only once built)
_PLANS_MAX = 8
_PLANS_LOCK = threading.Lock()


def _plan_keys(w_local_lst, key_lst):
    """(keys, sig0, slow): the selected keys, client 0's _raw_signature of them (or None) and the
    clients not known to have client 0's metadata — _build_plan compares those key by key."""
    if key_lst is None and len(w_local_lst) > 1:
        # the usual round: client 0's keys, verified natively in every client together with their
        # metadata — a client missing one of them makes the native check give up (the general
        # intersection below then runs), so passing it proves the intersection is client 0's keys
        k0 = list(w_local_lst[0].keys())
        s0 = _raw_signature(w_local_lst[0], k0)
        if s0 is not None and _same_signature_native(w_local_lst, k0, s0):
            return k0, s0, []
    keys = select_keys(w_local_lst, key_lst)
    sig0 = _raw_signature(w_local_lst[0], keys)
    if sig0 is not None and _same_signature_native(w_local_lst, keys, sig0):
        return keys, sig0, []
    return keys, sig0, [n for n in range(1, len(w_local_lst))
                        if sig0 is None or _raw_signature(w_local_lst[n], keys) != sig0]


def make_plan(agg_weight_lst, w_local_lst, key_lst=None) -> BucketPlan:
    """The bucket plan of one aggregation.  A federated run aggregates the same model with the
    same weights round after round, so a plan is reused when the selected keys, every client's
    (type, dtype, shape, layout) per key, the client count and the weights (types and exact values, by
    repr: -0.0 and NaN included) all equal a recent call's."""
    if len(w_local_lst) == 0 or len(agg_weight_lst) == 0:
        raise IndexError("list index out of range")  # reference: agg_weight_lst[0] (strategy.py:123)
    if len(agg_weight_lst) != len(w_local_lst):
        raise ValueError("agg_weight_lst and w_local_lst differ in length")
    keys, sig0, slow = _plan_keys(w_local_lst, key_lst)
    ck = None
    if sig0 is not None and not slow:
        ck = (tuple(keys), sig0, len(w_local_lst), tuple(map(type, agg_weight_lst)), repr(list(agg_weight_lst)))
        try:
            with _PLANS_LOCK:
                plan = _PLANS.get(ck)
                if plan is not None:
                    _PLANS.move_to_end(ck)
                    return plan
        except TypeError:  # something unhashable in the metadata: plan afresh, uncached
            ck = None
    plan = _build_plan(agg_weight_lst, w_local_lst, keys, slow)
    if ck is not None:
        with _PLANS_LOCK:
            _PLANS[ck] = plan
            while len(_PLANS) > _PLANS_MAX:
                _PLANS.popitem(last=False)
    return plan


def _build_plan(agg_weight_lst, w_local_lst, keys, slow) -> BucketPlan:
    numerics_by_dtype = {}
    groups: dict = {}
    key_group = {}
    key_segment = {}
    input_kinds = set()
    for k in keys:
        dt, shape, ik = _as_array_meta(w_local_lst[0][k], f"client 0 key {k!r}")
        input_kinds.add(ik)
        for n in slow:  # clients whose metadata differs somewhere: find and report it
            dtn, shn, ikn = _as_array_meta(w_local_lst[n][k], f"client {n} key {k!r}")
            input_kinds.add(ikn)
            if dtn != dt or shn != shape:
                raise ValueError(f"client {n} key {k!r}: {dtn}{list(shn)} does not match client 0's {dt}{list(shape)}")
        if dt not in numerics_by_dtype:
            # float16: numpy and torch uploads do not compute the same thing (semantics.resolve_half)
            numerics_by_dtype[dt] = (resolve_half(agg_weight_lst, ik) if dt == np.float16
                                     else resolve(agg_weight_lst, dt))
        nm = numerics_by_dtype[dt]
        g = groups.get(nm.kind)
        if g is None:
            g = groups[nm.kind] = Group(nm.kind, nm)
        elif g.numerics is not nm and not _same_numerics(g.numerics, nm):
            # (identity first: the dataclass __eq__ would compare the weight arrays elementwise
            # and raise for more than one client — a float64 model with int64 BN counters put
            # two dtypes' numerics into the f64 bucket and failed here)
            raise TypeError(f"key {k!r} needs different arithmetic than the rest of its bucket")
        numel = int(math.prod(shape))
        seg = Segment(k, shape, numel, g.stride, dt)
        g.segments.append(seg)
        key_segment[k] = seg
        g.stride += padded_span(numel, ALIGN_F16 if nm.kind == KIND_F16 else ALIGN)
        key_group[k] = nm.kind
    if KIND_F16 in groups:
        g = groups[KIND_F16]
        g.stride = -(-g.stride // STRIDE_ALIGN_F16) * STRIDE_ALIGN_F16
    if len(input_kinds) > 1:
        raise TypeError("mixing numpy arrays and torch tensors in one aggregation is not supported")
    return BucketPlan(keys, groups, key_group, key_segment, len(w_local_lst), input_kinds.pop() if input_kinds else "numpy")


def _same_numerics(a: Numerics, b: Numerics) -> bool:
    return ((a.kind, a.mode, a.denom, a.out_dtype) == (b.kind, b.mode, b.denom, b.out_dtype)
            and np.array_equal(a.weights, b.weights))


@dataclass(frozen=True)
class Shard:
    """A column range [c0, c1) of the f32 bucket that lives on one device (multi-GPU ingest).
    Non-f32 buckets (f64 / i64: BN counters, a few bytes) always live on shard 0."""

    index: int
    device: torch.device
    c0: int
    c1: int

    @property
    def width(self) -> int:
        return self.c1 - self.c0


def rank_width(stride: int, world: int) -> int:
    """Columns per rank of a column-sharded process group: equal, ALIGN-aligned (the last ranks'
    ranges may be short or empty; the all-gather pads them)."""
    return -(-stride // (world * ALIGN)) * ALIGN


def split_columns(stride: int, devices) -> list:
    """Near-equal ALIGN-aligned column ranges of a stride-wide bucket, one per device."""
    k = len(devices)
    units = stride // ALIGN
    bounds = [ALIGN * (units * i // k) for i in range(k + 1)]
    bounds[-1] = stride
    return [Shard(i, torch.device(d), bounds[i], bounds[i + 1]) for i, d in enumerate(devices)]


class Piece(NamedTuple):
    """Elements [src_lo, src_hi) of one flattened value: columns [dst_lo, ...) of one shard's stack."""
    segment: Segment
    src_lo: int
    src_hi: int
    shard: Shard
    dst_lo: int
