"""Wire codec — drop-in for flearn's ``Encrypt`` (flearn/common/Encrypt.py:17-44).

flearn's HTTP mode moves every upload and every global model as ``base64(pickle.dumps(obj))``:
clients encode in ``Client.upload`` (Client.py:201), the server decodes each upload in
``Server.ensemble`` (Server.py:126-131) and encodes the result (Server.py:142).  The reference
does this with ``base64.b64decode`` + ``pickle.loads`` on one core, after which the numpy arrays
are copied once more into the aggregation input.

``Encrypt`` here keeps the format byte for byte and makes the server side one pass:

* ``decode`` — a native restricted pickle scanner (flearn_amd/csrc/fa_wire.cpp) walks the pickle
  *through* the base64 text, decoding only its small header pieces, and reports every array
  payload as a (decoded offset, length) range.  The fp32 arrays of an upload's ``params`` are
  then decoded by a thread pool straight into ONE pinned row laid out exactly as the
  aggregation bucket (bucketplan.make_plan: key order, 64-element alignment), and handed back as
  numpy views of it — a plain dict of plain ndarrays, equal to what ``pickle.loads`` returns.
  When the engine later aggregates those uploads, the Packer recognises the rows and DMAs them
  to the GPU as they are (no pack copy).
* ``encode`` — the reference's pickle bytes, streamed by ``pickle.Pickler`` into a chunk list
  (large payloads by reference, pickle.dumps's own framing) and base64-encoded from those chunks
  by a multi-threaded native encoder writing directly into the result ``str``.

Safety: pickle content outside the scanner's subset (e.g. torch tensors) goes through a
*restricted* unpickler that only resolves numpy / torch / collections reconstructors; any other
global raises ``pickle.UnpicklingError`` — the reference's ``pickle.loads`` would execute it.
"""
from __future__ import annotations

import base64
import codecs
import collections
import ctypes
import io
import json
import math
import os
import pickle
import threading
import weakref
from typing import NamedTuple

import numpy as np
import torch

from . import _native as na
from .bucketplan import layout_slots, layout_stride, padded_span, row_layout

__all__ = ["BaseEncrypt", "Encrypt", "b64encode", "b64decode", "wire_row", "wire_device_stack",
           "release_device_staging"]

_F32 = np.dtype("<f4")

# CPython C API: zero-copy access to the bytes of an ASCII str, and str allocation
_AsUTF8AndSize = ctypes.pythonapi.PyUnicode_AsUTF8AndSize
_AsUTF8AndSize.restype = ctypes.c_void_p
_AsUTF8AndSize.argtypes = [ctypes.py_object, ctypes.POINTER(ctypes.c_ssize_t)]
_PyUnicode_New = ctypes.pythonapi.PyUnicode_New
_PyUnicode_New.restype = ctypes.py_object
_PyUnicode_New.argtypes = [ctypes.c_ssize_t, ctypes.c_uint32]
# a fresh, not yet shared bytes object whose buffer we fill (PyBytes_FromStringAndSize(NULL, n))
_PyBytes_New = ctypes.pythonapi.PyBytes_FromStringAndSize
_PyBytes_New.restype = ctypes.py_object
_PyBytes_New.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t]
_PyBytes_AsString = ctypes.pythonapi.PyBytes_AsString
_PyBytes_AsString.restype = ctypes.c_void_p
_PyBytes_AsString.argtypes = [ctypes.py_object]



def _probe_fill_in_place() -> bool:
    """The encoders write base64 text straight into a fresh str from PyUnicode_New(n, 127): a
    compact ASCII object whose UTF-8 view (PyUnicode_AsUTF8AndSize) IS its character buffer.
    That holds for CPython's PEP 393 strings (3.3+); it is checked here once, on the running
    interpreter, and the encoders fall back to base64.b64encode when it does not hold."""
    import sys

    if sys.implementation.name != "cpython" or sys.version_info < (3, 8):
        return False
    try:
        probe = _PyUnicode_New(8, 127)
        size = ctypes.c_ssize_t()
        p = _AsUTF8AndSize(probe, ctypes.byref(size))
        if not p or size.value != 8:
            return False
        ctypes.memmove(p, b"fA64prob", 8)
        return probe == "fA64prob" and len(probe) == 8
    except Exception:
        return False


_FILL_IN_PLACE = _probe_fill_in_place()

_THREADS = max(1, min(16, os.cpu_count() or 1))
_SERIAL_BYTES = 1 << 20  # below ~1 MB of payload, waking the pool costs more than it saves


def _threads(nbytes: int | None = None) -> int:
    return 1 if nbytes is not None and nbytes < _SERIAL_BYTES else _THREADS


def _ascii_ptr(s: str) -> tuple[int, int]:
    """(address, length) of the internal buffer of an ASCII str (no copy)."""
    size = ctypes.c_ssize_t()
    p = _AsUTF8AndSize(s, ctypes.byref(size))
    if not p:
        raise ValueError("string has no UTF-8 view")
    return p, size.value


def _check(L, rc, what):
    if rc != na.FA_OK:
        msg = L.fa_wire_last_error().decode(errors="replace")
        raise _WireError(rc, f"{what}: {msg}")


class _WireError(ValueError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


# ---------------------------------------------------------------------------------------------
# base64
# ---------------------------------------------------------------------------------------------


def b64encode(raw) -> str:
    """base64.b64encode(raw).decode() with the native encoder, written into the new str."""
    L = na.load()
    mv = memoryview(raw).cast("B")
    if not _FILL_IN_PLACE:
        return base64.b64encode(mv).decode("ascii")
    n = mv.nbytes
    m = 4 * ((n + 2) // 3)
    out = _PyUnicode_New(m, 127)
    if m == 0:
        return out
    dst, _ = _ascii_ptr(out)
    src = np.frombuffer(mv, dtype=np.uint8)
    _check(L, L.fa_b64_encode(src.ctypes.data, n, dst, m, _threads(n)), "base64 encode")
    return out


class _Chunks:
    """File object a pickle.Pickler streams into: keeps every chunk by reference (the pickler
    hands large payloads, e.g. array bytes, straight to write() and flushes its frames as
    separate bytes objects, with exactly pickle.dumps's framing)."""

    __slots__ = ("parts",)

    def __init__(self):
        self.parts = []

    def write(self, b):
        self.parts.append(b if type(b) is bytes else bytes(b))
        return len(self.parts[-1])


def pickle_b64(obj) -> str:
    """base64.b64encode(pickle.dumps(obj)).decode(), byte for byte, without joining the pickle
    into one bytes object: the chunks are base64-encoded in place, in order, natively."""
    sink = _Chunks()
    pickle.Pickler(sink, protocol=pickle.DEFAULT_PROTOCOL).dump(obj)
    parts = sink.parts
    if not _FILL_IN_PLACE:
        return b64encode(b"".join(parts))
    k = len(parts)
    n = sum(map(len, parts))
    m = 4 * ((n + 2) // 3)
    out = _PyUnicode_New(m, 127)
    if m == 0:
        return out
    L = na.load()
    dst, _ = _ascii_ptr(out)
    srcs = (ctypes.c_char_p * k)(*parts)  # the bytes objects' own buffers (kept alive by parts)
    lens = (ctypes.c_int64 * k)(*map(len, parts))
    _check(L, L.fa_b64_encode_gather(k, srcs, lens, dst, m, _threads(n)), "base64 encode")
    return out


def b64decode(s: str) -> bytes:
    """base64.b64decode(s) for canonical input (what b64encode produces), natively, into a new
    bytes object (no zero fill; io.BytesIO and pickle then read it without another copy)."""
    L = na.load()
    p, n = _ascii_ptr(s)
    total = L.fa_b64_decoded_size(p, n)
    if total < 0:
        raise _WireError(total, "not canonical base64")
    out = _PyBytes_New(None, total)
    if total:
        _check(L, L.fa_b64_decode(p, n, _PyBytes_AsString(out), total, _threads(total)), "base64 decode")
    return out


# ---------------------------------------------------------------------------------------------
# restricted unpickler (fallback for content outside the scanner's subset)
# ---------------------------------------------------------------------------------------------


def _load_storage_bytes(b):
    """torch.storage._load_from_bytes, but through torch.load(weights_only=True)."""
    return torch.load(io.BytesIO(b), weights_only=True)


class _RestrictedUnpickler(pickle.Unpickler):
    _NUMPY = {
        ("numpy._core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "_reconstruct"),
        ("numpy._core.multiarray", "scalar"), ("numpy.core.multiarray", "scalar"),
        ("numpy._core.numeric", "_frombuffer"), ("numpy.core.numeric", "_frombuffer"),
        ("numpy", "ndarray"), ("numpy", "dtype"),
    }
    _OTHER = {
        ("collections", "OrderedDict"): collections.OrderedDict,
        ("_codecs", "encode"): codecs.encode,  # protocol-2 bytes
        ("builtins", "bytearray"): bytearray,
        ("builtins", "set"): set,
        ("builtins", "frozenset"): frozenset,
        ("builtins", "complex"): complex,
        ("builtins", "slice"): slice,
        ("torch.storage", "_load_from_bytes"): _load_storage_bytes,
    }
    _TORCH = {"_rebuild_tensor_v2", "_rebuild_parameter", "_rebuild_parameter_with_state"}

    def find_class(self, module, name):
        if module == "__builtin__":  # protocol <= 2 spelling (fix_imports)
            module = "builtins"
        if (module, name) == ("builtins", "bytes"):
            return bytes
        if (module, name) in self._NUMPY or (module.startswith("numpy.dtypes") and name.endswith("DType")):
            return super().find_class(module, name)
        if (module, name) in self._OTHER:
            return self._OTHER[(module, name)]
        if module == "torch._utils" and name in self._TORCH:
            return super().find_class(module, name)
        if module == "torch" and (name == "Size" or name.endswith("Storage") or
                                  isinstance(getattr(torch, name, None), torch.dtype)):
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"global '{module}.{name}' is not allowed by the flearn_amd wire codec")


def restricted_loads(data) -> object:
    return _RestrictedUnpickler(io.BytesIO(data)).load()


# ---------------------------------------------------------------------------------------------
# pinned rows handed out by decode (weakly tracked, verified by address before reuse)
# ---------------------------------------------------------------------------------------------
class _Staged(NamedTuple):
    """Where _DeviceStage.stage put a decoded row: slot `slot` of round `gen` of `stage`."""
    stage: "_DeviceStage"
    gen: int
    slot: int


class _RowEntry(NamedTuple):
    """What the registry knows of one decoded params dict."""
    row_ref: weakref.ref  # its pinned row (a _RowArray), weakly
    layout: tuple  # the row's row_layout
    staged: _Staged | None  # its device copy, when decode staged one
    refs: tuple  # the arrays handed out, weakly, in layout order


_ROWS: dict[int, _RowEntry] = {}
# re-entrant: a row's weakref callback (_drop_entry) may run from the garbage collector while
# this thread already holds the lock
_ROWS_LOCK = threading.RLock()


class _RowArray(np.ndarray):
    """The numpy face of a pinned row; carries the torch tensor (`_fa_tensor`).  The arrays
    handed out are plain ndarray views whose base chain ends here, so the row lives exactly as
    long as any of them (the registry below only holds a weak reference)."""


def _register(params: dict, row_np: _RowArray, layout: tuple, staged=None):
    # the exact array objects handed out, weakly: wire_row then checks identity (an array that was
    # replaced is a different object; an array cannot move, so identity pins its address too)
    refs = tuple(weakref.ref(params[k]) for k, _, _ in layout_slots(layout))
    key = id(params)
    with _ROWS_LOCK:
        if len(_ROWS) > 4096:
            # over a snapshot: a weakref callback run by the collector during the scan deletes
            # from the dict (re-entrantly, under this same lock)
            for k in [k for k, ent in list(_ROWS.items()) if not _entry_alive(ent)]:
                _ROWS.pop(k, None)
        # the entry goes when its row dies (a params dict cannot be weakly referenced, so a dict
        # freed while its arrays live on leaves the entry behind: _live_entry drops it on lookup)
        _ROWS[key] = _RowEntry(weakref.ref(row_np, lambda r, k=key: _drop_entry(k, r)), layout, staged, refs)


def _entry_alive(ent: _RowEntry) -> bool:
    return ent.row_ref() is not None and all(r() is not None for r in ent.refs)


def _drop_entry(key: int, row_ref) -> None:
    with _ROWS_LOCK:
        ent = _ROWS.get(key)
        if ent is not None and ent.row_ref is row_ref:
            del _ROWS[key]


def _live_entry(params: dict):
    """The registry entry of this exact params dict, or None.  An entry is trusted only while its
    row and every array it handed out are alive AND are the ones the dict holds now: a dict at a
    reused id() (an earlier upload's dict freed, a new one allocated at the same address) never
    matches, and its stale entry is dropped here."""
    key = id(params)
    with _ROWS_LOCK:
        ent = _ROWS.get(key)
        if ent is None:
            return None
        if not _entry_alive(ent):
            del _ROWS[key]
            return None
    for (k, _shape, _off), ref in zip(layout_slots(ent.layout), ent.refs):
        if params.get(k) is not ref():
            with _ROWS_LOCK:
                if _ROWS.get(key) is ent:
                    del _ROWS[key]
            return None
    return ent


class _DeviceStage:
    """Device staging of decoded uploads (HTTP mode, `Encrypt(stage_to_device=True)`).

    flearn's server decodes every upload (Server.py:126-131) before it aggregates them
    (Server.py:140); the decode of upload i+1 is CPU work and the PCIe copy of upload i is DMA
    work, so they can overlap.  Each decoded row is copied, on a side stream, into slot i of a
    [cap, stride] device stack (one per device and layout) as soon as it is decoded; when the
    engine then aggregates exactly those uploads in that order, the stack IS the bucket and no
    H2D is left to do.  The copy is a snapshot taken at decode time."""

    def __init__(self, device: torch.device, layout: tuple):
        self.device, self.layout, self.stride = device, layout, layout_stride(layout)
        self.buf = None
        self.cap = 0
        self.n = 0  # rows staged in the current round
        self.gen = 0
        self.stream = torch.cuda.Stream(device)  # copies (copy engines): normal priority, streams.py
        self.done = None  # event after the last staged copy

    def stage(self, row: torch.Tensor):
        with torch.cuda.device(self.device):
            if self.n == 0:  # new round: slots may still be read by the previous round's reduce
                self.stream.wait_stream(torch.cuda.current_stream(self.device))
            if self.n == self.cap:
                cap = max(8, 2 * self.cap)
                with torch.cuda.stream(self.stream):
                    buf = torch.empty((cap, self.stride), dtype=torch.float32, device=self.device)
                    if self.n:
                        buf[: self.n].copy_(self.buf[: self.n], non_blocking=True)
                        self.buf.record_stream(self.stream)
                self.buf, self.cap = buf, cap
            with torch.cuda.stream(self.stream):
                # (torch's pinned-host allocator records this copy's event itself: the pinned row
                # is not reused before the DMA has read it)
                self.buf[self.n].copy_(row, non_blocking=True)
                self.done = torch.cuda.Event()
                self.done.record(self.stream)
        slot = self.n
        self.n += 1
        return _Staged(self, self.gen, slot)

    def take(self, n: int) -> torch.Tensor:
        """Hand the first n slots to the engine (its stream waits for the copies) and start a new
        round of slots."""
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.done)
        self.buf.record_stream(cur)  # read there by the reduce: not reused before it finishes
        view = self.buf[:n]
        self.gen += 1
        self.n = 0
        return view


_STAGES: dict = {}


def _stage_for(layout: tuple) -> _DeviceStage:
    dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev.index, layout)
    st = _STAGES.get(key)
    if st is None:
        st = _STAGES[key] = _DeviceStage(dev, layout)
    return st


def release_device_staging():
    """Free the device stacks of `stage_to_device` decoding."""
    _STAGES.clear()


def wire_device_stack(params_list, layout: tuple, device):
    """The staged device stack [N, stride] of these decoded uploads when every one was staged,
    in list order, into slots 0..N-1 of the same round on `device` and still holds the decoder's
    arrays — else None (the caller then DMAs the pinned rows or packs)."""
    ents = [_live_entry(p) for p in params_list]
    stages = {e.staged.stage for e in ents if e is not None and e.staged is not None}
    ok = bool(ents) and len(stages) == 1 and all(e is not None and e.staged is not None for e in ents)
    if ok:
        st, gen, _slot = ents[0].staged
        ok = st.device == torch.device(device) and st.n == len(ents) and gen == st.gen
        ok = ok and all(e.staged == (st, gen, i) and wire_row(p, layout) is not None
                        for i, (e, p) in enumerate(zip(ents, params_list)))
    if ok:
        return st.take(len(ents))
    for st in stages:  # these uploads go the pinned-row way: the next decode starts a new round
        st.gen += 1
        st.n = 0
    return None


def wire_row(params: dict, layout: tuple):
    """The pinned row behind a decoded upload's params when its fp32 arrays are still the
    decoder's views laid out as `layout` ((key, shape, offset), ..., stride) — else None."""
    ent = _live_entry(params)
    if ent is None or ent.layout != layout:
        return None
    row_np = ent.row_ref()
    return None if row_np is None else row_np._fa_tensor


# ---------------------------------------------------------------------------------------------
# decode: manifest -> objects
# ---------------------------------------------------------------------------------------------


class _Template:
    """The decode plan: everything decode_fast derives from a scanner manifest alone — the parsed
    tree (read-only once planned), the fp32 row's plan and layout, the aux-buffer layout and the
    payload ranges.  Uploads of one model with the same weight produce the same manifest text
    (pickle lays the same dict out the same way), so a round of N uploads plans once instead of
    N times; `build` then makes each upload's objects over its own row and aux buffer."""

    __slots__ = ("tree", "row_plan", "row_nodes", "layout", "aux_size", "offs", "lens", "rel", "in_row")

    def __init__(self, tree):
        self.tree = tree
        self.row_plan = {}  # id(node) -> row offset (elements)
        self.row_nodes = []  # the planned manifest nodes, in layout order
        self.layout = self._plan_row(tree)  # the pinned row's row_layout; None: no row
        self.aux_size = 0
        ranges = []  # per non-empty payload: (text offset, bytes, offset in its destination, is the row)
        self._place(tree, ranges)
        offs, lens, rel, in_row = zip(*ranges) if ranges else ((),) * 4
        self.offs, self.lens, self.rel = (np.array(c, np.int64) for c in (offs, lens, rel))
        self.in_row = np.array(in_row, bool)

    def _plan_row(self, tree):
        """Find the upload's params dict and lay out its fp32 C-order arrays as one row."""
        if not (isinstance(tree, dict) and "__d" in tree):
            return None
        params = None
        for k, v in tree["__d"]:
            if k == "params" and isinstance(v, dict) and ("__d" in v or "__od" in v):
                params = v
        if params is None:
            return None
        slots, stride = [], 0
        for k, v in params.get("__d", params.get("__od")):
            if not (isinstance(k, str) and isinstance(v, dict) and "__nd" in v):
                continue
            dt, shape, fortran, _off, _len, _ss = v["__nd"]
            if np.dtype(dt) != _F32 or (fortran and len(shape) > 1):
                continue
            self.row_plan[id(v)] = stride
            self.row_nodes.append(v)
            slots.append((k, tuple(shape), stride))
            stride += padded_span(math.prod(shape))
        return row_layout(slots, stride) if slots else None

    def _place(self, node, ranges):
        """One walk over the payload nodes: each gets its destination — its planned row slot,
        else the next 16-byte aligned place of the aux buffer (node["_aux"]) — and its text range."""
        if isinstance(node, list):
            for x in node:
                self._place(x, ranges)
        elif isinstance(node, dict):
            if "__nd" in node:
                o, ln = node["__nd"][3], node["__nd"][4]
            elif "__sc" in node:
                o, ln = node["__sc"][1], node["__sc"][2]
            elif "__b" in node:
                o, ln = node["__b"]
            else:
                for key in ("__t", "__d", "__od"):
                    if key in node:
                        self._place(node[key], ranges)
                return
            row = id(node) in self.row_plan
            if row:
                rel = 4 * self.row_plan[id(node)]
            else:
                rel = node["_aux"] = -(-self.aux_size // 16) * 16
                self.aux_size = rel + ln
            if ln:
                ranges.append((o, ln, rel, row))

    def build(self, node, row_np, aux_np, built):
        """The objects of one upload; built: id(node) -> the row view made for that planned node."""
        if isinstance(node, list):
            return [self.build(x, row_np, aux_np, built) for x in node]
        if not isinstance(node, dict):
            return node
        if "__nd" in node:
            dt, shape, fortran, _off, nbytes, setstate = node["__nd"]
            dtype = np.dtype(dt)
            if "_aux" not in node:
                o = self.row_plan[id(node)]
                arr = built[id(node)] = row_np[o : o + math.prod(shape)].view(np.ndarray).reshape(shape)
                return arr
            count = nbytes // dtype.itemsize if dtype.itemsize else 0
            flat = np.frombuffer(aux_np, dtype=dtype, count=count, offset=node["_aux"]) if count else np.empty(0, dtype)
            arr = flat.reshape(shape, order="F" if fortran else "C")
            if setstate and not dtype.isnative:  # ndarray.__setstate__ hands back native byte order
                arr = arr.astype(dtype.newbyteorder("="), order="K")
            return arr
        if "__sc" in node:
            dt, _off, nbytes = node["__sc"]
            return np.frombuffer(aux_np, dtype=np.dtype(dt), count=1, offset=node["_aux"])[0]
        if "__b" in node:
            o = node["_aux"]
            return bytes(aux_np[o : o + node["__b"][1]])
        if "__f" in node:
            return float.fromhex(node["__f"])
        if "__t" in node:
            return tuple(self.build(x, row_np, aux_np, built) for x in node["__t"])
        if "__dt" in node:
            return np.dtype(node["__dt"])
        if "__d" in node or "__od" in node:
            out = {} if "__d" in node else collections.OrderedDict()
            for k, v in node.get("__d", node.get("__od")):
                out[_hashable(self.build(k, row_np, aux_np, built))] = self.build(v, row_np, aux_np, built)
            return out
        raise _WireError(na.FA_ERR_UNSUPPORTED, f"unknown manifest node {list(node)}")


def _hashable(k):
    return tuple(_hashable(x) for x in k) if isinstance(k, list) else k


_GAPS: dict = {}  # row layout -> int64 indices of its alignment gaps


def _gap_index(layout: tuple) -> np.ndarray:
    idx = _GAPS.get(layout)
    if idx is None:
        parts, end = [], 0
        for _k, shape, off in layout_slots(layout):
            if off > end:
                parts.append(np.arange(end, off, dtype=np.int64))
            end = off + math.prod(shape)
        parts.append(np.arange(end, layout_stride(layout), dtype=np.int64))
        idx = np.concatenate(parts)
        if len(_GAPS) >= 64:
            _GAPS.clear()
        _GAPS[layout] = idx
    return idx


def _pinned_row(stride: int) -> torch.Tensor:
    return torch.empty(stride, dtype=torch.float32, pin_memory=torch.cuda.is_available())


_TEMPLATES: collections.OrderedDict = collections.OrderedDict()  # manifest text -> _Template
_TEMPLATES_MAX = 8
_TEMPLATES_LOCK = threading.Lock()


def _template(manifest: bytes) -> _Template:
    with _TEMPLATES_LOCK:
        t = _TEMPLATES.get(manifest)
        if t is not None:
            _TEMPLATES.move_to_end(manifest)
            return t
    t = _Template(json.loads(manifest.decode("utf-8")))
    with _TEMPLATES_LOCK:
        _TEMPLATES[manifest] = t
        while len(_TEMPLATES) > _TEMPLATES_MAX:
            _TEMPLATES.popitem(last=False)
    return t


def decode_fast(s: str, stage_to_device: bool = False):
    """Decode base64(pickle) text through the scanner; raises _WireError(FA_ERR_UNSUPPORTED /
    FA_ERR_DATA) when the content or the encoding is outside the fast path.  stage_to_device:
    also start the upload's H2D into a device staging stack (_DeviceStage)."""
    L = na.load()
    p, n = _ascii_ptr(s)
    cap = 1 << 16
    for _ in range(2):
        buf = ctypes.create_string_buffer(cap)
        need = ctypes.c_int64(0)
        rc = L.fa_pickle_scan_b64(p, n, buf, cap, ctypes.byref(need))
        if rc == na.FA_ERR_SIZE:
            cap = need.value + 1
            continue
        _check(L, rc, "pickle scan")
        break
    tmpl = _template(buf.raw[: need.value])
    layout = tmpl.layout
    aux_np = np.empty(max(tmpl.aux_size, 1), dtype=np.uint8)
    row, row_np = None, None
    if layout is not None:
        row = _pinned_row(layout_stride(layout))
        row_np = row.numpy().view(_RowArray)
        row_np._fa_tensor = row
        # zero the alignment gaps (reduced but never returned: keep them finite and deterministic)
        row_np[_gap_index(layout)] = 0
    if len(tmpl.offs):
        row_base = row_np.ctypes.data if row_np is not None else 0
        dsts = tmpl.rel + np.where(tmpl.in_row, row_base, aux_np.ctypes.data)
        rc = L.fa_b64_decode_ranges(p, n, len(tmpl.offs), tmpl.offs.ctypes.data, tmpl.lens.ctypes.data,
                                    dsts.ctypes.data, _threads(int(tmpl.lens.sum())))
        _check(L, rc, "payload decode")
    built = {}
    obj = tmpl.build(tmpl.tree, row_np, aux_np, built)
    if layout is not None:
        params = obj.get("params") if isinstance(obj, dict) else None
        if isinstance(params, dict):
            # the decoder's own views, laid out as planned (a key repeated in the pickled dict
            # would leave an earlier planned slot unreferenced: refuse rather than register it)
            for (k, _shape, _off), node in zip(layout_slots(layout), tmpl.row_nodes):
                if params.get(k) is not built.get(id(node)):
                    raise _WireError(na.FA_ERR_DATA, f"decoded array {k!r} is not in its planned slot")
            staged = None
            if stage_to_device and torch.cuda.is_available() and row.is_pinned():
                staged = _stage_for(layout).stage(row)
            _register(params, row_np, layout, staged)
    return obj


# ---------------------------------------------------------------------------------------------
# the codec objects
# ---------------------------------------------------------------------------------------------


FAST_MIN_CHARS = 2 << 20  # base64 characters from which uploads are decoded into pinned rows


class BaseEncrypt:
    """Identity codec (Encrypt.py:6-13)."""

    def encode(self, params):
        return params

    def decode(self, glob_params):
        return glob_params


class Encrypt(BaseEncrypt):
    """base64(pickle) codec, byte-compatible with flearn's Encrypt (Encrypt.py:16-44).
    fast_min_chars: strings from this length on are decoded into pinned bucket rows (default
    FAST_MIN_CHARS); shorter ones take native base64 + the restricted unpickler."""

    def __init__(self, fast_min_chars: int | None = None, stage_to_device: bool = False):
        self.fast_min_chars = FAST_MIN_CHARS if fast_min_chars is None else fast_min_chars
        # opt-in: copy each decoded upload to the GPU right away (overlaps PCIe with the next
        # decode); the engine then aggregates the device copy — a snapshot taken at decode time
        self.stage_to_device = stage_to_device

    def encode(self, params):
        """Encrypt.py:17-30: base64.b64encode(pickle.dumps(params)).decode() — the same text,
        encoded from the pickler's chunks (pickle_b64)."""
        return pickle_b64(params)

    def decode(self, glob_params):
        """Encrypt.py:32-44: pickle.loads(base64.b64decode(glob_params.encode())) — through the
        scanner and the pinned-row decoder when possible, else the restricted unpickler.
        Small strings (< fast_min_chars, e.g. a LeNet upload) take the native base64 + restricted
        unpickler route: the scanner's per-upload Python work (~0.3 ms) would exceed the pack
        copy it saves."""
        if isinstance(glob_params, str) and glob_params.isascii():
            if len(glob_params) >= self.fast_min_chars:
                try:
                    return decode_fast(glob_params, self.stage_to_device)
                except _WireError as e:
                    if e.code not in (na.FA_ERR_UNSUPPORTED, na.FA_ERR_DATA):
                        raise
                except (TypeError, ValueError):  # e.g. a dtype numpy rejects: let the unpickler report it
                    pass
            try:
                raw = b64decode(glob_params)
            except _WireError:
                raw = base64.b64decode(glob_params.encode())  # lenient input: the reference's decoder
            return restricted_loads(raw)
        return restricted_loads(base64.b64decode(glob_params.encode()))
