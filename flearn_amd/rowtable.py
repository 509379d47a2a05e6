"""Device-resident uploads of one bucket group read where they lie: their pointer table (`row_ptrs`),
the one-allocation case that needs none (`slab_stack`) and `RowTable`, what the row kernels take."""
import ctypes

import numpy as np
import torch

from . import _native as na
from .bucketplan import TORCH_DTYPE, BucketPlan, Group, _as_list, _plain_dicts

# device-upload dtypes a group's row table takes, and their fa_gather_rows_f64 source kind
_ROW_SOURCES = {torch.float64: {torch.float64: na.SRC_F64, torch.int64: na.SRC_I64, torch.float32: na.SRC_F32}}


def slab_stack(plan: BucketPlan, g: Group, w_local_lst, rp):
    """The uploads as a [N, stride] stack view when every client's fp32 tensors sit in ONE
    allocation laid out exactly as this bucket — key k of client n at row_base + n * pitch +
    offset(k), the same pitch for every client (flearn_amd.device_state_dicts makes such
    uploads) — else None.  The stack kernel then reads them in place: no pointer table, and
    the translations of one allocation instead of one per (client, tensor) (the row-pointer
    kernel's 7-8% at NS)."""
    segs, ptrs, keep, _src = rp
    n = plan.n_clients
    if not segs or ptrs.shape[1] != n:
        return None
    off = np.array([s.offset for s in segs], dtype=np.int64) * 4
    base = ptrs[0] - off[0]  # each client's row start
    if not np.array_equal(ptrs - off[:, None], np.broadcast_to(base, ptrs.shape)):
        return None
    pitch = int(base[1] - base[0]) if n > 1 else g.stride * 4
    if n > 1 and not (np.diff(base) == pitch).all():
        return None
    if pitch < g.stride * 4 or pitch % 16 or int(base[0]) % 16:
        return None
    t0 = w_local_lst[0][segs[0].key]
    st = t0.untyped_storage()
    lo, hi = st.data_ptr(), st.data_ptr() + st.nbytes()
    first, end = int(base[0]), int(base[0]) + (n - 1) * pitch + g.stride * 4
    if first < lo or end > hi:  # the rows must lie inside that one allocation
        return None
    return torch.empty(0, dtype=torch.float32, device=t0.device).set_(
        st, (first - lo) // 4, (n, g.stride), (pitch // 4, 1))


def row_ptrs(plan: BucketPlan, g: Group, w_local_lst, shards):
    """(segments, pointer table [segments][clients], tensors kept, source kinds) of
    device-resident uploads — RowTable's inputs — or None when some value is not a contiguous
    tensor of an accepted dtype on the bucket's (single, whole-bucket) device.  Accepted: the
    store dtype; for the float64 group also int64 and float32 values (BN num_batches_tracked),
    which fa_gather_rows_f64 converts as numpy's promotion does."""
    if len(shards) != 1 or shards[0].c0 != 0 or shards[0].c1 != g.stride:
        return None
    dev = shards[0].device
    store = TORCH_DTYPE[g.store_dtype]
    accept = _ROW_SOURCES.get(store, {store: na.SRC_F64})
    segs = [s for s in g.segments if s.numel > 0]
    w0 = w_local_lst[0]
    dts = tuple(getattr(w0[s.key], "dtype", None) for s in segs)
    if any(d not in accept for d in dts):
        return None
    src = [accept[d] for d in dts]
    ptrs = np.empty((len(segs), plan.n_clients), dtype=np.int64)
    L = na.load_torchmeta()
    if L is not None and _plain_dicts(w_local_lst):  # TensorImpl reads (csrc/fa_torchmeta.cpp)
        keep = [None] * (len(segs) * plan.n_clients)
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        if L.fa_tm_tensor_ptrs(_as_list(w_local_lst), tuple(s.key for s in segs), dts, index, ptrs.ctypes.data,
                               keep) == 0:
            return segs, ptrs, keep, src
    keep = []
    for j, s in enumerate(segs):
        row = ptrs[j]
        for n, w in enumerate(w_local_lst):
            t = w[s.key]
            if t.dtype != dts[j] or t.device != dev or not t.is_contiguous():
                return None
            row[n] = t.data_ptr()
            keep.append(t)
    return segs, ptrs, keep, src


class RowTable:
    """Device-resident uploads read where they lie (flearn's run2 path hands the server torch
    tensors, flearn/server/Communicator.py:287-292): a device table of per-(key, client) tensor
    pointers, [segments][clients], plus the bucket's piece table (fa_rows_plan, cached on the
    plan).  fa_reduce_f32_rows reads every upload once in one launch, with no pack copy; the
    8-byte kinds (BN counters) and unaligned fp32 tensors take one fa_gather_rows launch into a
    device stack instead of N*K copy kernels.  `shape` = (clients, stride) like a stack.

    The tensors are referenced until the launches that read them have completed (an event
    recorded after them is checked at the next use of the packer), so the caching allocator
    cannot hand their memory to another stream meanwhile."""

    def __init__(self, packer, plan: BucketPlan, g: Group, segs, ptrs: np.ndarray, keep, src, device):
        self.packer, self.plan, self.group, self.segs = packer, plan, g, segs
        self.src = tuple(src) if src is not None else (na.SRC_F64,) * len(segs)  # per segment
        self.converts = any(k != na.SRC_F64 for k in self.src)  # some segment is not the store dtype
        self.device = torch.device(device)
        self.shape = (plan.n_clients, g.stride)
        self.aligned = bool(ptrs.size == 0 or not (ptrs % 16).any())
        self.elem_size = np.dtype(g.store_dtype).itemsize
        # the pointer table: reused pinned staging (waited on before it is rewritten), then H2D
        key = ("rows", g.kind, str(self.device))
        host = packer._staging(key, (max(ptrs.size, 1),), torch.int64)
        host[: ptrs.size].numpy()[:] = ptrs.reshape(-1)
        self.ptrs = packer.device_bucket(key, (max(ptrs.size, 1),), torch.int64, self.device)
        self.ptrs.copy_(host, non_blocking=True)
        packer._staging_used(key, self.device)
        self.keep = keep
        self.work = packer.device_bucket(("rows_work", str(self.device)), (1,), torch.int32, self.device)

    def piece_table(self, op: int):
        """(device fa_piece array, slot count, grid) for this bucket layout and epilogue, cached
        on the plan."""
        mk = ("row_pieces", self.group.kind, int(op), str(self.device))
        hit = self.plan.memo.get(mk)
        if hit is None:
            L = na.load()
            cols = np.array([s.offset for s in self.segs], dtype=np.int64)
            lens = np.array([s.numel for s in self.segs], dtype=np.int64)
            cnt, grid = ctypes.c_int64(), ctypes.c_int32()
            with torch.cuda.device(self.device):  # the default grid follows this device's CUs
                na.check(L.fa_rows_plan(len(self.segs), cols.ctypes.data, lens.ctypes.data, int(op), 0, None, 0,
                                        ctypes.byref(cnt), ctypes.byref(grid)), "fa_rows_plan")
                arr = np.zeros((max(cnt.value, 1), ctypes.sizeof(na.Piece)), dtype=np.uint8)
                na.check(L.fa_rows_plan(len(self.segs), cols.ctypes.data, lens.ctypes.data, int(op), grid.value,
                                        arr.ctypes.data, cnt.value, ctypes.byref(cnt), ctypes.byref(grid)),
                         "fa_rows_plan")
            dev = torch.from_numpy(arr.reshape(-1)).to(self.device)  # once per layout
            hit = self.plan.memo[mk] = (dev, cnt.value, grid.value)
        return hit

    def gather_into(self, stack: torch.Tensor) -> None:
        """One launch: every (key, client) tensor into its segment of the device stack [N, stride]
        (converted to float64 per segment when the float64 group holds int64 / float32 values)."""
        L = na.load()
        mk = ("row_segs", self.group.kind, str(self.device), self.src)
        segs = self.plan.memo.get(mk)
        if segs is None:
            cols = [s.offset for s in self.segs] + [s.numel for s in self.segs]
            t = np.array(cols + (list(self.src) if self.converts else []), dtype=np.int64)
            segs = self.plan.memo[mk] = torch.from_numpy(t).to(self.device)
        # (float16 uploads are gathered, then reduced by fa_reduce_f16; the plain gather takes the element size)
        fn = "fa_gather_rows_f64" if self.converts else "fa_gather_rows_f16" if self.elem_size == 2 else "fa_gather_rows"
        size = (self.elem_size,) if fn == "fa_gather_rows" else ()
        na.check(getattr(L, fn)(stack.data_ptr(), stack.stride(0), self.shape[0], *size, self.ptrs.data_ptr(),
                                segs.data_ptr(), len(self.segs), na.stream_handle(self.device)), fn)
        self.release()

    def release(self) -> None:
        """Call after the launches that read the uploads are queued: the packer keeps them alive
        until those launches have completed."""
        self.packer.hold(self.keep, self.device)
        self.keep = []
