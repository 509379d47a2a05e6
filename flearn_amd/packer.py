"""Host<->device packing of client state_dicts into a plan's buckets (bucketplan.py): the native
pack calls with their table builders (AsyncPack, NativeRows) and the Packer that owns the staging."""
from __future__ import annotations

import collections
import concurrent.futures
import ctypes
import math
import os

import numpy as np
import torch

from . import _native as na
from .bucketplan import (_NP, FMT, SMALL_BYTES, TORCH_DTYPE, BucketPlan, Group, Piece, Shard, _as_list, _plain_dicts,
                         rank_width, split_columns)
from .rowtable import RowTable, row_ptrs, slab_stack
from .semantics import KIND_F32
from .wire import wire_device_stack, wire_row


def piece_columns(pieces, stagings) -> tuple:
    """(source, base, pitch, offset) of pieces as int64 columns, in bytes.  source: what both native
    tables take of a piece's value, by parameter name (value_bytes, fmt, first_byte, nbytes); then its
    destination: its shard's staging (`stagings`: _host_rows) and its offset within a row."""
    t = np.array([(p.segment.src_dtype.itemsize, p.segment.numel, FMT[p.segment.src_dtype], p.src_lo,
                   p.src_hi - p.src_lo, *stagings[p.shard.index], p.dst_lo) for p in pieces],
                 dtype=np.int64).reshape(-1, 8).T
    item = t[0]
    return dict(value_bytes=t[1] * item, fmt=t[2], first_byte=t[3] * item, nbytes=t[4] * item), t[5], t[6], t[7] * item


def _host_rows(hosts) -> tuple:
    """(address, row bytes) of every shard's staging; (0, 0) where there is none."""
    return tuple((h.data_ptr(), h.stride(0) * h.element_size()) if h is not None else (0, 0) for h in hosts)


def pack_threads() -> int:
    """Threads of a host-copy pool: as many as the process may use, from 4 up to 16."""
    try:
        cpus = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cpus = os.cpu_count() or 8
    return max(4, min(16, cpus))


class AsyncPack:
    """Host copies run by native threads (csrc/fa_pyhost.c fa_py_pack_start / fa_pack_wait /
    fa_py_pack_end): `rows` is an int64 table, one row per piece, of the columns `table` names.
    `start(dicts)` checks every value against the table under the GIL (all or nothing: None
    when a value is off the plan, nothing copied) and queues the copies in chunk order as jobs
    of SPLIT bytes; `wait(h, j)` returns (the GIL released) once chunk j's bytes are in, the
    waiting thread copying jobs of chunks <= j itself; `end(h)` waits for everything and drops
    the values.  No interpreter work per job: the Python pool's per-part GIL hand-offs kept the
    first chunk 0.5-0.9 ms from its launch in the client update."""

    SPLIT = 512 << 10  # bytes per native copy job

    def __init__(self, keys: tuple, rows: np.ndarray, nchunks: int, threads: int = 0):
        self.keys = keys
        self.desc = np.ascontiguousarray(rows.T).reshape(-1)
        self.nchunks = nchunks
        self.L = na.load_pyhost()
        self.threads = threads if threads > 0 else pack_threads()

    @staticmethod
    def table(*, src, value_bytes, fmt, dst, chunk, first_byte, nbytes) -> np.ndarray:
        """The [jobs, 7] int64 table `rows`, row i copying keys[i]: index of the source dict, the
        value's size in bytes, its format class (FMT), the destination address, the chunk, the first
        byte and the byte count copied.  Scalars and arrays broadcast; rows come out in C order."""
        cols = np.broadcast_arrays(src, value_bytes, fmt, dst, chunk, first_byte, nbytes)
        return np.stack(cols, axis=-1).astype(np.int64, copy=False).reshape(-1, 7)

    def start(self, dicts):
        st = ctypes.c_int32(0)
        h = self.L.fa_py_pack_start(dicts, self.keys, len(self.keys), self.desc.ctypes.data, self.nchunks,
                                    self.SPLIT, self.threads, ctypes.byref(st))
        if not h and st.value == 2:
            raise MemoryError("fa_py_pack_start: out of host memory")
        return h or None

    def wait(self, h, j: int) -> None:
        if self.L.fa_pack_wait(h, j) != 0:
            raise RuntimeError(f"fa_pack_wait({j}) failed")

    def end(self, h) -> None:
        self.L.fa_py_pack_end(h)


class NativeRows:
    """Packs client rows through fa_py_pack_rows (csrc/fa_pyhost.c): one native call walks the
    clients' dicts and copies every piece into the pinned staging, the GIL released around the
    copies.  Built per pack call from the plan's pieces; `__call__(lo, hi)` returns False when a
    value is not a plain C-contiguous array of its planned dtype (torch tensors, views of other
    layouts...), and the caller then packs those rows from Python."""

    def __init__(self, pieces, hosts, w_local_lst, rows, memo=None):
        self.fn = na.load_pyhost().fa_py_pack_rows
        # plain dicts only (dict / OrderedDict, whose item lookup the C side reproduces)
        self.clients = [w if type(w) in (dict, collections.OrderedDict) else None for w in w_local_lst]
        hp = _host_rows(hosts)
        # keyed by the pieces list (memoized on the plan: one object per kind and shard layout)
        # AND the staging addresses: two kinds' stagings of different packers can occupy the same
        # pinned block in turn (the host caching allocator hands a freed block out again), and a
        # table keyed by addresses alone then packed one kind's keys into the other's stack
        key = ("native_rows", id(pieces), hp)
        memo = {} if memo is None else memo
        cached = memo.get(key)
        if cached is None:
            source, base, pitch, off = piece_columns(pieces, hp)
            cached = memo[key] = (tuple(p.segment.key for p in pieces),
                                  self.table(dst_base=base, dst_row=pitch, dst_off=off, **source))
        self.keys, table = cached
        # ... then one skip flag per client row
        self.desc = np.concatenate([table, np.fromiter((r is not None for r in rows), dtype=np.int64, count=len(rows))])
        self.ptr = self.desc.ctypes.data

    @staticmethod
    def table(*, value_bytes, first_byte, nbytes, fmt, dst_base, dst_row, dst_off) -> np.ndarray:
        """What fa_py_pack_rows reads before its skip flags (one per client row): seven blocks of one
        int64 per key — the value's bytes, the first byte and byte count copied, the format class
        (FMT), the destination's address, row pitch (client r: row r) and offset.  Scalars broadcast."""
        return np.concatenate(np.broadcast_arrays(value_bytes, first_byte, nbytes, fmt, dst_base, dst_row, dst_off),
                              dtype=np.int64)

    @staticmethod
    def usable(pieces, hosts) -> bool:
        """Byte copies only: every source dtype is its bucket's storage dtype."""
        return bool(pieces) and all(
            h is not None and p.segment.src_dtype in FMT and np.dtype(_NP[h.dtype]) == p.segment.src_dtype
            for p in pieces for h in (hosts[p.shard.index],))

    def __call__(self, lo: int, hi: int) -> bool:
        return self.fn(self.clients, self.keys, len(self.keys), self.ptr, lo, hi) == 0


class Packer:
    """Owns reusable pinned staging and device buckets; packs uploads, unpacks results.

    The f32 bucket is split by columns over `devices` (one Shard each): every device receives
    its columns of every client through its own PCIe link, reduces them, and sends its slice of
    the global model back — per-GPU parallel H2D/D2H.  With one device this is the plain path."""

    def __init__(self, devices, workers: int = 8):
        self.devices = [torch.device(d) for d in devices]
        self.device = self.devices[0]
        self.workers = workers
        self._pinned = {}
        self._pin_events = {}  # pinned staging key -> event after its last queued H2D
        self._dev = {}
        self._shards = {}
        self._pool = None
        self._held = []  # (event, uploads read by launches queued before it): see hold()
        self.last_wire_rows = 0
        self.last_wire_staged = 0
        self.last_row_tables = {}  # kind -> "slab" | "rows" | "gather" | "copy" for device-resident uploads
        #: device uploads carved from one allocation laid out as the bucket run as a stack
        #: (_slab_stack); False: always the pointer table (tools/rows_pmc.py measures that kernel)
        self.use_slabs = True
        self.rank_cols = None  # (rank, world): pack only this rank's columns of the f32 bucket
        #: host uploads packed by native threads in growing row chunks (AsyncPack); False: the
        #: Python pool packs ~8 equal chunks (also the fallback for values off the plan)
        self.native_async = True
        self.async_lookahead = 0  # chunks packed ahead of the DMA (0: all queued at once)
        self.async_threads = 0  # native pack threads (0: AsyncPack's default, <= 16)
        # kind -> how its last host pack ran: "serial" | "async" | "mixed" (some chunks packed
        # from Python: values off the plan) | "pool"
        self.last_pack_paths = {}
        #: one device: results stored into fresh pinned buffers by fa_copy kernels (zero-copy
        #: writes) and handed out as views; False: copy-engine D2H into staging + host copy into
        #: pageable memory.  The pinned buffers come from torch's pinned caching allocator, which
        #: keeps freed pages locked for reuse: a server that retains many rounds' w_glob (history,
        #: checkpoints) pins one model per retained round — set False there
        self.zero_copy_out = True

    def _executor(self) -> concurrent.futures.ThreadPoolExecutor:
        """One persistent pool per Packer: creating threads per call costs ~0.3 ms, which is the
        whole budget of a LeNet-sized round."""
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(self.workers, thread_name_prefix="fa-pack")
        return self._pool

    def _buf(self, cache, key, shape, dtype, **kw):
        t = cache.get(key)
        if t is None or t.numel() < math.prod(shape) or t.dtype != dtype:
            cache.pop(key, None)
            t = torch.zeros(math.prod(shape), dtype=dtype, **kw)
            cache[key] = t
        return t[: math.prod(shape)].view(shape)

    def _staging(self, key, shape, dtype):
        """Reusable pinned staging to rewrite, once the H2D queued from it last (_staging_used) is done."""
        ev = self._pin_events.pop(key, None)
        if ev is not None:
            ev.synchronize()
        return self._buf(self._pinned, key, shape, dtype, pin_memory=True)

    def _staging_used(self, key, device) -> None:  # its H2D copies are queued on device's current stream
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._pin_events[key] = ev

    def hold(self, objs, device) -> None:
        """Keep `objs` (uploads read by queued launches) alive until the work queued so far on
        `device`'s current stream is done; earlier holds whose events completed are dropped."""
        self._held = [(e, o) for e, o in self._held if not e.query()]
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._held.append((ev, objs))

    def hold_slab(self, kind: str, stacks, device) -> None:
        """`hold` the stacks of `kind` when its last pack was a slab: the caller's memory, read in
        place by the launches queued so far, stays alive until they have read it."""
        if self.last_row_tables.get(kind) == "slab":
            self.hold(list(stacks), device)

    def dense_stack(self, plan: BucketPlan, kind: str, parts, n: int) -> tuple:
        """(shard, [n, stride] device tensor) of what `pack` returned for one unsharded bucket: a
        RowTable (device uploads) is gathered, in one launch, into the bucket's input stack; a
        stack comes back as packed."""
        ((sh, stack),) = parts
        if isinstance(stack, RowTable):
            g = plan.groups[kind]
            with torch.cuda.device(sh.device):
                buf = self.device_bucket(("in", kind, sh.index), (n, g.stride), TORCH_DTYPE[g.store_dtype], sh.device)
                stack.gather_into(buf)
            stack = buf
        return sh, stack

    def device_bucket(self, tag, shape, dtype, device=None):
        """A reusable device buffer (contents undefined)."""
        dev = self.device if device is None else torch.device(device)
        return self._buf(self._dev, (tag, str(dev)), shape, dtype, device=dev)

    def shards(self, plan: BucketPlan, kind: str) -> list:
        g = plan.groups[kind]
        if kind != KIND_F32:
            return [Shard(0, self.device, 0, g.stride)]
        key = (g.stride, tuple(str(d) for d in self.devices), self.rank_cols)
        if key not in self._shards:
            if self.rank_cols is not None:  # one rank of a column-sharded process group
                rank, world = self.rank_cols
                w = rank_width(g.stride, world)
                c0 = min(rank * w, g.stride)
                self._shards[key] = [Shard(0, self.device, c0, min(c0 + w, g.stride))]
            else:
                self._shards[key] = split_columns(g.stride, self.devices)
        return self._shards[key]

    @staticmethod
    def _pieces(g: Group, shards) -> list:
        """Each key segment cut at shard boundaries, as Pieces."""
        out = []
        for s in g.segments:
            lo, hi = s.offset, s.offset + s.numel
            for sh in shards:
                a, b = max(lo, sh.c0), min(hi, sh.c1)
                if a < b:
                    out.append(Piece(s, a - lo, b - lo, sh, a - sh.c0))
        return out

    def pack(self, plan: BucketPlan, w_local_lst) -> dict:
        """Copy every client's selected tensors into the device buckets.
        Returns kind -> [(shard, device stack [N, shard.width])]."""
        out = {}
        self.last_wire_staged = 0
        self.last_row_tables = {}
        self.last_pack_paths = {}
        for kind, g in plan.groups.items():
            shards = self.shards(plan, kind)
            devs = [self.device_bucket(("in", kind, sh.index), (plan.n_clients, sh.width), TORCH_DTYPE[g.store_dtype],
                                       sh.device) for sh in shards]
            pk = ("pieces", kind, tuple((sh.index, sh.c0, sh.c1) for sh in shards))
            pieces = plan.memo.get(pk)
            if pieces is None:
                pieces = plan.memo[pk] = self._pieces(g, shards)
            on_device = plan.input_kind == "torch" and all(
                w_local_lst[0][s.key].device.type == "cuda" for s in g.segments)
            pack = self._pack_device if on_device else self._pack_host
            out[kind] = pack(plan, g, shards, devs, pieces, w_local_lst)
        return out

    def _pack_device(self, plan: BucketPlan, g: Group, shards, devs, pieces, w_local_lst) -> list:
        """Device uploads of one kind: read in place (slab, aligned fp32 rows), else gathered or copied."""
        kind = g.kind
        rp = row_ptrs(plan, g, w_local_lst, shards)  # None unless one shard holds the whole bucket
        if rp is None:  # column shards over several devices, or values no table takes: per-piece copies
            self.last_row_tables[kind] = "copy"
            for n, w in enumerate(w_local_lst):
                for seg, lo, hi, sh, dst in pieces:
                    devs[sh.index][n, dst : dst + (hi - lo)].copy_(w[seg.key].reshape(-1)[lo:hi])
            return list(zip(shards, devs))
        if kind == KIND_F32 and self.use_slabs:
            slab = slab_stack(plan, g, w_local_lst, rp)
            if slab is not None:  # one allocation laid out as the bucket: the stack itself
                self.last_row_tables[kind] = "slab"
                return [(shards[0], slab)]
        table = RowTable(self, plan, g, *rp, shards[0].device)
        if kind == KIND_F32 and table.aligned:
            self.last_row_tables[kind] = "rows"
            return [(shards[0], table)]  # read in place by fa_reduce_f32_rows
        table.gather_into(devs[0])  # one launch for the whole bucket
        self.last_row_tables[kind] = "gather"
        return list(zip(shards, devs))

    def _pack_host(self, plan: BucketPlan, g: Group, shards, devs, pieces, w_local_lst) -> list:
        """Host uploads of one kind: the device copy staged at wire decode when there is one, else
        packed into pinned staging (rows the wire codec already pinned excepted) and DMA'd."""
        kind, n = g.kind, plan.n_clients
        rows = self._wire_rows(g, w_local_lst) if kind == KIND_F32 else [None] * n
        wired = all(r is not None for r in rows)  # every row already sits in pinned memory
        if wired and len(shards) == 1:
            staged = wire_device_stack(w_local_lst, g.row_layout, shards[0].device)
            if staged is not None:  # uploads already copied to the device at decode time
                self.last_wire_staged = n
                return [(shards[0], staged)]
        hkeys = [] if wired else [("in", kind, sh.index) for sh in shards]
        hosts = ([None] * len(shards) if wired else
                 [self._staging(hk, (n, sh.width), TORCH_DTYPE[g.store_dtype]) for hk, sh in zip(hkeys, shards)])
        self.last_pack_paths[kind] = self._pack_pipelined(plan, pieces, w_local_lst, shards, hosts, devs, rows)
        for hk, sh in zip(hkeys, shards):
            self._staging_used(hk, sh.device)
        return list(zip(shards, devs))

    def row_table(self, plan: BucketPlan, g: Group, w_local_lst, shards):
        """RowTable of device-resident uploads for bucket group g, or None (rowtable.row_ptrs)."""
        rp = row_ptrs(plan, g, w_local_lst, shards)
        return None if rp is None else RowTable(self, plan, g, *rp, shards[0].device)

    _slab_stack = staticmethod(slab_stack)

    def _wire_rows(self, g: Group, w_local_lst) -> list:
        """Per client: the pinned row the wire codec decoded its fp32 params into, when that row
        is laid out exactly as this bucket (flearn_amd.wire.decode) — else None."""
        rows = [wire_row(w, g.row_layout) for w in w_local_lst]
        self.last_wire_rows = sum(r is not None for r in rows)
        return rows

    def _pack_pipelined(self, plan: BucketPlan, pieces, w_local_lst, shards, hosts, devs, rows):
        """Host ingest: client rows are packed into pinned staging by a thread pool, chunk by
        chunk, and each finished chunk's H2D copies (one per shard, on that device's stream) are
        queued at once, so the DMA of chunk k runs while the CPU packs chunk k+1 (flearn's
        uploads are pageable host arrays: they must be copied once into pinned memory before a
        DMA engine can read them).  Clients whose fp32 params the wire codec decoded straight
        into a pinned row of this layout (`rows[n]`) skip the pack and are DMA'd from there."""
        host_np = [h.numpy() if h is not None else None for h in hosts]
        native = (NativeRows(pieces, hosts, w_local_lst, rows, plan.memo)
                  if NativeRows.usable(pieces, hosts) else None)

        def fill(n):
            if rows[n] is not None:
                return
            w = w_local_lst[n]
            cache = {}
            for seg, lo, hi, sh, dst in pieces:  # (a Piece, whole: this loop runs per client and piece)
                src = cache.get(seg.key)
                if src is None:
                    v = w[seg.key]
                    if isinstance(v, torch.Tensor):
                        v = v.detach().cpu().numpy()
                    src = cache[seg.key] = np.asarray(v).reshape(-1)
                host_np[sh.index][n, dst : dst + (hi - lo)] = src[lo:hi]

        def fill_rows(lo, hi):
            if native is None or not native(lo, hi):
                for r in range(lo, hi):
                    fill(r)

        def ship(lo, hi):
            for sh, h, dv in zip(shards, hosts, devs):
                with torch.cuda.device(sh.device):
                    r = lo
                    while r < hi:
                        if rows[r] is not None:
                            dv[r].copy_(rows[r][sh.c0 : sh.c1], non_blocking=True)
                            r += 1
                            continue
                        e = r
                        while e < hi and rows[e] is None:
                            e += 1
                        dv[r:e].copy_(h[r:e], non_blocking=True)
                        r = e

        n = plan.n_clients
        workers = max(1, min(self.workers, n))
        nbytes = sum(int(d.numel()) * d.element_size() for d in devs)
        if workers == 1 or nbytes < SMALL_BYTES or all(r is not None for r in rows):
            fill_rows(0, n)
            ship(0, n)
            return "serial"
        if self.native_async and native is not None and _plain_dicts(w_local_lst):
            aps, bounds = self._async_rows(plan, pieces, hosts, rows)
            lst = _as_list(w_local_lst)
            ahead = len(aps) if self.async_lookahead <= 0 else self.async_lookahead
            started = collections.deque()  # (chunk, handle or None: that chunk packs in Python)
            path = "async"
            try:
                for j in range(min(ahead, len(aps))):
                    started.append((j, aps[j].start(lst)))
                for j, (lo, hi) in enumerate(bounds):
                    _, h = started[0]
                    if h is None:  # a value off the plan in this chunk: the NativeRows / Python pack
                        fill_rows(lo, hi)
                        path = "mixed"
                    else:
                        aps[j].wait(h, 0)
                        aps[j].end(h)
                    started.popleft()  # only once its copies are done (the finally ends the rest)
                    ship(lo, hi)
                    if j + ahead < len(aps):
                        started.append((j + ahead, aps[j + ahead].start(lst)))
            finally:
                for j, h in started:  # only after an error: no copy may outlive the call
                    if h is not None:
                        aps[j].end(h)
            return path
        chunk = max(workers, -(-n // 8))  # ~8 chunks, at least one row per worker
        ex = self._executor()
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            list(ex.map(lambda r: fill_rows(r, r + 1), range(lo, hi)))
            ship(lo, hi)
        return "pool"

    def _async_rows(self, plan: BucketPlan, pieces, hosts, rows):
        """([AsyncPack per chunk], [(lo, hi)]): chunks of rows that grow 1, 2, 4, ... up to
        ~n/12 (the first DMA starts after one row is packed, ~0.5 ms for ResNet-18, where ~8
        equal chunks of a pool pack held it back by a whole chunk); each chunk's packed rows'
        pieces in row order.  Cached on the plan per staging address and wire-row pattern."""
        n = plan.n_clients
        skip = tuple(r is not None for r in rows)
        hp = _host_rows(hosts)
        key = ("async_rows", id(pieces), hp, skip, self.async_threads)
        hit = plan.memo.get(key)
        if hit is not None:
            return hit
        cap = max(1, -(-n // 12))
        bounds, lo, size = [], 0, 1
        while lo < n:
            hi = min(n, lo + size)
            bounds.append((lo, hi))
            lo, size = hi, min(cap, size * 2)
        source, base, pitch, off = piece_columns(pieces, hp)
        pkeys = tuple(p.segment.key for p in pieces)
        aps = []
        for lo, hi in bounds:
            r = np.array([i for i in range(lo, hi) if not skip[i]], dtype=np.int64)[:, None]
            table = AsyncPack.table(src=r, dst=base + off + r * pitch, chunk=0, **source)
            aps.append(AsyncPack(pkeys * len(r), table, 1, threads=self.async_threads))
        out = plan.memo[key] = (aps, bounds)
        return out

    def unpack(self, plan: BucketPlan, results: dict, as_torch: bool, out_dtype_override=None) -> dict:
        """results: kind -> [(shard, device tensor [shard.width])].  Returns {key: fresh value} in
        plan order with the reference's types: ndarray (numpy scalar for 0-d keys) or torch CPU
        tensor, views of ONE freshly allocated buffer per kind — nothing returned is shared with
        staging or with later calls."""
        if self.zero_copy_out and len({sh.device for parts in results.values() for sh, _ in parts}) == 1:
            fresh = self._unpack_zero_copy(plan, results)
        else:
            fresh = self._unpack_staged(plan, results)
        glob = {}
        for k in plan.keys:
            kind = plan.key_group[k]
            s = plan.key_segment[k]
            arr = fresh[kind][s.offset : s.offset + s.numel].reshape(s.shape)
            if out_dtype_override is not None:
                arr = arr.astype(out_dtype_override, copy=False)
            if as_torch:
                glob[k] = torch.from_numpy(arr)
            elif s.shape == ():
                glob[k] = arr.dtype.type(arr[()])  # numpy returns scalars for 0-d math
            else:
                glob[k] = arr
        return glob

    def _unpack_zero_copy(self, plan: BucketPlan, results: dict) -> dict:
        """One device: fa_copy kernels store each result straight into a fresh pinned buffer per
        kind over PCIe (~53 GB/s; the copy engine's D2H ran at ~30 GB/s)
        and the values handed out are views of it — no staging, no host copy.  The buffer comes
        from torch's pinned caching allocator and goes back to it when the views die (it stays
        page-locked in torch's cache: `zero_copy_out`)."""
        L = na.lib()
        fresh, dev = {}, None
        for kind, parts in results.items():
            buf = torch.empty(plan.groups[kind].stride, dtype=parts[0][1].dtype, pin_memory=True)
            for sh, t in parts:
                dev = sh.device
                src = t[: sh.width]
                dst = buf[sh.c0 : sh.c0 + sh.width]
                with torch.cuda.device(sh.device):
                    rc = -2
                    if src.is_contiguous() and src.is_cuda:
                        rc = L.fa_copy(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(),
                                       torch.cuda.current_stream(sh.device).cuda_stream)
                    if rc == na.FA_ERR_ALIGN:
                        dst.copy_(src, non_blocking=True)
                    else:
                        na.check(rc, "fa_copy")
            fresh[kind] = buf.numpy()
        if dev is not None:
            torch.cuda.current_stream(dev).synchronize()
        return fresh

    def _unpack_staged(self, plan: BucketPlan, results: dict) -> dict:
        """Each shard's D2H goes to reusable pinned staging on its device's stream (all links in
        parallel); the slices are then copied, by a thread pool, into ONE freshly allocated buffer
        per kind."""
        staged = []
        for kind, parts in results.items():
            for sh, t in parts:
                h = self._buf(self._pinned, ("out", kind, sh.index, t.dtype), (sh.width,), t.dtype, pin_memory=True)
                with torch.cuda.device(sh.device):
                    h.copy_(t[: sh.width], non_blocking=True)
                staged.append((kind, sh, h))
        for d in {sh.device for _, sh, _ in staged}:
            torch.cuda.current_stream(d).synchronize()
        fresh = {kind: np.empty(plan.groups[kind].stride, dtype=_NP[parts[0][1].dtype])
                 for kind, parts in results.items()}
        step = 1 << 22  # 4M elements per copy task
        tasks = []
        for kind, sh, h in staged:
            src = h.numpy()
            for lo in range(0, sh.width, step):
                hi = min(sh.width, lo + step)
                tasks.append((fresh[kind], sh.c0 + lo, src, lo, hi))

        def copy(t):
            dst, d0, src, lo, hi = t
            np.copyto(dst[d0 : d0 + (hi - lo)], src[lo:hi])

        nbytes = sum(int(h.numel()) * h.element_size() for _, _, h in staged)
        if len(tasks) > 1 and self.workers > 1 and nbytes >= SMALL_BYTES:
            list(self._executor().map(copy, tasks))
        else:
            for t in tasks:
                copy(t)
        return fresh
