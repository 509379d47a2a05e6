"""The one-shot push transport of the multi-GPU aggregation (flearn_amd.dist.ShardedReducer's `push=`): exportable
buckets (`DeviceBuffer`), their collective mapping and token check (`_map_peers`), the pool that keeps them mapped
from job to job (`_RecvPool`, `shutdown_push`) and one job's pushes (`PushGather`).  Invariants: DESIGN.md §6.
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass

import torch
import torch.distributed as dist

from . import _native as na
from .shardplan import round_up
from .streams import side_stream

MAX_PUSH_RANKS = 8  # fa_push's destination count: one MI355X node

#: how a push is ordered after its stripe's reduce: "host" (the host waits for the reduce, then
#: issues the push with no device-side cross-stream wait), "producer" (the push's streams wait on
#: an event of the reduce's stream) or "chain" (round 5: an event of the pusher's stream after its
#: wait on the reduce's).  "auto", the product's: the copy-engine push in host order — with
#: device-side waits its legs (and its own-copy kernel) started before the reduce had finished,
#: 1-30% of rank-steps among eight processes on one GPU — and the kernel push in producer order:
#: never wrong in the same probes (0 of 6,656 rank-steps, tests/push_order_probe.py), and host
#: order costs it a host round trip per stripe (100 x 3.2 M columns, a rank's share of NS at G = 8,
#: 4 stripes: 0.32-0.40 ms per step against 0.275)
_PUSH_ORDER = "auto"


def push_order(mode: str) -> str:
    """The order a PushGather of `mode` uses now (_PUSH_ORDER resolved)."""
    if _PUSH_ORDER != "auto":
        return _PUSH_ORDER
    return "producer" if mode == "kernel" else "host"


def peer_stream(device) -> torch.cuda.Stream:
    """A copy-engine leg's stream (normal priority; tests/push_order_probe.py overrides it)."""
    return torch.cuda.Stream(device)


@dataclass(frozen=True)
class PeerContext:
    """What the transport's collectives need to know of their ranks: the process group, its size, this rank, whether
    it is RCCL (flags are all-reduced on `device` then, on the host on gloo)."""

    group: object
    world: int
    rank: int
    nccl: bool
    device: torch.device

    @staticmethod
    def of(group, device) -> "PeerContext":
        return PeerContext(group, dist.get_world_size(group), dist.get_rank(group),
                           dist.get_backend(group) == "nccl", torch.device(device))


#: exported buckets released by their users, handed out again by DeviceBuffer.get (see
#: DeviceBuffer); per device they are kept within PARK_CAP x the largest bucket the device has
#: exported — beyond that the smallest are freed
_PARKED: list = []
PARK_CAP = 2
_LARGEST: dict = {}  # device -> bytes of the largest bucket it has exported
_TRIMMED = [0, 0]  # exported buckets freed to keep within the cap: (count, bytes)


def size_class(nbytes: int) -> int:
    """Bucket sizes come in four classes per octave (2^k, 1.25, 1.5, 1.75 x 2^k; at least 4 KiB): requests a few
    percent apart share one class, so released buckets fit the next job's."""
    nbytes = max(int(nbytes), 4096)
    return round_up(nbytes, 1 << max(nbytes.bit_length() - 3, 0))


class DeviceBuffer:
    """A device allocation of its own (C ABI fa_dev_alloc), outside torch's caching allocator: what the push gather
    exports.  A caching-allocator tensor lives inside a segment that other tensors share and that torch recycles
    (empty_cache frees it), and hipIpcGetMemHandle exports the whole segment; this is one bucket, one export.

    Once exported (`exported`), `free()` parks a bucket and `DeviceBuffer.get` hands it out again (re-exporting the
    same memory).  With several processes on one GPU, an exporter that freed imported memory and exported again made
    13-34% of later imports map the wrong allocation; with nothing exported freed, and a barrier after every unmap, 0
    of 1,920 imports were wrong (profiles/r05/ipc/).  Parking is bounded: per device the parked
    bytes stay within PARK_CAP x the largest bucket the device has exported, the smallest parked buckets beyond that
    are freed (`trimmed()` counts them) — a later import that maps the wrong allocation is still refused by the token
    check of every mapping (_map_peers), so the cost of a trim is at worst a refused push set-up (RCCL's all-gather
    then), never a wrong bucket.  `tensor()` views it (torch keeps this object alive while any view does); an
    unexported buffer is freed by `free()` or when the last view dies."""

    def __init__(self, nbytes: int, device):
        self.L, self.na = na.lib(), na
        self.nbytes, self.device = int(nbytes), torch.device(device)
        self._exported = False
        self._typestr = "<f4"
        self.ptr = self._alloc()

    def _alloc(self) -> int:
        p = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self.na.check(self.L.fa_dev_alloc(self.nbytes, ctypes.byref(p)), "fa_dev_alloc")
        return p.value

    def _release(self, ptr: int):
        with torch.cuda.device(self.device):
            self.na.check(self.L.fa_dev_free(ptr), "fa_dev_free")

    @property
    def exported(self) -> bool:
        """Set when peers may map it: from then on free() parks it."""
        return self._exported

    @exported.setter
    def exported(self, value: bool):
        if value and not self._exported:
            key = str(self.device)
            _LARGEST[key] = max(_LARGEST.get(key, 0), self.nbytes)
        self._exported = bool(value)

    @classmethod
    def get(cls, nbytes: int, device) -> "DeviceBuffer":
        """A parked (previously exported, released) buffer of at least nbytes on `device` — the smallest that fits —
        or a new one of nbytes' size class."""
        dev = torch.device(device)
        fits = [b for b in _PARKED if b.device == dev and b.nbytes >= nbytes]
        if fits:
            b = min(fits, key=lambda x: x.nbytes)
            _PARKED.remove(b)
            return b
        return cls(size_class(nbytes), dev)

    @staticmethod
    def parked_bytes(device=None) -> int:
        return sum(b.nbytes for b in _PARKED if device is None or b.device == torch.device(device))

    @staticmethod
    def park_cap(device) -> int:
        return PARK_CAP * _LARGEST.get(str(torch.device(device)), 0)

    @staticmethod
    def trimmed() -> dict:
        return {"buckets": _TRIMMED[0], "bytes": _TRIMMED[1]}

    @staticmethod
    def _trim(device):
        """Free the smallest parked buckets of `device` until the parked bytes fit the cap."""
        cap = DeviceBuffer.park_cap(device)
        parked = sorted((b for b in _PARKED if b.device == device), key=lambda b: b.nbytes)
        total = sum(b.nbytes for b in parked)
        for b in parked:
            if total <= cap:
                break
            _PARKED.remove(b)
            total -= b.nbytes
            ptr, b.ptr = b.ptr, None
            b._release(ptr)
            _TRIMMED[0] += 1
            _TRIMMED[1] += b.nbytes

    @property
    def __cuda_array_interface__(self):
        if not self.ptr:
            raise RuntimeError("DeviceBuffer already freed")
        item = int(self._typestr[-1])
        return {"shape": (self.nbytes // item,), "typestr": self._typestr, "data": (self.ptr, False),
                "version": 2, "strides": None}

    def tensor(self, dtype=torch.float32) -> torch.Tensor:
        """A 1-D view of the whole buffer (float32 or int32)."""
        self._typestr = {torch.float32: "<f4", torch.int32: "<i4"}[dtype]
        t = torch.as_tensor(self, device=self.device)
        if t.data_ptr() != self.ptr or t.device != self.device:
            raise RuntimeError("DeviceBuffer view does not alias its allocation")
        return t

    def free(self):
        """Release: an exported buffer is parked for reuse (freed only beyond the parking cap), any other freed."""
        if not self.ptr:
            return
        if self.exported:
            if self not in _PARKED:
                _PARKED.append(self)
                DeviceBuffer._trim(self.device)
            return
        ptr, self.ptr = self.ptr, None
        self._release(ptr)

    def __del__(self):
        try:
            if not self.exported:
                self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown: nothing left to report to
            pass


def _all_ok(ctx: PeerContext, ok: int) -> bool:
    t = torch.tensor([ok], dtype=torch.int32, device=ctx.device if ctx.nccl else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=ctx.group)
    return bool(t.item())


class HipIpc:
    """The IPC transport of the push gather: HIP IPC handles of device allocations (C ABI fa_ipc_*), read back through
    a copy engine.  `_IPC` is the one in use: the CPU tests put a shared-memory stand-in there to run the pool's
    collective protocol, token checks included, over gloo (tests/test_recv_pool.py)."""

    def accepts(self, device) -> bool:
        return torch.device(device).type == "cuda"

    def sync(self, device):
        torch.cuda.synchronize(device)

    def handle(self, ptr: int):
        """(handle bytes, byte offset of ptr in its allocation), or None."""
        h, off = ctypes.create_string_buffer(64), ctypes.c_int64(0)
        if na.lib().fa_ipc_handle(ptr, h, ctypes.byref(off)) != 0:
            return None
        return bytes(h.raw), int(off.value)

    def open(self, hb: bytes):
        """The base address a peer's handle maps at here, or None."""
        base = ctypes.c_void_p()
        if na.lib().fa_ipc_open(hb, ctypes.byref(base)) != 0 or not base.value:
            return None
        return base.value

    def read16(self, probe: torch.Tensor, addr: int) -> bool:
        """The 16 bytes at a mapped address into `probe` (4 int32, same device)."""
        s = torch.cuda.current_stream(probe.device)
        if na.lib().fa_copy_dma(probe.data_ptr(), addr, 16, s.cuda_stream) != 0:
            return False
        s.synchronize()
        return True

    def close(self, base: int):
        na.lib().fa_ipc_close(base)

    def last_error(self) -> bytes:
        return na.lib().fa_last_error()


_IPC = HipIpc()


def _map_peers(ctx: PeerContext, full: torch.Tensor | None):
    """Collective: register `full` (IPC handle of its allocation + offset) and map every peer's; (opened bases,
    per-rank device address of each rank's buffer, stale peers).  A token written into the buffer's first 16 bytes
    (the caller's bytes there are saved and put back) is read back through every mapping: an import that maps some
    other allocation than the one exported is refused instead of pushed into (the stale imports
    of round 4).  Every rank raises RuntimeError (nothing left mapped) if any rank cannot map or validate a peer, or
    has no buffer to offer (`full` None: it takes part in every collective here and refuses)."""
    ipc = _IPC
    bases, dsts, stale = [], [], []
    mine = saved = None  # mine stays None where this rank has nothing to offer: every rank then refuses
    if (full is not None and ctx.world <= MAX_PUSH_RANKS and ipc.accepts(full.device) and full.is_contiguous()
            and full.numel() >= 4):
        head = full.view(torch.int32)[:4]
        saved = head.clone()
        token = torch.randint(-2**31, 2**31 - 1, (4,), dtype=torch.int32)
        head.copy_(token)
        ipc.sync(full.device)
        got = ipc.handle(full.data_ptr())
        if got is not None:
            mine = (got[0], got[1], token.tolist())
    infos = [None] * ctx.world
    dist.all_gather_object(infos, mine, group=ctx.group)
    ok = int(all(i is not None for i in infos))
    if ok:
        probe = torch.empty(4, dtype=torch.int32, device=full.device)
        for r, (hb, off, tok) in enumerate(infos):
            if r == ctx.rank:
                dsts.append(full.data_ptr())
                continue
            base = ipc.open(hb)
            if base is None:
                ok = 0
                break
            bases.append(base)
            dsts.append(base + off)
            if not ipc.read16(probe, base + off):
                ok = 0
                break
            if probe.tolist() != tok:
                stale.append(r)
                ok = 0
    agreed = _all_ok(ctx, ok)  # every rank has read every token it reads: the heads may go back
    if saved is not None:
        full.view(torch.int32)[:4].copy_(saved)
    if not agreed:
        for b in bases:
            ipc.close(b)
        dist.barrier(group=ctx.group)  # nobody exports again while a peer is still closing
        err = ipc.last_error()
        why = (f" (here: the mappings of ranks {stale} did not hold their tokens)" if stale else
               f" (here: {err.decode(errors='replace')})" if err and not ok else "")
        raise RuntimeError("PushGather: a rank could not map its peers' receive buffers" + why)
    return bases, dsts, stale


def _unmap_all(ctx: PeerContext, bases):
    """Collective: close this rank's imports, then a barrier — after it no peer is still closing an import when any
    rank exports again (exporting while a peer closes made a third of the probe's imports map the wrong allocation:
    DESIGN.md section 6)."""
    for b in bases:
        _IPC.close(b)
    dist.barrier(group=ctx.group)


def _resolve_group(group):
    return group if group is not None else dist.distributed_c10d._get_default_group()


def _group_alive(g) -> bool:
    try:
        return g in dist.distributed_c10d._world.pg_map
    except Exception:  # noqa: BLE001 - a torch without the registry: assume alive
        return True


@dataclass
class _Slot:  # one receive bucket of a pool, mapped by every peer
    buf: DeviceBuffer
    view: torch.Tensor  # the bucket as fp32
    dsts: list  # per-rank device address of that rank's bucket of this slot
    bases: list  # the peers' mappings opened here (closed when the slot is retired)
    busy: bool = False


class _RecvPool:
    """Receive buckets of the one-shot push, per (device, process group): each an allocation of its own
    (DeviceBuffer), exported once and mapped once by every peer, handed out to job after job (`take` / `give`: a few
    ms of collective set-up and token checks saved per job — the bench's plan trials build a dozen jobs).  Released
    collectively: `shutdown_push(group)` (call it before destroying the group) has every peer close its imports, then
    a barrier, and the buckets are parked for the next pool to re-export (DeviceBuffer: freeing memory that a peer has
    imported is what made later imports map the wrong allocation).  A `take` that finds no free
    bucket large enough first releases the free ones (same protocol) and takes a parked one that fits or a new one of
    the request's size class (DeviceBuffer.get), so the buckets held stay near the largest set in use at once and the
    parked ones within DeviceBuffer's cap.  Every rank takes and gives in the same order, so the slots agree across
    ranks (checked at each take).

    Keyed by the group OBJECT (held, so its id cannot be reused by a later group): a destroyed and re-created default
    group gets a new pool.  A pool whose group was destroyed without shutdown_push is dropped locally the next time
    any pool is looked up (imports closed with no barrier possible any more — the unordered unmap the token check at
    the next set-up guards against — buckets parked)."""

    _pools: dict = {}

    def __init__(self, device, gobj):
        self.device, self.gobj = device, gobj
        self.slots: list[_Slot] = []

    @classmethod
    def get(cls, device, group):
        g = _resolve_group(group)
        for key in [k for k, p in cls._pools.items() if not _group_alive(p.gobj)]:
            cls._pools.pop(key)._drop_local()
        key = (str(device), id(g))
        if key not in cls._pools:
            cls._pools[key] = _RecvPool(device, g)
        return cls._pools[key]

    @classmethod
    def bytes_held(cls) -> int:
        return sum(s.buf.nbytes for p in cls._pools.values() for s in p.slots)

    def _retire(self, ctx: PeerContext, idx):
        """Collective: every rank closes its imports of the slots `idx` (the same everywhere), a barrier, parks them."""
        if not idx:
            return
        _unmap_all(ctx, [b for i in idx for b in self.slots[i].bases])
        for i in sorted(idx, reverse=True):
            self.slots.pop(i).buf.free()  # exported: parked for reuse (within the parking cap)

    def take(self, ctx: PeerContext, cols: int):
        i = next((j for j, s in enumerate(self.slots) if not s.busy and s.view.numel() >= cols), None)
        picks = [None] * ctx.world
        dist.all_gather_object(picks, (i, len(self.slots)), group=ctx.group)
        if len(set(picks)) != 1:
            raise RuntimeError(f"PushGather: the ranks' receive pools disagree ({picks})")
        if i is None:  # retire the free buckets that are too small, then a new one (collective)
            self._retire(ctx, [j for j, s in enumerate(self.slots) if not s.busy])
            if not _IPC.accepts(self.device):
                _map_peers(ctx, None)  # nothing to offer: raises, on every rank together
            buf = DeviceBuffer.get(round_up(max(cols, 4)) * 4, self.device)
            view = buf.tensor(torch.float32)
            buf.exported = True  # from here on parked when released
            try:
                bases, dsts, _stale = _map_peers(ctx, view)
            except RuntimeError:
                del view
                buf.free()  # parked; every peer closed its imports (and barriered) before the raise
                raise
            self.slots.append(_Slot(buf, view, dsts, bases))
            i = len(self.slots) - 1
        slot = self.slots[i]
        slot.busy = True
        return i, slot.view, slot.dsts

    def give(self, i: int):
        self.slots[i].busy = False

    def shutdown(self, ctx: PeerContext):
        """Collective: unmap every bucket on every rank, barrier, park."""
        busy = sum(s.busy for s in self.slots)
        if busy:
            warnings.warn(f"shutdown_push: {busy} receive bucket(s) still in use by a reducer that was "
                          "not released; their results are overwritten by the next push job", stacklevel=3)
        self._retire(ctx, list(range(len(self.slots))))

    def _drop_local(self):
        for s in self.slots:
            for b in s.bases:
                _IPC.close(b)
            s.buf.free()
        self.slots = []


def shutdown_push(group=None, device=None):
    """Collective over `group`: release the push gather's receive buckets of this process for that group — every
    peer's mapping closed, then a barrier, then each rank parks its own (DeviceBuffer).  Call it before
    dist.destroy_process_group; the next push job maps its buckets afresh."""
    g = _resolve_group(group)
    for key in [k for k, p in _RecvPool._pools.items() if p.gobj is g
                and (device is None or k[0] == str(torch.device(device)))]:
        pool = _RecvPool._pools.pop(key)
        pool.shutdown(PeerContext.of(group, pool.device))


class PushGather:
    """One-shot all-gather over xGMI by direct peer stores (C ABI fa_ipc_* / fa_push).

    Every rank registers its receive buffer `full` once (IPC handles exchanged with all_gather_object) and maps its
    peers' buffers; a reduced stripe is then pushed by ONE kernel into every rank's `full` at the same offset — each
    peer's copy crosses that peer's own xGMI link, nothing is forwarded, received data is never re-read, and the
    receiving GPU spends no kernel on it (RCCL's all-gather forwards chunks along rings and copies them out of its
    buffers on every GPU: HBM traffic that competes with the reduce).

    Ordering, all on this object's stream: `begin()` — a barrier after this rank's earlier work on the compute stream
    (no peer may overwrite a `full` its owner is still reading); `push()` after the stripe's reduce; `end()` — a
    barrier after the pushes, which the compute stream then waits for: once every rank has passed it, every peer's
    stores into this rank's `full` are complete (each push kernel ends with a system-scope release).  On RCCL the
    barriers are 1-element all_reduces ordered on the stream; on gloo (several processes sharing one GPU in the tests)
    host synchronisations plus dist.barrier.

    Construction is collective and all-or-nothing: if any rank cannot map a peer, every rank raises RuntimeError
    (nothing stays mapped) and the caller keeps RCCL's all-gather."""

    def __init__(self, full: torch.Tensor | None, group=None, mode: str = "kernel", cols: int = 0, device=None):
        """full: the receive buffer to register (exported and mapped for this object, unmapped by close()) — a
        DeviceBuffer (its fp32 view becomes `self.full`; once exported it is never freed: `free()` parks it), or a
        tensor, whose whole caching-allocator segment is exported (the caller must then keep that memory allocated for
        the process's lifetime: a freed exported segment makes later imports unreliable); or None
        with `cols` / `device`: a bucket of at least `cols` fp32 columns from the process's receive pool (_RecvPool:
        mapped once by every peer, reused until shutdown_push)."""
        if mode not in ("kernel", "dma"):
            raise ValueError(f"PushGather mode {mode!r}")
        self.mode, self.L, self.pool_slot = mode, na.lib(), None
        if full is None:
            device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        else:
            if isinstance(full, DeviceBuffer):  # exported from here on: parked when released
                full.exported = True
                self.owner, full = full, full.tensor(torch.float32)
            device = full.device
        self.ctx = ctx = PeerContext.of(group, device)
        self.group, self.world, self.rank, self.nccl, self.device = group, ctx.world, ctx.rank, ctx.nccl, ctx.device
        if full is None:
            self.pool = _RecvPool.get(self.device, group)
            self.pool_slot, buf, self.dst = self.pool.take(ctx, cols)
            self.full, self.bases, self.stale = buf[:cols], [], []
        else:
            self.full = full
            self.bases, self.dst, self.stale = _map_peers(ctx, full)
        # a high-priority stream, whose hardware queue is apart from the compute stream's — on a
        # shared queue the push kernels run in queue order with the next stripes' reduces instead
        # of beside them (streams.py)
        self.stream = side_stream(self.device)
        self.flag = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.grid = 0  # fa_push blocks (0: the library's default)
        # mode "dma": one stream per peer, each leg a copy-engine copy (fa_copy_dma) — copies on
        # one stream would run one after the other, one link at a time
        self.peer_streams = [peer_stream(self.device) for _ in range(self.world - 1)] if mode == "dma" else []
        self._pending = None  # host order: the last stripe whose push is not issued yet
        self._peer_handles = (ctypes.c_void_p * max(1, len(self.peer_streams)))(
            *[s.cuda_stream for s in self.peer_streams]) if self.peer_streams else None

    def _barrier(self):
        if self.nccl:
            with torch.cuda.stream(self.stream):
                dist.all_reduce(self.flag, group=self.group)
        else:
            torch.cuda.synchronize(self.device)
            dist.barrier(group=self.group)

    def begin(self):
        # a step abandoned between its pushes (an exception before end()) leaves its last stripe
        # pending: never issue it into this step's buckets
        self._pending = None
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._barrier()

    def push(self, src: torch.Tensor, elem_offset: int):
        """Stores src (this rank's reduced slice) into every rank's `full` at elem_offset."""
        n = src.numel() * src.element_size()
        if n == 0:
            return
        off = elem_offset * self.full.element_size()
        if elem_offset < 0 or off + n > self.full.numel() * self.full.element_size():
            raise ValueError("push outside the receive buffer")
        cur = torch.cuda.current_stream(self.device)
        order = push_order(self.mode)
        if order == "host":
            # (the copy-engine push) the push of stripe c is issued once the host has seen stripe
            # c's reduce complete — at push(c+1), after reduce c+1 is queued — and needs no
            # device-side wait.  With device-side waits (an event of the reduce's stream,
            # "producer"; round 5's event on the pusher's stream, "chain"), eight processes sharing
            # a GPU with the copy-engine legs' streams on hardware queues of their own copied
            # stripes before their reduce had finished — the own-copy KERNEL on the pusher's stream
            # included (tests/push_order_probe.py --forensic).  The kernel push
            # (no copy-engine streams) takes the device-side order below: see _PUSH_ORDER
            ev = torch.cuda.Event()
            ev.record(cur)
            prev, self._pending = self._pending, (ev, src, off, n)
            if prev is not None:
                self._issue(*prev)
            return
        self.stream.wait_stream(cur)
        self._legs(src, off, n, after=self.stream if order == "chain" else cur)

    def _issue(self, ev, src, off, n):
        """Host order: wait on the host for the stripe's reduce, then push it."""
        ev.synchronize()
        self._legs(src, off, n)

    def _peers_at(self, off):
        """The peers' addresses of byte offset `off` in their buckets, in the legs' order."""
        return [d + off for r, d in enumerate(self.dst) if r != self.rank]

    def _own_copy(self, src, off, n):
        """This rank's own slice into its own bucket, on the pusher's stream."""
        na.check(self.L.fa_copy(self.dst[self.rank] + off, src.data_ptr(), n, self.stream.cuda_stream), "fa_copy")

    def _legs(self, src, off, n, after=None):
        """One stripe's stores, which the caller has ordered after the reduce: the push kernel on the pusher's stream,
        or the copy-engine legs on theirs and this rank's own copy — `after` None (host order: the host has waited):
        one fa_copy_dma per leg; else fa_push_dma, whose legs wait on the stream `after`."""
        if self.mode == "kernel":
            dsts = (ctypes.c_void_p * self.world)(*[d + off for d in self.dst])
            na.check(self.L.fa_push(src.data_ptr(), n, dsts, self.world, self.grid, self.stream.cuda_stream), "fa_push")
            return
        peers = self._peers_at(off)
        if after is None:
            for d, s in zip(peers, self.peer_streams):
                na.check(self.L.fa_copy_dma(d, src.data_ptr(), n, s.cuda_stream), "fa_copy_dma")
        else:
            na.check(self.L.fa_push_dma(src.data_ptr(), n, (ctypes.c_void_p * len(peers))(*peers), len(peers),
                                        self._peer_handles, after.cuda_stream), "fa_push_dma")
        self._own_copy(src, off, n)

    def join(self):
        """Every push of the step is issued and the copy-engine legs are complete before the closing barrier: in host
        order the pending stripe is pushed and the host waits for the legs' streams; otherwise the pusher's stream
        waits on them (a pending stripe left by a switch of _PUSH_ORDER mid-step is flushed either way)."""
        if push_order(self.mode) == "host" or self._pending is not None:
            if self._pending is not None:
                pending, self._pending = self._pending, None
                self._issue(*pending)
            for s in self.peer_streams:
                s.synchronize()
            return
        if self.peer_streams:
            na.check(self.L.fa_stream_join(self.stream.cuda_stream, self._peer_handles, len(self.peer_streams)),
                     "fa_stream_join")

    def end(self):
        self.join()
        self._barrier()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def gather(self, src: torch.Tensor, elem_offset: int):
        """A whole all-gather of one slice: begin, push, end."""
        self.begin()
        self.push(src, elem_offset)
        self.end()

    def close(self):
        """Collective: after every rank's pushes are done (a barrier), a pool bucket goes back to the pool, still
        mapped; an explicitly registered `full` is unmapped by every peer and a second barrier follows, so no rank
        frees or re-exports its buffer while a peer still maps it."""
        if self.dst:
            torch.cuda.synchronize(self.device)
            dist.barrier(group=self.group)
            if self.pool_slot is not None:
                self.pool.give(self.pool_slot)
                self.pool_slot, self.dst = None, []
            else:
                _unmap_all(self.ctx, self.bases)
                self.bases, self.dst = [], []
