"""Device-side AVGM / FedOPT update of a received global model (the client_receive form).

The reference runs `mean_momentum` (avgm.py:19-36) and `adaptive_opt` (opt.py:23-65) per client
in numpy float64.  `DeviceUpdater` flattens w_local (fp32) and w_glob (the server's float64 —
or float32 — arrays) into aligned device buffers, keeps v_t resident in HBM across rounds and
runs one fa_opt_apply launch, with the reference's operation order and precision.
"""
from __future__ import annotations

import concurrent.futures
import ctypes
import math
import time
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np
import torch

from .. import _native as na
from .. import ops  # its _epilogue / apply_update are called through the module (tests patch them there)
from ..bucketplan import FMT, padded_span
from ..dist import DoubleBuffer
from ..packer import AsyncPack, NativeRows, pack_threads
from ..serverstate import _as_host

_F32 = np.dtype(np.float32)
_DEV_GLOB = (np.dtype(np.float64), _F32)  # w_glob dtypes the device path takes
_PART_BYTES = 16 << 20  # host copies are split into parts of about this size, one per pool task
_POOL = None


def _pool() -> concurrent.futures.ThreadPoolExecutor:
    global _POOL
    if _POOL is None:
        # the pack is host-memory copies (the GIL released): as many threads as the process may
        # use, up to 16 (the GPU box's CPU share per GPU)
        _POOL = concurrent.futures.ThreadPoolExecutor(pack_threads(), thread_name_prefix="fa-update")
    return _POOL


def _run(tasks):
    """Run zero-argument callables (copies that release the GIL) on the pool; their results."""
    if len(tasks) == 1:
        return [tasks[0]()]
    return [f.result() for f in [_pool().submit(t) for t in tasks]]


class _DictPack:
    """Copies one dict's arrays into a flat staging buffer at the layout's offsets with
    fa_py_pack_rows (csrc/fa_pyhost.c), in byte-balanced parts run on the pool; False when a
    value is not a C-contiguous array of the expected dtype (the caller then copies in Python)."""

    def __init__(self, lay, dtype, dst_ptr, part_bytes=_PART_BYTES):
        self.fn = na.load_pyhost().fa_py_pack_rows
        item, fmt = np.dtype(dtype).itemsize, FMT[np.dtype(dtype)]
        parts, cur, size = [], [], 0
        for k, _s, o, n in lay:
            cur.append((k, n, o))
            size += n * item
            if size >= part_bytes:
                parts.append(cur)
                cur, size = [], 0
        if cur:
            parts.append(cur)
        self.parts = []
        for part in parts:  # whole values into the one staging row, which is not skipped
            nb = np.array([n for _, n, _ in part], dtype=np.int64) * item
            desc = NativeRows.table(value_bytes=nb, first_byte=0, nbytes=nb, fmt=fmt, dst_base=dst_ptr, dst_row=0,
                                    dst_off=np.array([o for _, _, o in part], dtype=np.int64) * item)
            self.parts.append((tuple(k for k, _, _ in part), np.append(desc, 0)))

    def tasks(self, d: dict):
        """The pack as pool tasks (one per part); each returns 0 on success."""
        if type(d) is not dict:
            d = dict(d)
        clients = [d]
        return [(lambda keys=keys, desc=desc: self.fn(clients, keys, len(keys), desc.ctypes.data, 0, 1))
                for keys, desc in self.parts]

    def __call__(self, d: dict) -> bool:
        return all(rc == 0 for rc in _run(self.tasks(d)))


class _Slot(NamedTuple):
    """One key's place in the flat layout."""
    key: str
    shape: tuple
    offset: int
    numel: int


class _Chunk(NamedTuple):
    """A run of whole keys of the layout: one launch of the zero-copy paths."""
    first: int  # its element range [first, end) of the flat layout
    end: int
    pack_l: _DictPack  # its own pack tables into the shared staging (the Python-pool pack)
    pack_g: _DictPack
    keys: list  # its _Slots


@dataclass
class _Staging:
    """Pinned staging of one layout, and what is built on it: all dropped with it."""
    lh: torch.Tensor  # w_local, float32
    gh: torch.Tensor  # w_glob
    oh: torch.Tensor | None  # the copy-engine path's result (made when that path first runs)
    pack_l: _DictPack  # whole-layout pack tables
    pack_g: _DictPack
    chunks: list | None = None  # the zero-copy chunk plan
    apacks: dict = field(default_factory=dict)  # with w_local? -> the chunk plan's native pack
    dma: "_DmaBuffers | None" = None
    devmodel: "_DevModel | None" = None


class _DmaBuffers(NamedTuple):
    """transfer = "dma": device copies of the staging and the result, the copy-in / copy-out streams."""
    dl: torch.Tensor
    dg: torch.Tensor
    dout: torch.Tensor
    s_in: torch.cuda.Stream
    s_out: torch.cuda.Stream


@dataclass
class _DevModel:
    """update_on_device's buffers: the gathered local model, w_glob and the result on the device,
    the gather's segment table and its pointer table (pinned and device)."""
    dev: torch.device
    dl: torch.Tensor
    dg: torch.Tensor
    dout: torch.Tensor
    segs: torch.Tensor
    ptr_h: torch.Tensor
    ptr_d: torch.Tensor


class _AsyncPack(AsyncPack):
    """The zero-copy chunk plan's copies into the pinned staging as one native job list: per
    key, w_local's float32 value (when `lh_ptr` is given) and w_glob's value, in chunk order."""

    def __init__(self, chunks, lh_ptr, gh_ptr, gdtype):
        item = torch.empty((), dtype=gdtype).element_size()
        # the dicts copied from: (index in start()'s pair, staging address, itemsize, format class)
        srcs = [(0, lh_ptr, 4, ord("f"))] if lh_ptr is not None else []
        srcs.append((1, gh_ptr, item, ord("d") if item == 8 else ord("f")))
        src, base, size, fmt = np.array(srcs, dtype=np.int64).T
        # _Chunks, or any tuples that end in their slots: per slot its chunk, offset and elements
        chunk, off, numel = np.array([(j, o, n) for j, (*_, slots) in enumerate(chunks) for _k, _s, o, n in slots],
                                     dtype=np.int64).reshape(-1, 3).T[:, :, None]
        rows = self.table(src=src, value_bytes=numel * size, fmt=fmt, dst=base + off * size, chunk=chunk,
                          first_byte=0, nbytes=numel * size)
        keys = tuple(k for *_, slots in chunks for k, *_ in slots for _ in srcs)
        super().__init__(keys, rows, len(chunks))

    def start(self, local, glob):
        return super().start((local if local is not None else {}, glob))


class _ChunkFeed:
    """One call's packing of the chunk plan into the pinned staging.  Every chunk's copies are
    queued at once, in chunk order: native threads (or, for values the native pack refuses, the
    Python pool) stay busy whatever the chunk sizes, and each chunk's kernel is launched as soon
    as its own copies are in.  local None: w_glob only."""

    def __init__(self, ap: _AsyncPack | None, st: _Staging, local, glob):
        self.ap, self.st, self.local, self.glob = ap, st, local, glob
        self.h = ap.start(local, glob) if ap is not None else None
        self.futs = None
        if self.h is None:
            pool = _pool()
            self.futs = [([pool.submit(t) for t in c.pack_l.tasks(local)] if local is not None else [],
                          [pool.submit(t) for t in c.pack_g.tasks(glob)]) for c in st.chunks]

    def wait(self, j: int):
        """Chunk j is in the staging."""
        if self.h is not None:
            return self.ap.wait(self.h, j)
        for futs, host, src in zip(self.futs[j], (self.st.lh, self.st.gh), (self.local, self.glob)):
            if any(f.result() for f in futs):  # a value the native pack refuses: copy in Python
                for k, _s, o, n in self.st.chunks[j].keys:
                    host.numpy()[o : o + n] = src[k].reshape(-1)

    def end(self):
        """Every copy is done: releases the values."""
        if self.h is not None:
            self.ap.end(self.h)

    def abort(self, *streams):
        """After an error: no pack may still write the staging, nor a queued chunk read it or
        write its result."""
        self.end()
        if self.futs is not None:
            futs = [f for fl, fg in self.futs for f in fl + fg]
            for f in futs:
                f.cancel()
            concurrent.futures.wait(futs)
        for s in streams:
            s.synchronize()


class DeviceUpdater:
    #: zero-copy, chunked: the update kernel reads w_local / w_glob from the pinned staging and
    #: writes the result straight into a fresh pinned buffer over PCIe, one chunk of keys at a
    #: time, while the pool packs the next chunk; the new w_local values are views of that buffer
    #: (no copy-out).  False: pack everything, two H2D copies, one launch, one D2H, a host copy
    #: out; tools/bench_client_update.py --ab times both
    zero_copy = True
    #: with zero_copy: how the chunks cross PCIe.  "dma": each packed chunk is copied to the GPU
    #: by a copy engine on its own stream, updated there, and its result copied back into the
    #: pinned result by another copy engine — H2D and D2H run concurrently at DMA rate;
    #: "kernel": the update kernel itself reads the pinned staging and writes the pinned result
    #: over PCIe (zero-copy loads run below the DMA rate: 38 vs ~55 GB/s, round 4)
    transfer = "kernel"
    chunk_bytes = 64 << 20  # w_glob bytes per zero-copy chunk (the middle ones; 32 MiB: +0.3-0.8 ms, round 4)
    first_chunk_bytes = 4 << 20  # the first chunks grow from this (x2 each) so the GPU starts early
    last_chunk_bytes = 8 << 20  # ... and the last ones shrink towards this: a short exposed tail
    #: the zero-copy chunks are packed by native threads (fa_py_pack_start: 512 KiB jobs, no
    #: interpreter work per job, the waiting thread copies too); False: Python pool tasks of
    #: 4 MiB parts (the fallback for values the native pack refuses)
    native_pack = True
    #: a list to receive per-call phase times (tools/bench_client_update.py --phases), or None
    trace = None

    def __init__(self, op: str, device=None, beta=0.9, eta=1e-1, tau=1e-9, beta2=0.99):
        self.op = na.OP_BY_NAME[op]
        self.device = device
        self.params = dict(beta=beta, eta=eta, tau=tau, beta2=beta2)
        self.layout = None  # [(key, shape, offset, numel)]
        self.v = None  # v_t, a DoubleBuffer (the zero-copy paths: all or nothing; else in place)
        self.v_host = {}  # v_t of the keys computed on the host (integer buffers, scalars)
        self._stage = None  # the _Staging of the current layout
        self._lay_cache = None  # (signature, layout, total) of the last w_glob
        self._h2d_done = None  # update_on_device's last DMA out of the pinned staging
        self.last_pack = None  # "native" | "pool": how the last host-model zero-copy call packed

    def _layout(self, w_glob):
        """[(key, shape, offset, numel)], total — cached on the (key, shape) signature: the same
        model comes back every round."""
        sig = tuple((k, g.shape) for k, g in w_glob.items())
        if self._lay_cache is not None and self._lay_cache[0] == sig:
            return self._lay_cache[1:]
        lay, off = [], 0
        for k, shape in sig:
            n = math.prod(shape) if shape else 1
            lay.append(_Slot(k, shape, off, n))
            off += padded_span(n)
        self._lay_cache = (sig, lay, off)
        return lay, off

    def reset(self):
        """Forget v_t (device and host keys): the next call starts from zeros, as a fresh
        strategy object would."""
        self.layout, self.v, self._stage, self.v_host = None, None, None, {}

    def state(self):
        """v_t as the reference exposes it: {key: ndarray}."""
        out = {}
        if self.v is not None:
            host = self.v.cur.cpu().numpy()
            out = {k: host[o : o + n].reshape(s).copy() for k, s, o, n in self.layout}
        out.update(self.v_host)
        return out

    def __call__(self, w_local, w_glob, **override):
        t_call = time.perf_counter()
        n_trace = len(self.trace) if self.trace is not None else 0
        self._call(w_local, w_glob, **override)
        if self.trace is not None and len(self.trace) > n_trace:
            self.trace[-1]["call_s"] = time.perf_counter() - t_call
        return w_local

    def _call(self, w_local, w_glob, **override):
        na.lib()
        glob, local, host_keys = {}, {}, []
        gdt = None
        nd, tt = np.ndarray, torch.Tensor
        for k, g in w_glob.items():
            lv = w_local[k]
            # exact-type tests first: this loop runs over every key of every call (~0.2 ms for
            # ResNet-50's 320 keys with isinstance chains, part of what the call costs)
            if type(g) is not nd:
                if isinstance(g, tt):
                    g = g.detach().cpu().numpy()
                elif not isinstance(g, nd):
                    host_keys.append(k)
                    continue
            if type(lv) is not nd:
                if isinstance(lv, tt):
                    lv = lv.detach().cpu().numpy()
                elif not isinstance(lv, nd):
                    host_keys.append(k)
                    continue
            # the device handles fp32 parameters against a float64 / float32 global model, one
            # precision per call (the first key's); anything else (BN num_batches_tracked: int64
            # local, numpy-scalar global) takes the reference's numpy ops on the host, key by key,
            # as avgm.py / opt.py compute them
            dt = g.dtype
            if (g.ndim >= 1 and lv.dtype == _F32 and lv.shape == g.shape and dt in _DEV_GLOB
                    and (gdt is None or dt == gdt)):
                gdt = dt
                glob[k], local[k] = g, lv
            else:
                host_keys.append(k)
        if glob:
            self._device_step(w_local, glob, local, gdt, **override)
        if host_keys:
            self._host_step(w_local, w_glob, host_keys, **override)
        return w_local

    def _host_step(self, w_local, w_glob, keys, **override):
        """The reference's per-key numpy arithmetic (avgm.py:19-36 / opt.py:23-65) for the keys the
        device path does not take; their v_t lives on the host (np.zeros_like(delta) first).
        The common case — BN num_batches_tracked: a 0-d int64 local value against a float64
        scalar in w_glob — runs as ONE vectorised numpy evaluation of the same expressions over
        all such keys (elementwise, so every value is what the per-key scalar ops give; results
        are handed back as the np.float64 scalars numpy returns for 0-d operands)."""
        p = dict(self.params, **override)
        vh = self.v_host
        batch = [k for k in keys if type(w_local[k]) is np.ndarray and w_local[k].ndim == 0
                 and w_local[k].dtype == np.int64 and type(w_glob[k]) in (np.float64, float)
                 and (k not in vh or type(vh[k]) is np.float64)]
        if len(batch) > 1:
            lv = np.array([w_local[k] for k in batch], dtype=np.int64)
            g = np.array([w_glob[k] for k in batch], dtype=np.float64)
            delta = g - lv
            v = np.array([vh[k] if k in vh else 0.0 for k in batch], dtype=np.float64)
            out, v = self._numpy_update(p, lv, delta, v)
            for i, k in enumerate(batch):
                w_local[k] = out[i]
                vh[k] = v[i]
            done = set(batch)
            keys = [k for k in keys if k not in done]
        for k in keys:
            lv, g = _as_host(w_local[k]), _as_host(w_glob[k])
            delta = g - lv
            v = vh.get(k)
            if v is None:
                v = np.zeros_like(delta)
            w_local[k], vh[k] = self._numpy_update(p, lv, delta, v)

    def _numpy_update(self, p, lv, delta, v):
        """(new w_local, new v_t) by the reference's numpy expressions (avgm.py:28-35, opt.py:45-63)."""
        if self.op == na.OP_AVGM:
            v = delta + p["beta"] * v
            return lv + v, v
        sq = np.multiply(delta, delta)
        if self.op == na.OP_ADAGRAD:
            v = v + sq
        elif self.op == na.OP_YOGI:
            v = v - (1 - p["beta2"]) * sq * np.sign(v - sq)
        else:
            v = p["beta2"] * v + (1 - p["beta2"]) * sq
        return lv + p["eta"] * delta / (np.sqrt(v) + p["tau"]), v

    def _bind(self, glob, tdt, dev) -> tuple:
        """(layout, total, staging) of this call: v_t (zeros on first use, np.zeros_like(delta)) and
        the pinned staging bound to w_glob's layout and dtype; a change of either raises."""
        lay, total = self._layout(glob)
        if self.v is not None and (self.layout != lay or self.v.cur.dtype != tdt):
            raise ValueError("the model layout or w_glob's dtype changed between rounds: v_t no longer matches; "
                             "call reset() to start the optimizer state afresh")
        if self.v is None:
            self.layout = lay
            self.v = DoubleBuffer(torch.zeros(total, dtype=tdt, device=dev))
            self._stage = None
        if self._stage is None:  # made once per layout, and zeroed once: only the segments are ever
            # written, so the alignment gaps stay zero
            lh = torch.zeros(total, dtype=torch.float32, pin_memory=True)
            gh = torch.zeros(total, dtype=tdt, pin_memory=True)
            gdt = np.float64 if tdt == torch.float64 else np.float32
            self._stage = _Staging(lh, gh, None, _DictPack(lay, np.float32, lh.data_ptr()),
                                   _DictPack(lay, gdt, gh.data_ptr()))
        if self._h2d_done is not None:  # update_on_device's DMAs out of the shared pinned staging are done
            self._h2d_done.synchronize()
            self._h2d_done = None
        return lay, total, self._stage

    def _device_step(self, w_local, glob, local, gdt, **override):
        dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        tdt = torch.float64 if gdt == np.float64 else torch.float32
        lay, total, st = self._bind(glob, tdt, dev)
        if self.zero_copy:
            return self._device_step_zc(w_local, glob, local, lay, total, tdt, dev, **override)
        if st.oh is None:
            st.oh = torch.empty(total, dtype=tdt, pin_memory=True)
        lh, gh, oh = st.lh, st.gh, st.oh
        with torch.cuda.device(dev):
            # local -> pinned -> device, then the global model while the local one is in flight
            if not st.pack_l(local):
                for k, s, o, n in lay:
                    lh.numpy()[o : o + n] = local[k].reshape(-1)
            ld = lh.to(dev, non_blocking=True)
            if not st.pack_g(glob):
                for k, s, o, n in lay:
                    gh.numpy()[o : o + n] = glob[k].reshape(-1)
            gd = gh.to(dev, non_blocking=True)
            out = torch.empty(total, dtype=tdt, device=dev)
            params = dict(self.params, **override)
            kw = {"out64": out} if tdt == torch.float64 else {"out32": out}
            ops.apply_update(self.op, ld, gd, self.v.cur, **kw, **params)
            oh.copy_(out, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()  # staging is reused by the next call
        # one fresh array for the new w_local, filled from the pinned result by the pool
        src = oh.numpy()
        fresh = np.empty(total, dtype=src.dtype)
        step = 1 << 22
        _run([(lambda a=a: np.copyto(fresh[a : a + step], src[a : a + step])) for a in range(0, total, step)])
        for k, s, o, n in lay:  # replaced per key, like the reference (avgm.py:34-35, opt.py:62-63)
            w_local[k] = fresh[o : o + n].reshape(s)

    def _chunks(self, lay, total, tdt):
        """The staging's chunk plan, [_Chunk]: runs of whole keys of about chunk_bytes of w_glob, in
        layout order, with their own pack tables into the shared staging (made once per staging)."""
        st = self._stage
        if st.chunks is not None:
            return st.chunks
        gdt = np.float64 if tdt == torch.float64 else np.float32
        item = np.dtype(gdt).itemsize
        # target sizes: first_chunk_bytes doubling up to chunk_bytes, then chunk_bytes, and the
        # last ones halving down to last_chunk_bytes (the exposed ends of the pipeline: the first
        # chunk's pack before the GPU starts, the last chunk's kernel after the pack is done)
        total_b = sum(n for _k, _s, _o, n in lay) * item
        head, b = [], max(1, int(self.first_chunk_bytes))
        while b < self.chunk_bytes and sum(head) + b < total_b:
            head.append(b)
            b *= 2
        tail, b = [], max(1, int(self.last_chunk_bytes))
        while b < self.chunk_bytes and sum(head) + sum(tail) + b < total_b:
            tail.append(b)
            b *= 2
        tail.reverse()
        mid = max(0, total_b - sum(head) - sum(tail))
        targets = head + [self.chunk_bytes] * max(1, -(-mid // max(1, self.chunk_bytes))) + tail
        groups, cur, size = [], [], 0
        for e in lay:
            cur.append(e)
            size += e.numel * item
            if size >= targets[min(len(groups), len(targets) - 1)]:
                groups.append(cur)
                cur, size = [], 0
        if cur:
            groups.append(cur)
        bounds = [0] + [g[0].offset for g in groups[1:]] + [total]
        st.chunks = [_Chunk(bounds[j], bounds[j + 1], _DictPack(g, np.float32, st.lh.data_ptr(), 4 << 20),
                            _DictPack(g, gdt, st.gh.data_ptr(), 4 << 20), g) for j, g in enumerate(groups)]
        return st.chunks

    def _feed(self, local, glob) -> _ChunkFeed:
        """Start packing the chunk plan (w_glob only, or w_local and w_glob): the native async pack,
        made once per staging, or the Python pool."""
        st = self._stage
        ap = None
        if self.native_pack:
            ap = st.apacks.get(local is not None)
            if ap is None:
                ap = st.apacks[local is not None] = _AsyncPack(
                    st.chunks, st.lh.data_ptr() if local is not None else None, st.gh.data_ptr(), st.gh.dtype)
        return _ChunkFeed(ap, st, local, glob)

    def _device_step_zc(self, w_local, glob, local, lay, total, tdt, dev, **override):
        """All or nothing: v_t advances into the second buffer, which becomes v_t only after
        every chunk ran; on any error the queued chunks are waited for (they read the staging
        the next call repacks) and v_t, the staging and w_local are as before the call."""
        st = self._stage
        lh, gh = st.lh, st.gh
        L = na.lib()
        prec = na.PREC_F64 if tdt == torch.float64 else na.PREC_F32
        p = dict(self.params, **override)
        v_in, v_out = self.v.cur, self.v.other
        # the new w_local lives in a fresh pinned buffer the kernel writes over PCIe; the values
        # handed out are views of it (torch's host caching allocator recycles it once they die)
        t_alloc = time.perf_counter()
        res = torch.empty(total, dtype=tdt, pin_memory=True)
        dma = self.transfer in ("dma", "dma_in")
        dma_out = self.transfer == "dma"
        if dma and st.dma is None:
            st.dma = _DmaBuffers(torch.empty(total, dtype=torch.float32, device=dev),
                                 torch.empty(total, dtype=tdt, device=dev), torch.empty(total, dtype=tdt, device=dev),
                                 torch.cuda.Stream(dev), torch.cuda.Stream(dev))
        d = st.dma
        tr = [] if self.trace is not None else None
        t0 = time.perf_counter()
        chunks = self._chunks(lay, total, tdt)
        feed = self._feed(local, glob)
        self.last_pack = "native" if feed.h is not None else "pool"
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            sh = stream.cuda_stream
            try:
                for j, c in enumerate(chunks):
                    tp = time.perf_counter()
                    feed.wait(j)
                    first, end = c.first, c.end
                    if dma:  # copy engine in (own stream), the update on the device, copy engine out
                        with torch.cuda.stream(d.s_in):
                            d.dl[first:end].copy_(lh[first:end], non_blocking=True)
                            d.dg[first:end].copy_(gh[first:end], non_blocking=True)
                        stream.wait_stream(d.s_in)
                        src_l, src_g = d.dl[first:end], d.dg[first:end]
                        out = (d.dout if dma_out else res)[first:end].data_ptr()
                    else:  # the kernel reads the pinned staging and writes the pinned result over PCIe
                        src_l, src_g, out = lh[first:end], gh[first:end], res[first:end].data_ptr()
                    epi = ops._epilogue(self.op, src_l, v_in[first:end], p["beta"], p["eta"], p["tau"],
                                        p["beta2"], v_out=v_out[first:end])
                    na.check(L.fa_opt_apply(prec, ctypes.byref(epi), src_l.data_ptr(), src_g.data_ptr(),
                                            end - first, None if prec == na.PREC_F64 else out,
                                            out if prec == na.PREC_F64 else None, sh), "fa_opt_apply")
                    if dma_out:
                        d.s_out.wait_stream(stream)
                        with torch.cuda.stream(d.s_out):
                            res[first:end].copy_(d.dout[first:end], non_blocking=True)
                    if tr is not None:
                        tr.append((end - first, tp - t0, time.perf_counter() - t0))
            except BaseException:
                feed.abort(stream, *((d.s_in, d.s_out) if dma else ()))
                raise
            ts = time.perf_counter()
            feed.end()
            # the new values' views are made while the GPU finishes (they read nothing yet)
            fresh = res.numpy()
            views = [(k, fresh[o : o + n].reshape(s)) for k, s, o, n in lay]
            stream.synchronize()
            if dma:
                d.s_out.synchronize()
        self.v.flip()
        if tr is not None:
            self.trace.append({"chunks": tr, "launched_s": ts - t0, "done_s": time.perf_counter() - t0,
                               "alloc_s": t0 - t_alloc})
        w_local.update(views)  # replaced per key, like the reference (avgm.py:34-35, opt.py:62-63)

    # ---- the model already on the GPU (client_receive with a CUDA model) ---------------------
    @staticmethod
    def device_model_ok(weights, w_glob) -> bool:
        """True when client_receive can update the model where it lives: every state_dict value
        a contiguous float32 CUDA tensor on one device, and every w_glob value an ndarray of the
        same shape, all float64 or all float32 (what the server returns for fp32 models).
        Anything else — BN counters (whose numpy scalars make the reference's convert_to_tensor
        raise), CPU models, other dtypes — takes the reference's host path unchanged."""
        if not weights or not w_glob:
            return False
        devs = set()
        for v in weights.values():
            if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
                return False
            devs.add(v.device)
        if len(devs) != 1:
            return False
        gdt = None
        for k, g in w_glob.items():
            lv = weights.get(k)
            if lv is None or type(g) is not np.ndarray or g.dtype not in (np.float64, np.float32):
                return False
            if tuple(g.shape) != tuple(lv.shape):
                return False
            if gdt is None:
                gdt = g.dtype
            elif g.dtype != gdt:
                return False
        return True

    def update_on_device(self, local: dict, w_glob: dict, **override) -> dict:
        """The update of a model that lives on the GPU: w_local's values are the model's float32
        CUDA tensors (gathered in one launch, fa_gather_rows), w_glob's host arrays go to the GPU
        in chunks (packed by the pool into pinned staging, one DMA each) and each chunk's update
        runs as soon as it lands.  Returns {key: the new value as a CUDA tensor in w_glob's dtype}
        for w_glob's keys — what load_state_dict then casts into the float32 parameters, exactly
        as it casts the reference's float64 host arrays.  Only the server's model crosses PCIe
        (the reference moves the local model down and the result back up as well).  v_t is the
        same double-buffered state the host path keeps, so the two paths may alternate."""
        L = na.lib()
        glob = {k: np.ascontiguousarray(g) for k, g in w_glob.items()}
        gdt = next(iter(glob.values())).dtype
        tdt = torch.float64 if gdt == np.float64 else torch.float32
        dev = next(iter(local.values())).device
        lay, total, st = self._bind(glob, tdt, dev)
        gh = st.gh
        if st.devmodel is None or st.devmodel.dev != dev:
            segs = torch.tensor([o for _, _, o, _ in lay] + [n for _, _, _, n in lay], dtype=torch.int64).to(dev)
            st.devmodel = _DevModel(dev, torch.zeros(total, dtype=torch.float32, device=dev),
                                    torch.empty(total, dtype=tdt, device=dev), torch.empty(total, dtype=tdt, device=dev),
                                    segs, torch.empty(len(lay), dtype=torch.int64, pin_memory=True),
                                    torch.empty(len(lay), dtype=torch.int64, device=dev))
        db = st.devmodel
        dl, dg, dout = db.dl, db.dg, db.dout
        v_in, v_out = self.v.cur, self.v.other
        prec = na.PREC_F64 if tdt == torch.float64 else na.PREC_F32
        p = dict(self.params, **override)
        chunks = self._chunks(lay, total, tdt)
        feed = self._feed(None, glob)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            sh = stream.cuda_stream
            try:
                # the local model: one gather launch of every tensor into its layout slot
                db.ptr_h.numpy()[:] = [local[k].data_ptr() for k, _, _, _ in lay]
                db.ptr_d.copy_(db.ptr_h, non_blocking=True)
                na.check(L.fa_gather_rows(dl.data_ptr(), total, 1, 4, db.ptr_d.data_ptr(), db.segs.data_ptr(), len(lay),
                                          sh), "fa_gather_rows")
                for j, c in enumerate(chunks):
                    feed.wait(j)
                    first, end = c.first, c.end
                    dg[first:end].copy_(gh[first:end], non_blocking=True)
                    epi = ops._epilogue(self.op, dl[first:end], v_in[first:end], p["beta"], p["eta"], p["tau"],
                                        p["beta2"], v_out=v_out[first:end])
                    out = dout[first:end].data_ptr()
                    na.check(L.fa_opt_apply(prec, ctypes.byref(epi), dl[first:end].data_ptr(), dg[first:end].data_ptr(),
                                            end - first, None if prec == na.PREC_F64 else out,
                                            out if prec == na.PREC_F64 else None, sh), "fa_opt_apply")
            except BaseException:
                feed.abort(stream)
                raise
            feed.end()
            done = torch.cuda.Event()
            done.record(stream)
        self._h2d_done = done
        self.v.flip()
        # fresh result buffer per call: the returned tensors must not be overwritten by the next
        db.dout = torch.empty(total, dtype=tdt, device=dev)
        return {k: dout[o : o + n].view(s) for k, s, o, n in lay}
