"""Device aggregation engine behind Strategy.server_ensemble.

`Aggregator.ensemble(agg_weight_lst, w_local_lst, key_lst)` is the MI355X replacement for
flearn/common/strategy/strategy.py:102-130: plan the buckets (bucketplan.py), copy the uploads into
HBM, run ONE fused reduce launch per bucket kind on torch's current stream, and hand back a
fresh dict with the reference's value types.  `begin_round` aggregates the same round in chunks of
clients (streaming.py); both end in the same server step (`Aggregator._server_step`), fed by
either kind of weighted sum (ops.StackSum, ops.FoldedSum).  `ensemble_trimmed` is the robust round:
coordinate-wise trimmed sums (ops.trim_sum_stack) into the same server step.  `ensemble_krum` is the
per-client robust round: the clients' Gram matrix (ops.gram_stack), krum.krum_select on the host, and
the selected uploads' mean from the stacks already on the device.

The device-level entry points on torch CUDA tensors are ops.py, the resident optimizer state
(`ServerOptimizer`, `DynState`) serverstate.py, the small-host-round fast path smallround.py; every
name this module defined before it was split is re-exported here as the same object.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _native as na
from . import krum, smallround
from .bucketplan import TORCH_DTYPE, BucketPlan, Group, Shard, make_plan, rank_width, select_keys
from .dist import gather_columns
from .ops import (FoldedSum, StackSum, _byte_range, _check_arrays, _check_cuda, _check_stack, _check_v_out,  # noqa: F401
                  _check_weights, _check_window, _epilogue, _ptr, _reduce_stack8, apply_dyn, apply_update, fill_uniform,
                  last_launch, mean_tables, reduce_stack, reduce_stack_f16, reduce_stack_f64, reduce_stack_i64,
                  set_reduce_grid)
from .ops import _ACC_TORCH, acc_kind_of, gram_stack, gram_workspace, trim_sum_stack
from .packer import Packer
from .rowtable import RowTable
from .semantics import KIND_F16, KIND_F32, Numerics
from .serverstate import (DynState, ServerOptimizer, _as_host, _bucket_host, _flatten, _host_array,  # noqa: F401
                          _layout_signature, _to_shards)
from .smallround import _SmallBucket, _SmallChain, _SmallRecord, chain_table  # noqa: F401
from .streaming import RoundAccumulator

_F64 = np.dtype(np.float64)
_ONE_W32 = Numerics(KIND_F32, na.MODE_W32_DIV64, np.ones(1, np.float32), 1.0, np.dtype(np.float32), _F64)  # fl32(1.0)

OUTPUTS = ("reference", "float32", "device")


class Aggregator:
    """output: "reference" — values with the reference's types and dtypes (float64 ndarrays, numpy
    scalars for 0-d buffers, torch CPU tensors when the uploads were tensors);
    "float32" — fp32 ndarrays for fp32 keys (the values load_state_dict ends up with);
    "device" — fresh torch CUDA tensors on the first device, fp32 for fp32 keys (no D2H).
    float16 keys (model.half() clients; fa_reduce_f16): "reference" returns the reference's dtypes —
    float64, or float16 / float32 for np.float16 / np.float32 weights; "float32" means "what
    load_state_dict ends up with", which for a float16 key is a float16 array holding fl16(fl32(q))
    (load_state_dict of the float64 result goes through float: not fl16(q)); "device" returns fresh
    float16 device tensors with those same values.  Server-fused optimizers and devices=[...] /
    group= sharding refuse float16 buckets with a TypeError before anything is queued.

    devices: the HIP devices the f32 bucket is split over (column shards); each ingests its
    columns through its own PCIe link.  Default: torch's current device only."""

    #: small host rounds (_small_round): the reduce kernel reads the uploads straight from the
    #: pinned staging and writes the result into pinned host memory (zero-copy over PCIe) instead
    #: of an H2D copy, the launch and a D2H copy: C1 server call 141 -> 123 us on one box, same
    #: process, bit-equal (tools/prof_host_c1.py --ab, profiles/r03/c1_zc/); False = copy engines
    small_zero_copy = True
    #: the zero-copy fp32 bucket of a small round may be summed in this many chained launches
    #: (client parts, each launched as soon as native threads have packed it: packer.AsyncPack);
    #: 1 = one native pack on the calling thread, one launch.  At flearn's config 1 every extra
    #: launch costs more than the overlap saves: 1 / 2 / 3 / 4 launches 113.5 / 120.3 / 127.4 /
    #: 135.7 us per server call, numpy 142 us (tools/prof_host_c1.py --parts, profiles/r04/c1_parts/)
    small_parts = 1
    #: _small_round(plan, w_local_lst): the small-host-round fast path (smallround.py), bound here as
    #: a method so the server call pays no extra Python call for the split
    _small_round = smallround._small_round

    def __init__(self, device=None, output: str = "reference", workers: int = 8, devices=None, group=None,
                 reorder: bool = False, chunk_clients: int | None = None):
        na.lib()  # fail loudly right away if the HIP path is unavailable
        if output not in OUTPUTS:
            raise ValueError(f"output must be one of {OUTPUTS}")
        # chunk_clients = K: ensemble() runs the round through begin_round() in chunks of K clients
        # (device memory O(K * stride): a round larger than HBM); None: one stack, one launch
        self.chunk_clients = chunk_clients
        self._chunk_packers = None  # the two staging / stack sets of streamed rounds (streaming.py)
        if group is not None and devices is not None and len(devices) > 1:
            raise ValueError("group (one GPU per process) and devices (several GPUs in this process) exclude each other")
        if devices is None:
            devices = [torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())]
        self.devices = [torch.device(d) for d in devices]
        self.device = self.devices[0]
        self.output = output
        self.reorder = reorder  # allow the split-N kernel (not bit-exact; <= 1e-6 normwise)
        self.packer = Packer(self.devices, workers)
        # group: this process is one rank of a column-sharded aggregation (flearn_amd.dist): it
        # packs and reduces only its columns of the fp32 bucket and an RCCL all-gather over xGMI
        # reassembles the global model on every rank.  True = the default process group.
        self.group = None
        self._dist = group is not None
        if self._dist:
            import torch.distributed as dist

            self.group = None if group is True else group
            if not dist.is_initialized():
                raise RuntimeError("group= needs torch.distributed initialised (one process per GPU)")
            self.packer.rank_cols = (dist.get_rank(self.group), dist.get_world_size(self.group))
        self.last_plan: BucketPlan | None = None
        self._wcache = {}  # (device, dtype, bytes) -> device weights: a pageable H2D per round saved

    def _weights(self, nm: Numerics, device) -> torch.Tensor:
        key = (str(device), nm.weights.dtype.str, nm.weights.tobytes())
        t = self._wcache.get(key)
        if t is None:
            if len(self._wcache) >= 64:
                self._wcache.clear()
            w = nm.weights
            if w.dtype == np.float16:  # fa_reduce_f16 takes the float16 weights widened (exact)
                w = w.astype(np.float32)
            t = self._wcache[key] = torch.from_numpy(np.ascontiguousarray(w)).to(device)
        return t

    def _refuse_half(self, plan: BucketPlan, server_opt) -> None:
        """float16 uploads outside what fa_reduce_f16 reproduces raise before anything is queued."""
        if KIND_F16 not in plan.groups:
            return
        if server_opt is not None:
            raise TypeError(f"float16 uploads: the server-fused {getattr(server_opt, 'name', 'optimizer')} step "
                            "runs on fp32 models only (aggregate with AVG and update on the client side)")
        if self._dist or len(self.devices) > 1:
            raise TypeError("float16 uploads: a float16 bucket is not sharded over devices=[...] / group=")

    def begin_round(self, key_lst=None, server_opt=None, chunk_clients: int = 16):
        """One round aggregated as it arrives (streaming.RoundAccumulator): `add(upload)` per
        {"agg_weight", "params"} dict, folded in chunks of chunk_clients clients, then `finish()`,
        which returns what `ensemble` returns for the same uploads, bit for bit."""
        return RoundAccumulator(self, key_lst, server_opt, chunk_clients)

    def _ensemble_chunked(self, agg_weight_lst, w_local_lst, key_lst, server_opt):
        if len(w_local_lst) == 0 or len(agg_weight_lst) == 0 or len(agg_weight_lst) != len(w_local_lst):
            make_plan(agg_weight_lst, w_local_lst, key_lst)  # raises what the one-launch path raises
        # the whole list is here: the reference's key intersection (strategy.py:119-121) as ever
        # (and its length: no chunk stack taller than the round)
        acc = self.begin_round(select_keys(w_local_lst, key_lst), server_opt, min(self.chunk_clients, len(w_local_lst)))
        for a, w in zip(agg_weight_lst, w_local_lst):
            acc.add({"agg_weight": a, "params": w})
        return acc.finish()

    def ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt: ServerOptimizer | None = None):
        if self.chunk_clients is not None:
            return self._ensemble_chunked(agg_weight_lst, w_local_lst, key_lst, server_opt)
        plan = make_plan(agg_weight_lst, w_local_lst, key_lst)
        self.last_plan = plan
        self._refuse_half(plan, server_opt)
        if server_opt is None and not self._dist and len(self.devices) == 1 and self.output != "device":
            glob = self._small_round(plan, w_local_lst)
            if glob is not None:
                return glob
        stacks = self.packer.pack(plan, w_local_lst)
        results = self._server_step(plan, stacks, server_opt)
        for kind, parts in stacks.items():
            if self.packer.last_row_tables.get(kind) == "slab":  # the caller's memory, read in place:
                self.packer.hold([st for _, st in parts], parts[0][0].device)  # alive until read
        if self._dist and KIND_F32 in results:
            results[KIND_F32] = self._gather_columns(plan, results[KIND_F32])
        return self._finish(plan, results)

    # -- robust rounds: coordinate-wise trimmed mean and median ----------------------------------
    def ensemble_trimmed(self, w_local_lst, trim: int, key_lst=None, server_opt: ServerOptimizer | None = None):
        """The coordinate-wise trimmed mean of the uploads (Yin et al., ICML 2018): per element, the
        N clients' values in IEEE totalOrder, the `trim` smallest and the `trim` largest dropped, the
        rest summed in ascending order in the bucket's sum type and divided by N - 2 * trim (the
        median is trim = (N - 1) // 2).  There are no weights: a client cannot buy influence with
        its own agg_weight, and the result does not depend on the order of the uploads.  The plan is
        make_plan's for Python-int weights (key intersection, layouts and errors as in `ensemble`),
        the uploads are packed as ever (host, device, slab), fa_trim_sum makes each bucket's sums,
        and the server step — the divide, a fused AVGM / OPT update, the three output modes — is
        the one a streamed round ends in.

        Refused before anything is queued: float16 buckets and FedDyn state (TypeError: its h
        update needs the plain sum over all N); several devices, group= and chunk_clients
        (ValueError: every client must be present for a column's order statistics); more than
        128 clients and a trim outside 0 <= 2 * trim < N (ValueError)."""
        if self.chunk_clients is not None:
            raise ValueError("a robust round needs every client at once: chunk_clients is not supported")
        if self._dist:
            raise ValueError("a robust round is not sharded over a process group (group=)")
        if len(self.devices) > 1:
            raise ValueError("a robust round runs on one device: devices=[...] with several devices is not supported")
        if isinstance(server_opt, DynState):
            raise TypeError("FedDyn's h update needs the plain sum over all clients: no robust round with Dyn state")
        n = len(w_local_lst)
        if n > na.TRIM_MAX_CLIENTS:
            raise ValueError(f"a robust round takes at most {na.TRIM_MAX_CLIENTS} clients, got {n}")
        plan = make_plan([1] * n, w_local_lst, key_lst)
        if KIND_F16 in plan.groups:
            raise TypeError("float16 uploads: a robust round aggregates fp32 / float64 / int64 buckets only")
        if isinstance(trim, bool) or not isinstance(trim, (int, np.integer)) or trim < 0 or 2 * trim >= n:
            raise ValueError(f"trim must be an integer with 0 <= 2 * trim < {n} clients, got {trim!r}")
        trim = int(trim)
        # the divide is by the kept count (the plan is make_plan's cached one: a copy carries it)
        groups = {kind: Group(kind, dataclasses.replace(g.numerics, denom=float(n - 2 * trim)), g.segments, g.stride)
                  for kind, g in plan.groups.items()}
        plan = dataclasses.replace(plan, groups=groups)
        self.last_plan = plan
        stacks = self.packer.pack(plan, w_local_lst)
        sums = {}
        for kind, parts in stacks.items():
            g = plan.groups[kind]
            ((sh, stack),) = parts
            with torch.cuda.device(sh.device):
                if isinstance(stack, RowTable):  # device uploads: the one-launch gather into the stack
                    buf = self.packer.device_bucket(("in", kind, sh.index), (n, g.stride), TORCH_DTYPE[g.store_dtype],
                                                    sh.device)
                    stack.gather_into(buf)
                    stack = buf
                ak = acc_kind_of(kind, g.numerics.mode)
                acc = self.packer.device_bucket(("acc", kind), (g.stride,), _ACC_TORCH[ak], sh.device)
                trim_sum_stack(ak, stack, trim, acc, n_clients=n)
                if self.packer.last_row_tables.get(kind) == "slab":  # the caller's memory, read in place
                    self.packer.hold([stack], sh.device)
            sums[kind] = [(sh, FoldedSum(acc, ak, n, sh.width))]
        return self._finish(plan, self._server_step(plan, sums, server_opt))

    # -- robust rounds: Krum / multi-Krum ---------------------------------------------------------
    def ensemble_krum(self, w_local_lst, f: int, m: int, key_lst=None, server_opt: ServerOptimizer | None = None,
                      center=None):
        """Multi-Krum (Blanchard et al., NeurIPS 2017; Krum is m = 1): the m uploads closest to their
        N - f - 2 nearest neighbours are averaged, the others are left out whole, and `last_krum`
        says which.  The uploads are planned (make_plan for Python-int weights) and packed as ever
        (host, device, slab); the fp32 bucket's client Gram matrix (ops.gram_stack, centred on
        `center`) goes to the host (8 N^2 bytes per run of keys), krum.krum_select picks the uploads,
        and their mean is taken from the device stacks already there — the fp32 bucket through a
        row table of the selected rows' addresses, the 8-byte buckets gathered into a compact stack
        — with unit weights, in upload order: bit-identical to
        ensemble([1] * m, [the selected uploads in upload order], the round's keys, server_opt) — the keys
        common to all N uploads (or key_lst), in the round's order, whoever is selected.

        Distances are measured on the fp32 bucket only: float64 / int64 values (BN counters and the
        like) do not enter them, and are averaged over the selected clients like the rest.
        center: a w_glob-like dict (the server's own state, never a client's upload); its fp32 keys
        are laid out into one fp32 row and subtracted from every upload before the products, which
        keeps the cancellation in G_ii + G_jj - 2 G_ij harmless for models that differ little.

        self.last_krum = {"gram", "scores", "selected", "centered"} (host arrays) is the audit.
        Refused before anything is queued: float16 buckets and FedDyn state (TypeError); several
        devices, group=, chunk_clients, more than 128 clients, bad f / m, and uploads without an
        fp32 bucket to measure distances on (ValueError).  More than f non-finite uploads: ValueError
        after the Gram."""
        if self.chunk_clients is not None:
            raise ValueError("a robust round needs every client at once: chunk_clients is not supported")
        if self._dist:
            raise ValueError("a robust round is not sharded over a process group (group=)")
        if len(self.devices) > 1:
            raise ValueError("a robust round runs on one device: devices=[...] with several devices is not supported")
        if isinstance(server_opt, DynState):
            raise TypeError("FedDyn's h update needs the plain sum over all clients: no robust round with Dyn state")
        n = len(w_local_lst)
        if n > na.GRAM_MAX_CLIENTS:
            raise ValueError(f"a Krum round takes at most {na.GRAM_MAX_CLIENTS} clients, got {n}")
        plan = make_plan([1] * n, w_local_lst, key_lst)
        if KIND_F16 in plan.groups:
            raise TypeError("float16 uploads: a robust round aggregates fp32 / float64 / int64 buckets only")
        f, m = krum.check_counts(n, f, m)
        g32 = plan.groups.get(KIND_F32)
        if g32 is None or not any(s.numel > 0 for s in g32.segments):
            raise ValueError("Krum measures distances on the fp32 bucket, and these uploads have none")
        centre = self._check_center(g32, center)  # refused here, before anything is queued
        self.last_plan = plan
        self.last_krum = None
        stacks = self.packer.pack(plan, w_local_lst)
        dense = {}
        for kind, parts in stacks.items():
            g = plan.groups[kind]
            ((sh, stack),) = parts
            with torch.cuda.device(sh.device):
                if isinstance(stack, RowTable):  # device uploads: the one-launch gather into the stack
                    buf = self.packer.device_bucket(("in", kind, sh.index), (n, g.stride), TORCH_DTYPE[g.store_dtype],
                                                    sh.device)
                    stack.gather_into(buf)
                    stack = buf
            dense[kind] = (sh, stack)
        sh, stack = dense[KIND_F32]
        with torch.cuda.device(sh.device):
            row = self._center_row(g32, centre, sh.device)
            runs = key_runs(g32)
            grams = self.packer.device_bucket(("gram", KIND_F32), (len(runs), n, n), torch.float64, sh.device)
            work = self.packer.device_bucket(("gram_work", KIND_F32), (max(gram_workspace(n, c1 - c0) for c0, c1 in runs),),
                                             torch.uint8, sh.device)
            for i, (c0, c1) in enumerate(runs):
                gram_stack(stack, center=row, n_clients=n, col_begin=c0, n_cols=c1 - c0, out=grams[i], workspace=work)
            host = grams.cpu().numpy()  # the one synchronisation of the round before its result
        gram = host[0].copy()
        for part in host[1:]:  # partial Grams add: in key order, float64
            gram += part
        # (a slab, the caller's memory read in place, needs no hold for the Gram launches: the copy
        # above has waited for them; the selected rows' reduce keeps it through its row table)
        selected, scores = krum.krum_select(gram, f, m)
        self.last_krum = {"gram": gram, "scores": scores, "selected": selected, "centered": row is not None}
        sel = [int(i) for i in selected]
        # The mean of the selected uploads, planned as ensemble([1] * m, ..., the round's keys) plans
        # it.  Over the ROUND's keys in the round's order, never the selected uploads' own: the
        # stack is laid out by the round's plan (upload 0's key order, the keys common to all N),
        # and a left-out upload must not move a column by ordering its dict differently or by
        # lacking a key.
        plan_m = make_plan([1] * m, [w_local_lst[i] for i in sel], list(plan.keys))
        sums = {}
        for kind, (dsh, st) in dense.items():
            gm, g = plan_m.groups.get(kind), plan.groups[kind]
            if gm is None or gm.stride != g.stride or [(s.key, s.offset, s.numel) for s in gm.segments] != [
                    (s.key, s.offset, s.numel) for s in g.segments]:
                raise RuntimeError(f"the selected uploads' {kind} bucket is not laid out as the round's")
            segs = [s for s in gm.segments if s.numel > 0]
            esz = st.element_size()
            ptrs = np.empty((len(segs), m), dtype=np.int64)
            base = np.array([st.data_ptr() + i * st.stride(0) * esz for i in sel], dtype=np.int64)
            for j, s in enumerate(segs):
                ptrs[j] = base + s.offset * esz
            with torch.cuda.device(dsh.device):
                table = RowTable(self.packer, plan_m, gm, segs, ptrs, [st], None, dsh.device)
                if kind == KIND_F32:
                    # rows of a 16-B aligned stack at 64-element offsets: fa_reduce_f32_rows reads them in place
                    if not table.aligned:
                        raise RuntimeError("the fp32 stack's rows are not 16-B aligned")
                    total = table
                else:
                    total = self.packer.device_bucket(("sel", kind), (m, gm.stride), TORCH_DTYPE[gm.store_dtype], dsh.device)
                    table.gather_into(total)
            sums[kind] = [(dsh, total)]
        if set(plan_m.groups) != set(dense):
            raise RuntimeError("the selected uploads' buckets are not the round's")
        self.last_plan = plan_m
        try:
            results = self._server_step(plan_m, sums, server_opt)
        finally:
            for kind, ((dsh, total),) in sums.items():
                if isinstance(total, RowTable):
                    total.release()  # the stack (a slab: the caller's memory) stays alive until the reduce is done
        return self._finish(plan_m, results)

    @staticmethod
    def _check_center(g32: Group, center):
        """[(segment, flat tensor)] of `center`'s fp32 keys, or None; ValueError for a centre that is
        no dict, lacks a key of the bucket or has another element count.  Touches no device."""
        if center is None:
            return None
        if not hasattr(center, "keys"):
            raise ValueError("center must be a w_glob-like dict or None")
        out = []
        for s in g32.segments:
            if s.numel == 0:
                continue
            if s.key not in center:
                raise ValueError(f"center has no key {s.key!r}")
            v = center[s.key]
            v = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
            if v.numel() != s.numel:
                raise ValueError(f"center[{s.key!r}] has {v.numel()} elements, the uploads have {s.numel}")
            out.append((s, v.reshape(-1)))
        return out

    def _center_row(self, g32: Group, centre, device):
        """_check_center's pieces laid out as one fp32 row of the bucket (zeros elsewhere), or None."""
        if centre is None:
            return None
        row = self.packer.device_bucket(("center", KIND_F32), (g32.stride,), torch.float32, device)
        row.zero_()
        for s, v in centre:
            row[s.offset : s.offset + s.numel].copy_(v, non_blocking=False)
        return row

    # -- the server step of a round: one-launch and streamed rounds alike ------------------------
    def _server_step(self, plan: BucketPlan, sums: dict, server_opt) -> dict:
        """Divide every bucket's weighted sum and run the server update.  sums: kind -> [(shard,
        sum)], a sum being an ops.FoldedSum (a streamed round's accumulator) or a client stack still
        to be summed (torch stack or RowTable), which becomes an ops.StackSum with the shard's device
        weights here, right before its launch.  Returns kind -> [(shard, tensor)]."""
        fused = False
        self._post_denom = None
        if server_opt is not None and KIND_F32 in plan.groups:
            if self._dist:
                server_opt.group = (self.group, self.packer.rank_cols[1])
            fused = server_opt.prepare(plan, [sh for sh, _ in sums[KIND_F32]])
        # the split-N kernel reads a torch stack only, and FedDyn's step never asks for it
        reorder = self.reorder and not isinstance(server_opt, DynState)
        results, first_means = {}, {}
        for kind, parts in sums.items():
            g = plan.groups[kind]
            nm = g.numerics
            res = []
            for sh, total in parts:
                with torch.cuda.device(sh.device):
                    if isinstance(total, (torch.Tensor, RowTable)):
                        total = StackSum(total, self._weights(nm, sh.device),
                                         reorder and not isinstance(total, RowTable))
                    if kind == KIND_F32:
                        out = self._mean_f32(nm, sh, total, server_opt, fused, first_means)
                    elif kind == KIND_F16:  # no folded form
                        out = self._reduce_f16(g, sh, total.stack, total.weights)
                    else:
                        out = self.packer.device_bucket(("out64", kind, sh.index), (sh.width,), torch.float64, sh.device)
                        total.mean(nm, nm.denom, out64=out)
                res.append((sh, out))
            results[kind] = res
        if server_opt is not None and first_means:
            server_opt.adopt(plan, [sh for sh, _ in sums[KIND_F32]], first_means)
        return results

    def _mean_f32(self, nm: Numerics, sh, total, server_opt, fused, first_means):
        """The fp32 bucket's server step on one shard: total.mean(...) divides the sum, with the
        update fused where there is one.  A double-buffered state advances only once that call has
        returned: a refused launch leaves it on the pair it had."""
        want64 = self.output == "reference" and nm.out_dtype == _F64
        # column-sharded plain mean with float64 output: gather fp32 sums, divide after
        sums = self._dist and want64 and server_opt is None and nm.mode == na.MODE_W32_DIV64
        if sums:
            self._post_denom = float(nm.denom)
        if sh.width == 0:  # a rank whose column range is empty (tiny model, many ranks)
            if isinstance(server_opt, ServerOptimizer) and not fused:
                first_means[sh.index] = torch.empty(0, dtype=torch.float32, device=sh.device)
            gathers64 = want64 and not sums
            return torch.empty(0, dtype=torch.float64 if gathers64 else torch.float32, device=sh.device)
        if sums:
            out32 = self.packer.device_bucket(("sum32", KIND_F32, sh.index), (sh.width,), torch.float32, sh.device)
            total.mean(nm, 1.0, out32=out32)
            return out32
        out64 = (self.packer.device_bucket(("out64", KIND_F32, sh.index), (sh.width,), torch.float64, sh.device)
                 if want64 else None)
        if isinstance(server_opt, DynState):
            return server_opt.step(self, sh, total, nm, want64)
        if server_opt is not None and fused:
            # fused: fl32(w) becomes the next round's prev (the model clients load), v_t advances;
            # both into the other pair, which becomes the state only once the launch call has returned
            prev, v, prev_o, v_o = server_opt.step_buffers(sh)
            total.mean(nm, nm.denom, out32=prev_o, out64=out64, op=server_opt.op, prev=prev, v=v, v_out=v_o,
                       beta=server_opt.beta, eta=server_opt.eta, tau=server_opt.tau, beta2=server_opt.beta2)
            server_opt.advance(sh)
            return out64 if want64 else prev_o
        out32 = None
        if not want64 or server_opt is not None:
            out32 = self.packer.device_bucket(("out32", KIND_F32, sh.index), (sh.width,), torch.float32, sh.device)
        total.mean(nm, nm.denom, out32=out32, out64=out64)
        if server_opt is not None:
            first_means[sh.index] = out32
        return out64 if want64 else out32

    def _reduce_f16(self, g, sh, stack, w):
        """The float16 bucket: "reference" stores the reference's dtype (float64; float16 / float32 for
        np.float16 / np.float32 weights), "float32" and "device" the float16 values
        load_state_dict ends up with, fl16(fl32(q))."""
        nm = g.numerics
        name, odt = "out16", torch.float16
        if self.output == "reference" and nm.out_dtype == _F64:
            name, odt = "out64", torch.float64
        elif self.output == "reference" and nm.out_dtype == np.float32:
            name, odt = "out32", torch.float32
        out = self.packer.device_bucket((name, KIND_F16, sh.index), (sh.width,), odt, sh.device)
        reduce_stack_f16(stack, w, nm.mode, nm.denom, **{name: out})
        return out

    def _gather_columns(self, plan: BucketPlan, parts):
        """Column-sharded group: every rank's reduced columns -> the whole f32 bucket on every
        rank, one all_gather_into_tensor (RCCL over xGMI; equal padded widths).

        Plain mean in FA_MODE_W32_DIV64 with the reference's float64 output: the ranks reduced
        with W = 1, i.e. they hold the exact fp32 sums acc (fl32(fl64(acc)/1) = acc), so the
        gather moves P*4 bytes instead of P*8, and one 1-client reduce of the gathered sums
        (weight fl32(1.0), W = np.sum(weights)) then computes fl64(acc)/W — the value the
        unsharded kernel's epilogue computes, bit for bit."""
        (sh, out), = parts
        stride = plan.groups[KIND_F32].stride
        full = gather_columns(out[: sh.width], rank_width(stride, self.packer.rank_cols[1]), stride, self.group)
        if self._post_denom is not None:
            out64 = self.packer.device_bucket(("out64_full", KIND_F32), (stride,), torch.float64, self.device)
            one = self._weights(_ONE_W32, self.device)
            reduce_stack(full.view(1, stride), one, na.MODE_W32_DIV64, self._post_denom, out64=out64)
            full = out64
        return [(Shard(0, self.device, 0, stride), full)]

    def _finish(self, plan: BucketPlan, results: dict):
        if self.output == "device":
            return assemble_on_device(plan, results, self.device)
        return self.packer.unpack(plan, results, as_torch=plan.input_kind == "torch")


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


def assemble_on_device(plan: BucketPlan, results: dict, device) -> dict:
    """output="device": the global model as fresh tensors on `device`.  Per bucket kind ONE fresh
    buffer of the bucket's stride is filled with one copy per column shard (a peer copy over
    xGMI for shards on other GPUs; a plain device copy for the local one), and every key is a
    view of it — not one slice copy per (key, shard).  results: kind -> [(shard, tensor)]."""
    device = torch.device(device)
    full = {}
    for kind, parts in results.items():
        dt = parts[0][1].dtype
        buf = torch.empty(plan.groups[kind].stride, dtype=dt, device=device)
        for sh, t in parts:
            buf[sh.c0 : sh.c1].copy_(t[: sh.width], non_blocking=True)
        full[kind] = buf
    glob = {}
    for k in plan.keys:
        s = plan.key_segment[k]
        glob[k] = full[plan.key_group[k]][s.offset : s.offset + s.numel].view(s.shape)
    return glob
