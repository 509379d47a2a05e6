"""Device aggregation engine behind Strategy.server_ensemble.

`Aggregator.ensemble(agg_weight_lst, w_local_lst, key_lst)` is the MI355X replacement for
flearn/common/strategy/strategy.py:102-130: plan the buckets (bucketplan.py), copy the uploads into
HBM, run ONE fused reduce launch per bucket kind on torch's current stream, and hand back a
fresh dict with the reference's value types.  `begin_round` aggregates the same round in chunks of
clients (streaming.py); both end in the same server step (`Aggregator._server_step`), fed by
either kind of weighted sum (ops.StackSum, ops.FoldedSum).  The robust rounds, `ensemble_trimmed`
(coordinate-wise trimmed mean and median), `ensemble_krum` (Krum / multi-Krum) and
`ensemble_clipped` (norm clipping), are
robustround.py's, bound on the class; they end in the same server step.  `begin_clipped_round` and
`ensemble_clipped_chunked` (clipstream.py) run the clipped round in chunks of clients;
`ensemble_quantized` (quantround.py) sums int8 block-quantized uploads.

The device-level entry points on torch CUDA tensors are ops.py, the resident optimizer state
(`ServerOptimizer`, `DynState`) serverstate.py, the small-host-round fast path smallround.py; every
name this module defined before it was split is re-exported here as the same object.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as na
from . import clipstream, quantround, robustround, smallround
from .bucketplan import BucketPlan, Shard, key_runs, make_plan, rank_width, select_keys  # noqa: F401
from .dist import gather_columns
from .ops import (FoldedSum, StackSum, _byte_range, _check_arrays, _check_cuda, _check_stack, _check_v_out,  # noqa: F401
                  _check_weights, _check_window, _epilogue, _ptr, _reduce_stack8, apply_dyn, apply_update, fill_uniform,
                  last_launch, mean_tables, reduce_stack, reduce_stack_f16, reduce_stack_f64, reduce_stack_i64,
                  set_reduce_grid)
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
    #: the robust rounds (robustround.py), bound the same way; last_krum: the last Krum round's audit
    ensemble_trimmed = robustround.ensemble_trimmed
    ensemble_krum = robustround.ensemble_krum
    ensemble_clipped = robustround.ensemble_clipped
    #: the streamed clipped / DP-FedAvg round (clipstream.py): any number of clients, a fixed tau
    begin_clipped_round = clipstream.begin_clipped_round
    ensemble_clipped_chunked = clipstream.ensemble_clipped_chunked
    _check_center = staticmethod(robustround._check_center)
    _center_row = robustround._center_row
    last_krum = None
    last_clip = None  # the last clipped round's audit
    #: the round of int8 block-quantized uploads (quantround.py); last_quant: its audit
    ensemble_quantized = quantround.ensemble_quantized
    last_quant = None

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
            self.packer.hold_slab(kind, [st for _, st in parts], parts[0][0].device)
        if self._dist and KIND_F32 in results:
            results[KIND_F32] = self._gather_columns(plan, results[KIND_F32])
        return self._finish(plan, results)

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
