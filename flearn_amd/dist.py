"""Multi-GPU aggregation: element-range sharding of the bucket + RCCL all-gather over xGMI.

One process per GPU (torch.distributed, backend "nccl" = RCCL).  The aggregation is independent
per element, so the flattened fp32 bucket is split by COLUMNS: every rank holds its columns of
all N clients and reduces them with the same fused kernel; the only exchange is reassembling the
global model.  Layer-granular sharding (what the north star's wording suggests) would cap
ResNet-18 at ~5x on 8 GPUs because fc/layer4 tensors are up to 20% of the model; columns
balance exactly.

Column layout (block-cyclic, `stripes` stripes of per-rank widths S_c, multiples of 64):
    O_c = S_0 + ... + S_{c-1};  P_pad = W * (S_0 + ... + S_{last})
    stripe c covers global columns [W*O_c, W*(O_c + S_c)); rank r owns [W*O_c + r*S_c, +S_c)
    rank r's local stack is [N, sum S_c]: local column O_c + j <-> global W*O_c + r*S_c + j
so the all-gather of stripe c writes one contiguous range of the global bucket, and stripe c's
gather (on RCCL's stream) overlaps the reduce of stripe c+1 (on the compute stream).
Optionally the plan ends in a REPLICATED tail of `rep` columns, [W*sum(S), W*sum(S) + rep) =
[n_cols - rep, n_cols): every rank holds those columns of all N clients and reduces them itself,
after its stripes, while the last gathers are in flight — redundant compute instead of
communication, worth it where the all-gather, not the reduce, sets the step (few GPUs, one xGMI
link per peer: at G = 2 every GPU receives half the model over ONE link).  The rank's local
columns are then [stripes..., tail]; the tail's results are written straight into the global
bucket (bit-identical on every rank: same data, same kernel, same order).
Optimizer state (prev, v_t) is sharded the same way and never communicated.

The same code runs on the gloo backend (CPU tests, and two processes sharing one GPU on a
1-GPU box, where RCCL refuses two ranks on one device): device tensors are then staged through
host memory around the collective (`all_gather_into`).

Here: the collectives, the double-buffered state and the reducer.  The planner (`ShardPlan`,
`StripeModel`, `plan_shards`, ...) is flearn_amd.shardplan, the one-shot push gather (`PushGather`,
its receive pool) flearn_amd.push; their names are re-exported here, but what tests and probes
replace in the transport (`_IPC`, `_map_peers`, the streams, `_PUSH_ORDER`) must be replaced there.
"""
from __future__ import annotations

import warnings

import torch
import torch.distributed as dist

from .ops import reduce_stack
from .push import (MAX_PUSH_RANKS, PARK_CAP, DeviceBuffer, HipIpc, PushGather, _all_ok, _group_alive,  # noqa: F401
                   _IPC, _LARGEST, _map_peers, _PARKED, _PUSH_ORDER, _RecvPool, _resolve_group, _TRIMMED, _unmap_all,
                   peer_stream, push_order, shutdown_push, side_stream, size_class)
from .shardplan import (ALIGN, CONTENTION_PRIOR, REP_FRACTIONS, ShardPlan, StripeModel, plan_shards,  # noqa: F401
                        plan_stripes, shard_candidates)


def _host_staged(t: torch.Tensor, group) -> bool:
    """gloo cannot be trusted with device tensors for every collective: stage them on the host."""
    return t.device.type != "cpu" and dist.get_backend(group) == "gloo"


def all_gather_into(dst: torch.Tensor, src: torch.Tensor, group=None, async_op: bool = False):
    """dist.all_gather_into_tensor(dst, src), host-staged on gloo for device tensors (then
    synchronous: returns None).  On RCCL it is the collective itself (async when asked)."""
    if not _host_staged(src, group):
        return dist.all_gather_into_tensor(dst, src, group=group, async_op=async_op)
    hsrc = src.detach().to("cpu")
    hdst = torch.empty(dst.shape, dtype=dst.dtype)
    dist.all_gather_into_tensor(hdst, hsrc, group=group)
    dst.copy_(hdst)
    return None


class DoubleBuffer:
    """A state tensor and its twin: a step reads `cur`, writes `other`, and `flip()` — called once
    the launch returned, so a refused step changes nothing — makes what it wrote current (stores
    onto just-loaded lines cost 1-3% per launch, DESIGN.md §4 finding 20).  The twin is allocated
    when `other` is first asked for; buf[i] is buffer i of the pair, `index` the current one's."""

    __slots__ = ("cur", "_other", "index")

    def __init__(self, t: torch.Tensor):
        self.cur, self._other, self.index = t, None, 0

    @property
    def other(self) -> torch.Tensor:
        if self._other is None:
            self._other = torch.empty_like(self.cur)
        return self._other

    def flip(self):
        self.cur, self._other = self.other, self.cur
        self.index ^= 1

    def __getitem__(self, i: int) -> torch.Tensor:
        return self.cur if i == self.index else self.other


class PingPong:
    """Double-buffered state of a fused server step on one rank's columns (FedAVGM / FedOPT):
    step k reads (prev[k % 2], v[k % 2]) and writes the global model and v_t into the other pair
    (two DoubleBuffers).  `out` is where the current step writes the fp32 model (the next step's
    prev); `flip()` advances after every stripe of a step is launched."""

    def __init__(self, prev: torch.Tensor, v: torch.Tensor):
        self.prev, self.v = DoubleBuffer(prev), DoubleBuffer(v)

    @property
    def cur(self) -> int:
        return self.v.index

    @cur.setter
    def cur(self, i: int):
        for buf in (self.prev, self.v):
            if buf.index != i:
                buf.flip()

    @property
    def out(self) -> torch.Tensor:
        return self.prev.other

    def window(self, c0: int, n: int):
        """(prev, v, v_out) of local columns [c0, c0 + n) for the current step."""
        return self.prev.cur[c0 : c0 + n], self.v.cur[c0 : c0 + n], self.v.other[c0 : c0 + n]

    def flip(self):
        self.prev.flip()
        self.v.flip()


class ShardedReducer:
    """Runs one aggregation step on this rank's shard and reassembles the full bucket.

    reduce_fn(col_begin, n_cols, out_slice) reduces local columns [col_begin, +n_cols) into
    out_slice — on a GPU it is the HIP kernel (ops.reduce_stack); the CPU tests inject
    the oracle to check the sharding and gather logic with gloo.
    """

    def __init__(self, plan: ShardPlan, reduce_fn, device, group=None, local_out=None, gather=None, state=None,
                 push: bool | str = False, push_grid: int = 0):
        self.plan = plan
        self.reduce_fn = reduce_fn
        self.device = torch.device(device)
        self.group = group
        # gather=None: all-gather only when there is more than one rank; True forces the
        # collective path (a 1-rank RCCL group exercises the exact multi-GPU call sequence)
        self.gather = plan.world > 1 if gather is None else gather
        # state: the PingPong of a fused optimizer — each step writes into its `out` buffer;
        # local_out may alias the sharded `prev` of a fused optimizer updated in place
        self.state = state
        self._local_out = (None if state is not None else
                           torch.empty(plan.local_stride, dtype=torch.float32, device=self.device)
                           if local_out is None else local_out)
        # the replicated tail goes straight into the global bucket unless its local results are
        # state (a fused optimizer's next prev): then it is reduced locally and copied across
        self._tail_direct = state is None and local_out is None
        # one rank: local columns ARE the global columns, nothing to reassemble
        # push: False (RCCL's all-gather), True / "kernel" (fa_push stores) or "dma" (copy engines):
        # reassemble with direct peer stores (PushGather) into a bucket from the process's receive
        # pool (mapped by the peers once); RuntimeError on every rank if some rank cannot map a peer
        self.pusher = (PushGather(None, group, mode="dma" if push == "dma" else "kernel", cols=plan.full_cols,
                                  device=self.device) if self.gather and push else None)
        self.full = (self.pusher.full if self.pusher is not None else
                     torch.empty(plan.full_cols, dtype=torch.float32, device=self.device) if self.gather else None)
        if self.pusher is not None:
            self.pusher.grid = push_grid

    def release(self):
        """Collective when pushing: after every rank's pushes, the bucket goes back to the receive
        pool.  The tensor step() returned is a view of that bucket: the next pushing job reuses it,
        and shutdown_push frees it — copy a result out before releasing if it must outlive the
        job."""
        if self.pusher is not None:
            self.pusher.close()
            self.pusher = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False

    def __del__(self):
        if getattr(self, "pusher", None) is not None:
            # release() is collective: it cannot run here; the bucket stays taken until
            # shutdown_push frees the pool
            try:
                warnings.warn("ShardedReducer with a push gather dropped without release(): its receive bucket "
                              "stays in use until shutdown_push", ResourceWarning, stacklevel=2)
            except Exception:  # noqa: BLE001 - interpreter shutdown: nothing left to warn
                pass

    @property
    def local_out(self) -> torch.Tensor:
        """Where the current step writes this rank's columns."""
        return self.state.out if self.state is not None else self._local_out

    def step(self) -> torch.Tensor:
        p = self.plan
        works = []
        out = self.local_out
        pg = self.pusher
        if pg is not None:
            pg.begin()
        for c in range(p.stripes):
            lo, sc = p.local_begin(c), p.shard_of(c)
            self.reduce_fn(lo, sc, out[lo : lo + sc])
            if pg is not None:  # this rank's slice of stripe c, into every rank's bucket
                pg.push(out[lo : lo + sc], p.world * lo + p.rank * sc)
            elif self.gather:
                g0 = p.world * lo  # stripe c's contiguous range of the global bucket
                dst = self.full[g0 : g0 + p.world * sc]
                # this module's global, looked up at each call: bench.py's fault injections assign it
                w = all_gather_into(dst, out[lo : lo + sc], group=self.group, async_op=True)
                if w is not None:
                    works.append(w)
        if p.rep:  # the replicated tail, while the last gathers are in flight
            lo, g0 = p.local_stripes, p.padded
            if self.gather and self._tail_direct:
                self.reduce_fn(lo, p.rep, self.full[g0 : g0 + p.rep])
            else:
                self.reduce_fn(lo, p.rep, out[lo : lo + p.rep])
                if self.gather:
                    self.full[g0 : g0 + p.rep].copy_(out[lo : lo + p.rep])
        if self.state is not None:
            self.state.flip()
        if pg is not None:
            pg.end()
        for w in works:
            w.wait()
        return self.full[: p.n_cols] if self.gather else out[: p.n_cols]


def hip_reduce_fn(stack, weights, mode, denom, reorder=False, state: PingPong | None = None, **epilogue):
    """reduce_fn over a device-resident local stack [N, local_cols] with the fused HIP kernel.
    Epilogue state: a PingPong (double-buffered: the step reads its current pair, writes the
    model into out_slice — the PingPong's `out` — and v_t into the other v), or prev / v
    local-column tensors updated in place.  reorder: allow the split-N kernel
    (ops.reduce_stack)."""
    prev, v = epilogue.pop("prev", None), epilogue.pop("v", None)

    def fn(col_begin, n_cols, out_slice):
        kw = dict(epilogue)
        if state is not None:
            p_in, v_in, v_out = state.window(col_begin, n_cols)
            kw.update(prev=p_in, v=v_in, v_out=v_out)
        elif prev is not None:
            kw.update(prev=prev[col_begin : col_begin + n_cols], v=v[col_begin : col_begin + n_cols])
        reduce_stack(stack, weights, mode, denom, col_begin=col_begin, n_cols=n_cols, out32=out_slice, reorder=reorder,
                     **kw)

    return fn


def gather_columns(local: torch.Tensor, width: int, stride: int, group=None) -> torch.Tensor:
    """Reassemble a column-sharded bucket (Aggregator(group=...)): rank r holds columns
    [r*width, r*width + local.numel()) of a `stride`-wide bucket (the last ranks' ranges may be
    short or empty).  One all_gather_into_tensor of `width` padded columns per rank; returns the
    first `stride` columns of the gathered buffer (on every rank)."""
    world = dist.get_world_size(group)
    if local.numel() == width:
        src = local
    else:
        src = torch.zeros(width, dtype=local.dtype, device=local.device)
        src[: local.numel()] = local
    full = torch.empty(world * width, dtype=local.dtype, device=local.device)
    all_gather_into(full, src, group=group)
    return full[:stride]
