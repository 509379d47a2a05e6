"""Server-side optimizer state, resident in HBM between rounds.

`ServerOptimizer` keeps the previous global model and the optimizer state v_t and fuses the
FedAVGM / FedOPT update (avgm.py:19-36, opt.py:23-65 — in the reference these run in
client_receive with w_local = the client's weights; here w_local = the previous global model)
into the round's launch, so the server step reads every client byte once and touches the O(P)
state once.  `DynState` does the same for FedDyn's h and theta (dyn.py:10-36).

Both keep flat arrays laid out like the f32 bucket, cut into the column shards of the devices
(or, with a process group, this rank's columns only), double-buffered: a step reads one buffer,
writes the other, and the state advances only once the launch call has returned.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as na
from .bucketplan import BucketPlan, rank_width
from .dist import DoubleBuffer, gather_columns
from .ops import apply_dyn
from .semantics import KIND_F32, Numerics


def _layout_signature(plan: BucketPlan, shards):
    """(segments, shards): what the resident state is bound to between rounds."""
    return (tuple((s.key, s.shape) for s in plan.f32.segments), tuple((sh.device, sh.c0, sh.c1) for sh in shards))


def _flatten(stride: int, dtype, segments, values: dict) -> np.ndarray:
    """values[key] of every segment at its offset of a zeroed stride-wide host array."""
    flat = np.zeros(stride, dtype=dtype)
    for s in segments:
        flat[s.offset : s.offset + s.numel] = np.asarray(values[s.key], dtype=dtype).reshape(-1)
    return flat


def _to_shards(flat: np.ndarray, shards, dtype=None) -> dict:
    """shard index -> the shard's columns of the flat host array as a device tensor."""
    return {sh.index: torch.from_numpy(flat[sh.c0 : sh.c1].copy()).to(sh.device, dtype) for sh in shards}


def _bucket_host(cols, stride: int, group) -> np.ndarray:
    """The per-shard tensors `cols` (in shard order) as one host array over the whole bucket.
    With a column-sharded process group (group, world) every rank holds only its columns: this is
    then a collective (an all-gather) that every rank must call."""
    if group is None:
        return np.concatenate([t.cpu().numpy() for t in cols])
    (loc,) = cols
    pg, world = group
    return gather_columns(loc, rank_width(stride, world), stride, pg).cpu().numpy()


class ServerOptimizer:
    """FedAVGM / FedOPT state for the fused server step.

    op     : "avgm" | "adagrad" | "yogi" | "adam"
    state  : per column shard (one per device), prev (fp32 previous global, flattened like the
             f32 bucket) and v_t (f64, or fp32 when the weights make the reference's w_glob
             float32), resident in HBM and never communicated.
    First round without `init_global`: the update is skipped (the mean is returned), prev is set
    to the fp32 mean and v_t to zeros — the reference has no previous global model either.
    """

    def __init__(self, op: str, beta=0.9, eta=1e-1, tau=1e-9, beta2=0.99):
        if op not in ("avgm", "adagrad", "yogi", "adam"):
            raise ValueError(f"unknown server optimizer {op!r}")
        self.op = na.OP_BY_NAME[op]
        self.name = op
        self.beta, self.eta, self.tau, self.beta2 = beta, eta, tau, beta2
        self.state = {}  # shard index -> (prev, v) DoubleBuffers: the previous global model and v_t
        self._sig = None
        self._pending_init = None
        self._pending_v = None
        self._plan = None  # the bucket plan the state is bound to (the last round's)
        self.group = None  # (process group, world) when bound to a column-sharded Aggregator

    def init_global(self, glob: dict):
        """Set the previous global model (dict of arrays/tensors); v_t is reset to zeros."""
        self._pending_init = {k: _host_array(v) for k, v in glob.items()}
        self._pending_v = None
        self.state, self._sig = {}, None

    def set_v_t(self, v_t: dict):
        """Restore v_t — the dict `v_t()` returns (keyed like w_glob, f64, or fp32 when the
        weights make w_glob float32) — for the next fused round.  Follows `init_global` (or
        `load_state`): the state a restarted server needs is the previous global model AND v_t
        (avgm.py:28-32 / opt.py:45-60 keep v_t across rounds).  Applied when the next round binds
        the state to its bucket; a key of the model that v_t lacks, or a shape that differs,
        raises there (KeyError / ValueError)."""
        if self._pending_init is None:
            raise RuntimeError("set_v_t restores v_t next to a previous global model: call init_global(w_glob) "
                               "first (or load_state)")
        self._pending_v = {k: _host_array(v) for k, v in v_t.items()}

    def load_state(self, state: dict):
        """Restore what `state_dict()` returned ({"w_glob": previous global, "v_t": v_t}; without
        "v_t" it is zeros, as after init_global)."""
        self.init_global(state["w_glob"])
        if state.get("v_t") is not None:
            self.set_v_t(state["v_t"])

    def state_dict(self, plan: BucketPlan | None = None) -> dict:
        """{"w_glob": the fp32 previous global model the next fused round starts from, "v_t":
        v_t()} as host arrays keyed like w_glob (plan: the last round's by default): what
        `load_state` restores on a fresh optimizer.  With a column-sharded process group this is a
        collective (two all-gathers)."""
        return {"w_glob": self._host_dict(plan, 0), "v_t": self._host_dict(plan, 1)}

    @staticmethod
    def _signature(plan: BucketPlan, shards):
        return _layout_signature(plan, shards) + (plan.f32.numerics.out_dtype.str,)

    @staticmethod
    def _vdtype(plan):
        return torch.float32 if plan.f32.numerics.out_dtype == np.float32 else torch.float64

    def prepare(self, plan: BucketPlan, shards) -> bool:
        """Bind the state to this plan's f32 bucket.  Returns False when there is no previous
        model yet (first round): the caller then runs a plain mean and calls `adopt`."""
        g = plan.f32
        sig = self._signature(plan, shards)
        if self._pending_init is not None:
            prev = _flatten(g.stride, np.float32, g.segments, self._pending_init)
            vdt = np.float32 if self._vdtype(plan) == torch.float32 else np.float64
            vflat = np.zeros(g.stride, dtype=vdt)
            if self._pending_v is not None:
                for s in g.segments:
                    if s.key not in self._pending_v:
                        raise KeyError(s.key)
                    v = self._pending_v[s.key]
                    if tuple(v.shape) != tuple(s.shape):
                        raise ValueError(f"v_t[{s.key!r}] shape {v.shape} != model shape {tuple(s.shape)}")
                vflat = _flatten(g.stride, vdt, g.segments, self._pending_v)
            self._bind(plan, shards, _to_shards(prev, shards), _to_shards(vflat, shards))
            self._pending_init = self._pending_v = None
            return True
        if self._sig is None:
            return False
        if sig != self._sig:
            raise ValueError("model layout changed between rounds; call init_global() again")
        self._plan = plan
        return True

    def adopt(self, plan: BucketPlan, shards, means: dict):
        """First round: the fp32 mean becomes prev, v_t = 0.  means: shard index -> fp32 tensor."""
        self._bind(plan, shards, {sh.index: means[sh.index][: sh.width].clone() for sh in shards},
                   {sh.index: torch.zeros(sh.width, dtype=self._vdtype(plan), device=sh.device) for sh in shards})

    def _bind(self, plan: BucketPlan, shards, prev: dict, v: dict):
        """New state (fresh double buffers) bound to this plan and these shards."""
        self.state = {sh.index: (DoubleBuffer(prev[sh.index]), DoubleBuffer(v[sh.index])) for sh in shards}
        self._sig, self._plan = self._signature(plan, shards), plan

    def step_buffers(self, sh):
        """(prev, v, prev_out, v_out) of a fused step on shard sh: it reads the current pair and
        writes the other one (double-buffered, DESIGN.md §4 finding 20).  `advance(sh)` makes the
        output pair the state — once the launch call has returned, never before."""
        prev, v = self.state[sh.index]
        return prev.cur, v.cur, prev.other, v.other

    def advance(self, sh):
        prev, v = self.state[sh.index]
        prev.flip()
        v.flip()

    def v_t(self, plan: BucketPlan | None = None) -> dict:
        """The state as the reference exposes it (self.v_t dict of arrays; plan: the last round's by
        default).  With a column-sharded process group (Aggregator(group=...)) every rank holds
        only its columns: this is then a collective (an all-gather) that every rank must call."""
        return self._host_dict(plan, 1)

    def _host_dict(self, plan: BucketPlan, i: int) -> dict:
        """State i (0: prev, 1: v_t) over the whole bucket, keyed like w_glob."""
        plan = plan if plan is not None else self._plan
        if not self.state or plan is None:
            raise RuntimeError("no server optimizer state yet (no fused round has run)")
        host = _bucket_host([self.state[j][i].cur for j in sorted(self.state)], plan.f32.stride, self.group)
        return {s.key: host[s.offset : s.offset + s.numel].reshape(s.shape).copy() for s in plan.f32.segments}


def _host_array(v):
    return np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)


def _as_host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v


class DynState:
    """FedDyn server state (flearn/common/strategy/dyn.py:10-36), resident in HBM.

    h      : the caller's dict (a model state_dict).  fp32 entries for fp32 model keys live on the
             device as one flat fp32 array per column shard, laid out like the f32 bucket, and are
             updated in place by the fused epilogue; `sync_h()` copies them back into the
             caller's arrays (the reference mutates them in place, dyn.py:26).  Integer entries
             (BN counters) are the keys whose in-place float update numpy refuses: the reference
             skips them (dyn.py:24-31) and so do we — w_glob keeps the plain mean there.
    theta  : per shard, in the precision numpy gives w_glob (f64 for Python-float weights, fp32
             for np.float32 weights); starts as a copy of h (dyn.py:14) and becomes w_glob each
             round (dyn.py:34).
    One launch per round: mean, delta_theta, h, w and theta for every fp32 column.  When h does
    not cover every fp32 key, the mean is computed first and the update is applied to the
    covered column runs only.
    """

    op = na.OP_DYN
    name = "dyn"

    def __init__(self, h, alpha: float = 0.01):
        self.alpha = alpha
        self.h_host = h
        self._theta_init = None if h is None else {k: np.array(_as_host(v), copy=True) for k, v in h.items()}
        self.state = {}  # shard index -> (h fp32, theta DoubleBuffer)
        self._plan = None  # the bucket plan the state is bound to (the last round's)
        self._sig = None
        self._tdt = None
        self._dirty = False
        self._covered = True
        self.dev_keys = ()
        self.skipped = ()
        self.group = None  # (process group, world) when bound to a column-sharded Aggregator

    # -- state management -------------------------------------------------------------------
    def set_h(self, h):
        """Replace h (uploaded at the next round); theta is kept."""
        self.sync_h()
        if self.state:
            self._theta_init = self.theta_host()
        self.h_host, self.state, self._sig = h, {}, None

    def set_theta(self, theta):
        self.sync_h()
        self._theta_init = {k: np.array(_as_host(v), copy=True) for k, v in theta.items()}
        self.state, self._sig = {}, None

    def classify(self, plan: BucketPlan):
        """(device keys, skipped keys) of h for this plan; raises like the reference would."""
        if self.h_host is None:
            raise AttributeError("FedDyn h is None (dyn.py:20 iterates self.h.keys())")
        dev, skip = [], []
        for k, hv in self.h_host.items():
            if k not in plan.key_group:
                raise KeyError(k)  # dyn.py:21: w_glob[k]
            a = _as_host(hv)
            if not isinstance(a, np.ndarray):
                raise NotImplementedError(f"FedDyn h[{k!r}] is a {type(a).__name__}, expected an array")
            if np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_:
                skip.append(k)  # h[k] -= float array raises in numpy: skipped  dyn.py:24-29
                continue
            seg = plan.key_segment[k]
            if plan.key_group[k] != KIND_F32 or a.dtype != np.float32:
                raise NotImplementedError(
                    f"FedDyn h[{k!r}] ({a.dtype}) on a {plan.key_group[k]} key: only fp32 h on fp32 keys runs on the device")
            if tuple(a.shape) != tuple(seg.shape):
                raise ValueError(f"FedDyn h[{k!r}] shape {a.shape} != model shape {seg.shape}")
            dev.append(k)
        return dev, skip

    def prepare(self, plan: BucketPlan, shards) -> bool:
        g = plan.f32
        dev, skip = self.classify(plan)
        tdt = torch.float32 if g.numerics.out_dtype == np.float32 else torch.float64
        sig = _layout_signature(plan, shards) + (tuple(dev),)
        if not self.state:
            segs = [plan.key_segment[k] for k in dev]
            hs = _to_shards(_flatten(g.stride, np.float32, segs, {k: _as_host(self.h_host[k]) for k in dev}), shards)
            th = _to_shards(_flatten(g.stride, np.float64, segs, self._theta_init), shards, tdt)
            self.state = {sh.index: (hs[sh.index], DoubleBuffer(th[sh.index])) for sh in shards}
            self._sig, self._tdt = sig, tdt
        elif sig != self._sig:
            raise ValueError("model layout changed between FedDyn rounds; set h again")
        elif tdt != self._tdt:
            raise TypeError("FedDyn: the weights' type changed between rounds (theta precision)")
        self.dev_keys, self.skipped = tuple(dev), tuple(skip)
        self._covered = len(dev) == len(g.segments)
        self._plan = plan
        return True

    def step(self, agg, sh, total, nm: Numerics, want64: bool):
        """The fused round for one shard over the round's weighted sum `total` (ops.StackSum or
        ops.FoldedSum): returns the output tensor (theta itself for f64)."""
        hs, theta = self.state[sh.index]
        th = theta.cur
        f64 = th.dtype == torch.float64
        self._dirty = True
        if self._covered:
            out32 = None if want64 else agg.packer.device_bucket(("out32", KIND_F32, sh.index), (sh.width,),
                                                                   torch.float32, sh.device)
            # theta double-buffered (read one, write the other, advance once the launch call has
            # returned; DESIGN.md §4 finding 20); h, the caller-visible state synced back by sync_h,
            # stays in place
            th_o = theta.other
            total.mean(nm, nm.denom, out32=out32, out64=th_o if want64 else None, op=na.OP_DYN, v=th, v_out=th_o,
                       h=hs, alpha=self.alpha)
            theta.flip()
            return th_o if want64 else out32
        # partial coverage: mean in theta's precision, then the update on the covered runs
        gbuf = agg.packer.device_bucket(("dyn_g", KIND_F32, sh.index), (sh.width,), th.dtype, sh.device)
        total.mean(nm, nm.denom, out32=None if f64 else gbuf, out64=gbuf if f64 else None)
        for a, b in self._runs(sh):
            gs = gbuf[a:b]
            apply_dyn(gs, hs[a:b], th[a:b], total.n_clients, self.alpha,
                      out64=gs if f64 else None, out32=None if f64 else gs)
        if want64 or not f64:
            return gbuf
        return gbuf.to(torch.float32)

    def _runs(self, sh):
        """Maximal column runs [a, b) of device keys within the shard, shard-relative."""
        segs = sorted((s.offset, s.offset + s.numel) for s in self._plan.f32.segments if s.key in set(self.dev_keys))
        runs = []
        for lo, hi in segs:
            lo, hi = max(lo, sh.c0), min(hi, sh.c1)
            if lo >= hi:
                continue
            if runs and runs[-1][1] == lo - sh.c0:
                runs[-1][1] = hi - sh.c0
            else:
                runs.append([lo - sh.c0, hi - sh.c0])
        return runs

    # -- host views ---------------------------------------------------------------------------
    def _host_flat(self, i):
        """State i (0: h, 1: theta) over the whole bucket.  With a column-sharded process group
        every rank holds only its columns: this is then a collective (an all-gather) that every
        rank must call — reading `Dyn.h`, `set_h`, `set_theta` included."""
        cols = [self.state[j][i] if i == 0 else self.state[j][i].cur for j in sorted(self.state)]
        return _bucket_host(cols, self._plan.f32.stride, self.group)

    def sync_h(self):
        """Copy the device h into the caller's arrays (in place) and return the dict."""
        if self._dirty and self.state:
            flat = self._host_flat(0)
            for k in self.dev_keys:
                s = self._plan.key_segment[k]
                val = flat[s.offset : s.offset + s.numel].reshape(s.shape)
                dst = self.h_host[k]
                if isinstance(dst, torch.Tensor):
                    dst.copy_(torch.from_numpy(val))
                else:
                    np.copyto(dst, val)
            self._dirty = False
        return self.h_host

    def theta_host(self) -> dict:
        flat = self._host_flat(1)
        out = dict(self._theta_init)
        for k in self.dev_keys:
            s = self._plan.key_segment[k]
            out[k] = flat[s.offset : s.offset + s.numel].reshape(s.shape).copy()
        return out
