"""A norm-clipped or DP-FedAvg round aggregated in chunks of clients: `ClippedRoundAccumulator`
(Aggregator.begin_clipped_round) and the whole-list form `ensemble_clipped_chunked`, bound on
Aggregator.

With a fixed radius tau a client's scale depends on its own norm only, and the clipped sum is a
running fp32 sum in list order, so a chunk that continues from the
previous chunk's accumulator (ops.clip_fold_stack) leaves exactly the bits of the one-launch round
(robustround.ensemble_clipped).  The norms chunk exactly too: a client's squared norm does not
depend on which chunk it arrives in.  The round is a streaming.RoundAccumulator with unit weights —
its first-upload layout, its later-upload checks, its two alternating packer sets and its final
plan — whose fp32 bucket is measured and clip-folded where the plain round folds it; float64 / int64
buckets fold as there.  Device memory is O(chunk_clients * stride) whatever the client count, and
the client count is not limited.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as na
from . import clip, ops
from .bucketplan import key_runs, make_plan, select_keys
from .robustround import _NOISE_AUDIT, _center_row, _check_center
from .semantics import KIND_F32
from .serverstate import DynState
from .streaming import RoundAccumulator


class _Measured:
    """A chunk whose norm launches are queued and whose clip fold is still to be: the stack (and the
    packer that made it: a slab stays alive until its fold is queued), the pinned host norms and the
    event recorded behind their copy."""

    __slots__ = ("packer", "group", "stack", "n", "host", "event", "slot")

    def __init__(self, packer, group, stack, n, host, event, slot):
        self.packer, self.group, self.stack, self.n = packer, group, stack, n
        self.host, self.event, self.slot = host, event, slot


class ClippedRoundAccumulator(RoundAccumulator):
    """One clipped round aggregated as it arrives: `add(upload)` per {"agg_weight", "params"} dict,
    then `finish()`, which returns what `Aggregator.ensemble_clipped(uploads, tau, None, ...)` returns
    for the same uploads, bit for bit, for any number of clients.  `agg_weight` is required and
    ignored: the round's weights are Python-int 1.

    Per chunk of at most chunk_clients clients the fp32 bucket's norms are queued
    (ops.rownorm2_stack per run of keys) and copied to pinned host memory behind an event; the
    chunk's clip fold is queued one chunk later, when its norms have long arrived, so the host does
    not wait on work it has just queued: the stream sees norms(0), norms(1), fold(0), norms(2),
    fold(1), ..., fold(last).  The two alternating stack sets make that safe: set (c - 1) % 2 is
    rewritten only by copies queued, on the same stream, behind fold(c - 1).  `lag=False` (a
    measuring aid) folds every chunk right behind its own norms.

    center None: nothing is measured or clipped, the round is the unit-weight streamed mean."""

    _device_tags = RoundAccumulator._device_tags + ("center", "norm2s", "norm2_work", "clip_scale")
    _measured = None  # _fold_bucket's hand-over to _fold_pending: the chunk it has just measured

    def __init__(self, agg, tau, center, key_lst=None, server_opt=None, chunk_clients: int = 16, noise_multiplier=None,
                 seed=None, sequence=0, quantile=None, lag: bool = True):
        if quantile is not None:
            raise ValueError("a streamed round cannot know a quantile of norms it has not seen: give a fixed tau "
                             "(or use ensemble_clipped, which has every client at once)")
        self.tau, _ = clip.check_radius(tau, None)
        if isinstance(server_opt, DynState):
            raise TypeError("FedDyn's h update needs the plain sum over all clients: no clipped round with Dyn state")
        super().__init__(agg, key_lst, server_opt, chunk_clients)  # group=, several devices, chunk_clients < 1
        if self.chunk_clients > na.CLIP_MAX_CLIENTS:
            raise ValueError(f"chunk_clients must be in [1, {na.CLIP_MAX_CLIENTS}]: a chunk is one norm launch, "
                             f"got {chunk_clients}")
        if center is not None and not hasattr(center, "keys"):
            raise ValueError("center must be a w_glob-like dict or None")
        self._noise = clip.check_noise(noise_multiplier, seed, sequence, self.tau, None, center is not None)
        # a round not asked for noise keeps the audit's keys; one asked for it with a multiplier of 0 added none
        self._audit = {} if noise_multiplier is None else dict(zip(_NOISE_AUDIT, self._noise or (None,) * len(_NOISE_AUDIT)))
        self._center_dict = center
        self._centre = None  # _check_center's pieces, at the first upload
        self._row = None  # the centre laid out as one fp32 row of the bucket
        self._lag = bool(lag)
        self._waiting = None  # the _Measured chunk whose fold is not queued yet
        self._norm2, self._scale = [], []  # per chunk, in list order
        self._pins = None  # per stack set: (pinned norms, pinned scales)
        agg.last_clip = None

    # -- uploads ----------------------------------------------------------------------------
    def add(self, upload) -> None:
        upload["agg_weight"]  # required, as in flearn's upload format, and not used
        super().add({"agg_weight": 1, "params": upload["params"]})

    def _first(self, w, params) -> None:
        super()._first(w, params)
        try:
            g32 = make_plan([1], [params], self._keys).groups.get(KIND_F32)  # the round's layout (host only)
            if g32 is None or not any(s.numel > 0 for s in g32.segments):
                raise ValueError("norm clipping measures the fp32 bucket, and these uploads have none")
            self._centre = _check_center(g32, self._center_dict)
        except Exception:
            self._keys = None  # nothing was accepted: the next upload is the first again
            raise

    # -- folding ----------------------------------------------------------------------------
    def _fold_pending(self) -> None:
        super()._fold_pending()  # packs the chunk; _fold_bucket below takes its fp32 stack
        if self._centre is None:
            return
        measured, self._measured = self._measured, None
        if self._lag:
            measured, self._waiting = self._waiting, measured
        if measured is not None:
            self._clip_fold(measured)

    def _fold_bucket(self, packer, g, stack, n: int) -> None:
        if g.kind != KIND_F32 or self._centre is None:
            return super()._fold_bucket(packer, g, stack, n)
        agg, dev, K = self.agg, self.agg.device, self.chunk_clients
        runs = key_runs(g)
        slot = self._chunks % 2
        if self._row is None:
            self._row = _center_row(agg, g, self._centre, dev)
            self._work_bytes = max(ops.rownorm_workspace(K, c1 - c0) for c0, c1 in runs)
            self._pins = [(torch.empty((len(runs) * K,), dtype=torch.float64, pin_memory=True),
                           torch.empty((K,), dtype=torch.float32, pin_memory=True)) for _ in range(2)]
        # robustround.client_norm2's launches: one per run of keys (padding may hold another layout's values)
        norms = agg.packer.device_bucket(("norm2s", KIND_F32, slot), (len(runs), n), torch.float64, dev)
        work = agg.packer.device_bucket(("norm2_work", KIND_F32), (self._work_bytes,), torch.uint8, dev)
        for i, (c0, c1) in enumerate(runs):
            ops.rownorm2_stack(stack, center=self._row, n_clients=n, col_begin=c0, n_cols=c1 - c0, out=norms[i],
                               workspace=work)
        host = self._pins[slot][0][: len(runs) * n].view(len(runs), n)
        host.copy_(norms, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(dev))
        self._measured = _Measured(packer, g, stack, n, host, event, slot)

    def _clip_fold(self, m: _Measured) -> None:
        """The deferred half of a chunk: its norms from the host copy, its scales, its clip fold."""
        agg, dev = self.agg, self.agg.device
        m.event.synchronize()
        host = m.host.numpy()
        norm2 = host[0].copy()
        for part in host[1:]:  # the runs summed in key order, as client_norm2 does
            norm2 += part
        scale = clip.clip_scales(norm2, self.tau)
        self._norm2.append(norm2)
        self._scale.append(scale)
        with torch.cuda.device(dev):
            # a pinned copy per stack set: the copy queued from this one two chunks ago is done (it
            # was queued before the norms whose event has just been waited for)
            pin = self._pins[m.slot][1][: m.n]
            pin.copy_(torch.from_numpy(scale))
            dscale = agg.packer.device_bucket(("clip_scale", KIND_F32), (self.chunk_clients,), torch.float32, dev)
            dscale[: m.n].copy_(pin, non_blocking=True)
            acc = agg.packer.device_bucket(("acc", KIND_F32), (m.group.stride,), torch.float32, dev)
            # the whole stride in one launch: padding columns hold sums nobody reads
            ops.clip_fold_stack(m.stack, self._row, dscale, self._acc.get(KIND_F32), acc, n_clients=m.n)
            self._acc[KIND_F32] = acc
            m.packer.hold_slab(KIND_F32, [m.stack], dev)

    # -- the end of the round -----------------------------------------------------------------
    def finish(self):
        if self._finished:
            raise RuntimeError("finish() was already called: begin a new round")
        agg = self.agg
        if self._weights and self._centre is not None:
            if self._pending:
                self._fold_pending()
            if self._waiting is not None:
                measured, self._waiting = self._waiting, None
                self._clip_fold(measured)
            if self._noise is not None:  # on the sum, before the divide; the padding's noise is never read
                _, sigma, seed, sequence = self._noise
                with torch.cuda.device(agg.device):
                    ops.gauss_add(self._acc[KIND_F32], sigma, seed, sequence)
        w_glob = super().finish()  # an empty round raises here what ensemble_clipped([]) raises
        if self._centre is None:
            none = np.empty(0, dtype=np.int64)
            agg.last_clip = {"norm2": None, "scale": None, "tau": None, "clipped": none, "replaced": none.copy(),
                             "centered": False, "chunks": self._chunks, **self._audit}
        else:
            norm2, scale = np.concatenate(self._norm2), np.concatenate(self._scale)
            agg.last_clip = {"norm2": norm2, "scale": scale, "tau": self.tau, "clipped": np.flatnonzero(scale < 1.0),
                             "replaced": np.flatnonzero(scale == 0.0), "centered": True, "chunks": self._chunks,
                             **self._audit}
        return w_glob


def begin_clipped_round(agg, tau, center, key_lst=None, server_opt=None, chunk_clients: int = 16, noise_multiplier=None,
                        seed=None, sequence=0, *, quantile=None):
    """One norm-clipped (noise_multiplier: DP-FedAvg) round aggregated as it arrives
    (ClippedRoundAccumulator): `add(upload)` per {"agg_weight", "params"} dict, measured and
    clip-folded in chunks of chunk_clients <= 128 clients, then `finish()`, which returns what
    `ensemble_clipped` returns for the same uploads, bit for bit; `last_clip` is its audit plus
    "chunks", for any number of clients.  tau: the fixed radius; center: the server's own model (a
    w_glob-like dict), None for an unclipped unit-weight mean.

    Refused before anything is queued: chunk_clients outside [1, 128], group= and several devices, a
    quantile radius (ValueError: a streamed round cannot know a quantile of norms it has not seen),
    FedDyn state (TypeError), clip.check_noise's refusals; at the first upload: float16 uploads
    (TypeError), uploads without an fp32 bucket and a centre lacking a key (ValueError)."""
    return ClippedRoundAccumulator(agg, tau, center, key_lst, server_opt, chunk_clients, noise_multiplier, seed, sequence,
                                   quantile)


def ensemble_clipped_chunked(agg, w_local_lst, tau, key_lst=None, server_opt=None, center=None, chunk_clients=None,
                             noise_multiplier=None, seed=None, sequence=0, *, quantile=None):
    """`ensemble_clipped` with a fixed tau for a list of any length, in chunks of chunk_clients clients
    (default: the engine's chunk_clients, else 16) through begin_clipped_round: the reference's key
    intersection over the whole list first, then min(chunk_clients, N) clients per chunk."""
    k = chunk_clients if chunk_clients is not None else (16 if agg.chunk_clients is None else agg.chunk_clients)
    acc = begin_clipped_round(agg, tau, center, None, server_opt, k, noise_multiplier, seed, sequence, quantile=quantile)
    if len(w_local_lst) == 0:
        make_plan([], w_local_lst, key_lst)  # raises what the one-launch round raises
    # the whole list is here: the reference's key intersection, and no chunk stack taller than the round
    acc._key_lst = select_keys(w_local_lst, key_lst)
    acc.chunk_clients = min(acc.chunk_clients, len(w_local_lst))
    for w in w_local_lst:
        acc.add({"agg_weight": 1, "params": w})
    return acc.finish()
