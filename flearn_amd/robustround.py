"""The robust rounds of the engine, bound on Aggregator as `ensemble_trimmed`, `ensemble_krum` and
`ensemble_clipped`.

All need every client at once, on one device, with unit weights: they share their refusals
(`_refuse`, `_plan_unit_weights`), pack the uploads as ever, take each bucket as one dense
[N, stride] stack (Packer.dense_stack) and end in the server step every round ends in
(Aggregator._server_step).  The trimmed round makes each bucket's sums with ops.trim_sum_stack; the
Krum round is three steps: `client_gram` (ops.gram_stack per run of keys, to the host),
krum.krum_select, and `selected_sums` (the selected rows, read where they are).  The clipped round
measures each client's update norm (`client_norm2`: ops.rownorm2_stack per run of keys, to the host),
takes its radius and scales from clip.py and sums the clipped uploads with ops.clip_sum_stack; a
DP-FedAvg round then adds Gaussian noise to that sum (ops.gauss_add).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _native as na
from . import clip, krum, ops
from .bucketplan import TORCH_DTYPE, BucketPlan, Group, key_runs, make_plan
from .rowtable import RowTable
from .semantics import KIND_F16, KIND_F32
from .serverstate import DynState, ServerOptimizer


def _refuse(agg, server_opt) -> None:
    """What no robust round does, refused before the uploads are looked at."""
    if agg.chunk_clients is not None:
        raise ValueError("a robust round needs every client at once: chunk_clients is not supported")
    if agg._dist:
        raise ValueError("a robust round is not sharded over a process group (group=)")
    if len(agg.devices) > 1:
        raise ValueError("a robust round runs on one device: devices=[...] with several devices is not supported")
    if isinstance(server_opt, DynState):
        raise TypeError("FedDyn's h update needs the plain sum over all clients: no robust round with Dyn state")


def _plan_unit_weights(w_local_lst, key_lst, max_clients: int, what: str) -> BucketPlan:
    """make_plan's plan for Python-int weights of 1 (key intersection, layouts and errors as in
    `ensemble`), for at most max_clients uploads and no float16 bucket."""
    n = len(w_local_lst)
    if n > max_clients:
        raise ValueError(f"a {what} round takes at most {max_clients} clients, got {n}")
    plan = make_plan([1] * n, w_local_lst, key_lst)
    if KIND_F16 in plan.groups:
        raise TypeError("float16 uploads: a robust round aggregates fp32 / float64 / int64 buckets only")
    return plan


# -- coordinate-wise trimmed mean and median ---------------------------------------------------
def ensemble_trimmed(agg, w_local_lst, trim: int, key_lst=None, server_opt: ServerOptimizer | None = None):
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
    _refuse(agg, server_opt)
    plan = _plan_unit_weights(w_local_lst, key_lst, na.TRIM_MAX_CLIENTS, "robust")
    n = plan.n_clients
    if isinstance(trim, bool) or not isinstance(trim, (int, np.integer)) or trim < 0 or 2 * trim >= n:
        raise ValueError(f"trim must be an integer with 0 <= 2 * trim < {n} clients, got {trim!r}")
    trim = int(trim)
    # the divide is by the kept count (the plan is make_plan's cached one: a copy carries it)
    groups = {kind: Group(kind, dataclasses.replace(g.numerics, denom=float(n - 2 * trim)), g.segments, g.stride)
              for kind, g in plan.groups.items()}
    plan = dataclasses.replace(plan, groups=groups)
    agg.last_plan = plan
    packer = agg.packer
    stacks = packer.pack(plan, w_local_lst)
    sums = {}
    for kind, parts in stacks.items():
        g = plan.groups[kind]
        sh, stack = packer.dense_stack(plan, kind, parts, n)
        with torch.cuda.device(sh.device):
            ak = ops.acc_kind_of(kind, g.numerics.mode)
            acc = packer.device_bucket(("acc", kind), (g.stride,), ops._ACC_TORCH[ak], sh.device)
            ops.trim_sum_stack(ak, stack, trim, acc, n_clients=n)
            packer.hold_slab(kind, [stack], sh.device)
        sums[kind] = [(sh, ops.FoldedSum(acc, ak, n, sh.width))]
    return agg._finish(plan, agg._server_step(plan, sums, server_opt))


# -- Krum / multi-Krum ---------------------------------------------------------------------------
def ensemble_krum(agg, w_local_lst, f: int, m: int, key_lst=None, server_opt: ServerOptimizer | None = None,
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
    _refuse(agg, server_opt)
    plan = _plan_unit_weights(w_local_lst, key_lst, na.GRAM_MAX_CLIENTS, "Krum")
    n = plan.n_clients
    f, m = krum.check_counts(n, f, m)
    g32 = plan.groups.get(KIND_F32)
    if g32 is None or not any(s.numel > 0 for s in g32.segments):
        raise ValueError("Krum measures distances on the fp32 bucket, and these uploads have none")
    centre = _check_center(g32, center)  # refused here, before anything is queued
    agg.last_plan = plan
    agg.last_krum = None
    stacks = agg.packer.pack(plan, w_local_lst)
    dense = {kind: agg.packer.dense_stack(plan, kind, parts, n) for kind, parts in stacks.items()}
    gram = client_gram(agg, plan, dense, centre)
    # (a slab, the caller's memory read in place, needs no hold for the Gram launches: client_gram's
    # copy to the host has waited for them; the selected rows' reduce keeps it through its row table)
    selected, scores = krum.krum_select(gram, f, m)
    agg.last_krum = {"gram": gram, "scores": scores, "selected": selected, "centered": centre is not None}
    sel = [int(i) for i in selected]
    # The mean of the selected uploads, planned as ensemble([1] * m, ..., the round's keys) plans
    # it.  Over the ROUND's keys in the round's order, never the selected uploads' own: the
    # stack is laid out by the round's plan (upload 0's key order, the keys common to all N),
    # and a left-out upload must not move a column by ordering its dict differently or by
    # lacking a key.
    plan_m = make_plan([1] * m, [w_local_lst[i] for i in sel], list(plan.keys))
    sums = selected_sums(agg, plan, plan_m, dense, sel)
    agg.last_plan = plan_m
    try:
        results = agg._server_step(plan_m, sums, server_opt)
    finally:
        for ((_, total),) in sums.values():
            if isinstance(total, RowTable):
                total.release()  # the stack (a slab: the caller's memory) stays alive until the reduce is done
    return agg._finish(plan_m, results)


# -- norm clipping ------------------------------------------------------------------------------
_NOISE_AUDIT = ("noise_multiplier", "sigma", "seed", "sequence")  # clip.check_noise's tuple, as last_clip names it


def ensemble_clipped(agg, w_local_lst, tau, quantile, key_lst=None, server_opt: ServerOptimizer | None = None,
                     center=None, noise_multiplier=None, seed=None, sequence=0):
    """The mean of the uploads after each client's update x_i - g has been projected onto the ball of
    radius tau around `center` (g, the server's own model): norm clipping (Sun et al. 2019; the clipping
    step of McMahan et al. 2018).  Exactly one of tau (a float > 0) and quantile (q in (0, 1]: tau is
    the ceil(q * F)-th smallest of the F finite client norms, Andrew et al. 2021) is given.  No upload
    is left out and no bound on the number of attackers is needed: a scaled upload keeps its direction
    and loses its leverage, and a NaN / inf upload becomes a zero update (the centre), so the global
    model stays finite however many uploads are bad.

    The uploads are planned (make_plan for Python-int weights) and packed as ever (host, device,
    slab).  Only the fp32 bucket is measured and clipped: d2_i = sum_k fl32(x_ik - g_k)^2 per run of
    keys (ops.rownorm2_stack), one copy to the host — the round's one synchronisation —, the radius
    and the scales in float64 there (clip.py), then one ops.clip_sum_stack over the bucket: row i as
    it is where s_i = 1, fl32(g + fl32(s_i * fl32(x - g))) where 0 < s_i < 1, g (the row unread)
    where s_i = 0, summed in list order in fp32 and divided by N in the one server step.  With every
    s_i = 1 the round is bit-identical to ensemble([1] * N, uploads, keys, server_opt).  Float64 /
    int64 buckets (BN counters) do not enter the norm and are averaged over all N clients.
    center=None: no clip, the round is that unit-weight mean itself.

    noise_multiplier > 0 makes the round DP-FedAvg's (McMahan et al. 2018): after
    the clipped sum and before the divide, one ops.gauss_add over the whole stride adds
    fl32(sigma * z) to every column of the SUM, sigma = fl32(noise_multiplier * tau) — tau being the
    most one client moves the sum by — and z the standard normal of (seed, sequence, column); the
    mean's noise has standard deviation sigma / N.  Padding columns get noise nobody reads.  The caller
    advances `sequence` once per noised round: the same (seed, sequence) repeats the noise.  With
    noise_multiplier None or 0 nothing is launched and the round is the one above, bit for bit.
    Float64 / int64 buckets (BN counters) are neither measured, clipped nor noised: they are outside
    the guarantee.  So is everything else a guarantee needs — the accounting of (epsilon, delta), the
    sampling of clients — and Philox is a statistical generator, not a cryptographic one.

    self.last_clip = {"norm2", "scale", "tau", "clipped", "replaced", "centered"} (host arrays; clipped:
    the indices with s < 1, replaced: those with s = 0) is the audit; a round called with a
    noise_multiplier also carries "noise_multiplier", "sigma", "seed" and "sequence", all None when no
    noise was added (a multiplier of 0).  Refused before anything is
    queued: float16 buckets and FedDyn state (TypeError); several devices, group=, chunk_clients, more
    than 128 clients, a bad tau / quantile, uploads without an fp32 bucket and a centre lacking a key
    (ValueError); and noise with quantile=, with tau = inf, without a centre, without a seed, or with a
    negative or non-finite multiplier (ValueError, clip.check_noise).  No finite norm under a quantile
    radius: ValueError after the norms."""
    _refuse(agg, server_opt)
    plan = _plan_unit_weights(w_local_lst, key_lst, na.CLIP_MAX_CLIENTS, "clipped")
    n = plan.n_clients
    clip.check_radius(tau, quantile)
    noise = clip.check_noise(noise_multiplier, seed, sequence, tau, quantile, center is not None)
    # a round not asked for noise keeps the audit's six keys; one asked for it with a multiplier of 0 added none
    audit = {} if noise_multiplier is None else dict(zip(_NOISE_AUDIT, noise or (None,) * len(_NOISE_AUDIT)))
    g32 = plan.groups.get(KIND_F32)
    if g32 is None or not any(s.numel > 0 for s in g32.segments):
        raise ValueError("norm clipping measures the fp32 bucket, and these uploads have none")
    centre = _check_center(g32, center)  # refused here, before anything is queued
    agg.last_clip = None
    if centre is None:
        w_glob = agg.ensemble([1] * n, w_local_lst, key_lst, server_opt)
        none = np.empty(0, dtype=np.int64)
        agg.last_clip = {"norm2": None, "scale": None, "tau": None, "clipped": none, "replaced": none.copy(),
                         "centered": False, **audit}
        return w_glob
    agg.last_plan = plan
    packer = agg.packer
    stacks = packer.pack(plan, w_local_lst)
    dense = {kind: packer.dense_stack(plan, kind, parts, n) for kind, parts in stacks.items()}
    sh, stack = dense[KIND_F32]
    with torch.cuda.device(sh.device):
        row = _center_row(agg, g32, centre, sh.device)
        norm2 = client_norm2(agg, g32, stack, row, n, sh.device)
        radius = clip.clip_radius(norm2, tau, quantile)
        scale = clip.clip_scales(norm2, radius)
        agg.last_clip = {"norm2": norm2, "scale": scale, "tau": radius, "clipped": np.flatnonzero(scale < 1.0),
                         "replaced": np.flatnonzero(scale == 0.0), "centered": True, **audit}
        dscale = packer.device_bucket(("clip_scale", KIND_F32), (n,), torch.float32, sh.device)
        dscale.copy_(torch.from_numpy(scale))
        acc = packer.device_bucket(("acc", KIND_F32), (g32.stride,), torch.float32, sh.device)
        # the whole stride in one launch: padding columns hold sums nobody reads
        ops.clip_sum_stack(stack, row, dscale, acc, n_clients=n)
        if noise is not None:  # on the sum, before the divide; the padding's noise is never read
            _, sigma, seed, sequence = noise
            ops.gauss_add(acc, sigma, seed, sequence)
        packer.hold_slab(KIND_F32, [stack], sh.device)
    sums = {KIND_F32: [(sh, ops.FoldedSum(acc, na.ACC_F32, n, sh.width))]}
    for kind, (dsh, st) in dense.items():
        if kind != KIND_F32:  # the plan's unit weights average the 8-byte buckets over all N
            sums[kind] = [(dsh, st)]
    results = agg._server_step(plan, sums, server_opt)
    for kind, (dsh, st) in dense.items():
        if kind != KIND_F32:
            packer.hold_slab(kind, [st], dsh.device)
    return agg._finish(plan, results)


def client_norm2(agg, g32: Group, stack, row, n: int, device) -> np.ndarray:
    """The clients' float64 squared update norms over the fp32 bucket's keys, on the host: one
    ops.rownorm2_stack launch per run of keys (padding columns may hold another layout's values), one
    copy — the round's one synchronisation —, the runs summed in key order."""
    runs = key_runs(g32)
    norms = agg.packer.device_bucket(("norm2", KIND_F32), (len(runs), n), torch.float64, device)
    work_bytes = max(ops.rownorm_workspace(n, c1 - c0) for c0, c1 in runs)
    work = agg.packer.device_bucket(("norm2_work", KIND_F32), (work_bytes,), torch.uint8, device)
    for i, (c0, c1) in enumerate(runs):
        ops.rownorm2_stack(stack, center=row, n_clients=n, col_begin=c0, n_cols=c1 - c0, out=norms[i], workspace=work)
    host = norms.cpu().numpy()
    norm2 = host[0].copy()
    for part in host[1:]:
        norm2 += part
    return norm2


def client_gram(agg, plan: BucketPlan, dense: dict, centre):
    """The clients' float64 [N, N] Gram matrix of the fp32 bucket, on the host: one ops.gram_stack
    launch per run of keys, `centre` (_check_center's pieces, or None) subtracted from every row,
    and the one synchronisation of the round before its result."""
    g32, n = plan.groups[KIND_F32], plan.n_clients
    sh, stack = dense[KIND_F32]
    with torch.cuda.device(sh.device):
        row = _center_row(agg, g32, centre, sh.device)
        runs = key_runs(g32)
        grams = agg.packer.device_bucket(("gram", KIND_F32), (len(runs), n, n), torch.float64, sh.device)
        work_bytes = max(ops.gram_workspace(n, c1 - c0) for c0, c1 in runs)
        work = agg.packer.device_bucket(("gram_work", KIND_F32), (work_bytes,), torch.uint8, sh.device)
        for i, (c0, c1) in enumerate(runs):
            ops.gram_stack(stack, center=row, n_clients=n, col_begin=c0, n_cols=c1 - c0, out=grams[i], workspace=work)
        host = grams.cpu().numpy()
    gram = host[0].copy()
    for part in host[1:]:  # partial Grams add: in key order, float64
        gram += part
    return gram


def same_layout(gm: Group | None, g: Group) -> bool:
    """The selected uploads' bucket has the round's stride and its keys at the round's columns."""
    return gm is not None and gm.stride == g.stride and [(s.key, s.offset, s.numel) for s in gm.segments] == [
        (s.key, s.offset, s.numel) for s in g.segments]


def selected_sums(agg, plan: BucketPlan, plan_m: BucketPlan, dense: dict, sel: list) -> dict:
    """kind -> [(shard, the rows `sel` of the round's dense stack)] for the server step over plan_m:
    the fp32 bucket as a RowTable of the rows' addresses, read in place (the caller releases it),
    the 8-byte buckets gathered into a compact [m, stride] stack."""
    m = len(sel)
    sums = {}
    for kind, (dsh, st) in dense.items():
        gm = plan_m.groups.get(kind)
        if not same_layout(gm, plan.groups[kind]):
            raise RuntimeError(f"the selected uploads' {kind} bucket is not laid out as the round's")
        segs = [s for s in gm.segments if s.numel > 0]
        esz = st.element_size()
        ptrs = np.empty((len(segs), m), dtype=np.int64)
        base = np.array([st.data_ptr() + i * st.stride(0) * esz for i in sel], dtype=np.int64)
        for j, s in enumerate(segs):
            ptrs[j] = base + s.offset * esz
        with torch.cuda.device(dsh.device):
            table = RowTable(agg.packer, plan_m, gm, segs, ptrs, [st], None, dsh.device)
            if kind == KIND_F32:
                # rows of a 16-B aligned stack at 64-element offsets: fa_reduce_f32_rows reads them in place
                if not table.aligned:
                    raise RuntimeError("the fp32 stack's rows are not 16-B aligned")
                total = table
            else:
                total = agg.packer.device_bucket(("sel", kind), (m, gm.stride), TORCH_DTYPE[gm.store_dtype], dsh.device)
                table.gather_into(total)
        sums[kind] = [(dsh, total)]
    if set(plan_m.groups) != set(dense):
        raise RuntimeError("the selected uploads' buckets are not the round's")
    return sums


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


def _center_row(agg, g32: Group, centre, device):
    """_check_center's pieces laid out as one fp32 row of the bucket (zeros elsewhere), or None."""
    if centre is None:
        return None
    row = agg.packer.device_bucket(("center", KIND_F32), (g32.stride,), torch.float32, device)
    row.zero_()
    for s, v in centre:
        row[s.offset : s.offset + s.numel].copy_(v, non_blocking=False)
    return row
