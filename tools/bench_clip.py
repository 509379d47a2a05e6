"""Norm clipping (fa_rownorm2_f32, fa_clip_sum_f32 + fa_fold_finish) against the weighted mean
(fa_reduce_f32) on the SAME client stack (measurement tool, not a gate).

    python tools/bench_clip.py [--shapes 100x25610152,64x25610152,10x25610152] [--reps 20] [--warmup 3]
                               [--out profiles/clip/bench_clip.json]

One process, values generated on the device (fa_fill_uniform_f32), FA_MODE_W32_DIV64 with the
float64 result.  Per shape the variants are timed in turn within every repetition (alternating, so
drift hits all alike), each between two device events, 3 warm-up rounds, median of 20:

    mean              fa_reduce_f32 over the whole stack: the line to compare against
    rownorm           fa_rownorm2_f32 (both kernels)
    clip_0pct         fa_clip_sum_f32 with every scale 1, then fa_fold_finish
    clip_10pct        every tenth row at scale 0.5
    clip_100pct       every row at scale 0.5
    clip_10pct_zero   every tenth row at scale 0 (not read); 100 clients only

Prints and writes one JSON document: per shape and variant ms (median, min, max), the kernel
instantiation and grid fa_last_launch named, GB/s on the client bytes N*P*4, the ratio of its time
to the mean's, the byte floor at 8 TB/s and the derived VALU time (lane operations per element at
256 CUs x 64 lanes x 2.4 GHz); per clip variant also the round's two passes together.  The norms of
the timed stack are compared with a float64 sum and reported as a fraction of the derived bound.
Before anything is timed the first 4,096 columns are checked against tests/clip_ref.py.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import clip_ref as cr  # noqa: E402
from flearn_amd import _native as na  # noqa: E402
from flearn_amd import ops  # noqa: E402

NS = 25610152
PEAK = 8e12  # bytes/s, MI355X HBM3E
VALU = 256 * 64 * 2.4e9  # lane operations per second
DEFAULT_OUT = REPO / "profiles" / "clip" / "bench_clip.json"


def check_against_ref(x, g, n, scales, acc, work):
    cols = min(4096, x.shape[1])
    hx, hg = x[:, :cols].cpu().numpy(), g[:cols].cpu().numpy()
    got = ops.rownorm2_stack(x, center=g, n_cols=cols, workspace=work).cpu().numpy()
    want = cr.norm2(hx, hg)
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    bound = cr.norm_bound(cr.launch_plan(n, cols, cus))
    if not (np.abs(got - want) <= bound * want).all():
        sys.exit(f"fa_rownorm2_f32 misses its bound at N = {n}")
    for name, s in scales.items():
        ops.clip_sum_stack(x, g, s, acc, n_cols=cols)
        if acc[:cols].cpu().numpy().tobytes() != cr.clipped_sum(hx, hg, s.cpu().numpy()).tobytes():
            sys.exit(f"fa_clip_sum_f32 differs from clip_ref at N = {n}, {name}")


def norm_error(x, g, n, p, work):
    """The worst relative error of the device's norms over the timed window, and the derived bound."""
    got = ops.rownorm2_stack(x, center=g, n_cols=p, workspace=work).cpu().numpy()
    grid = ops.last_launch()[1]
    want = np.array([float(((x[i, :p] - g[:p]).double() ** 2).sum()) for i in range(n)])
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    plan = cr.launch_plan(n, p, cus)
    assert plan.grid == grid, (plan.grid, grid)
    err = float((np.abs(got - want) / want).max())
    bound = cr.norm_bound(plan)
    return {"worst_rel_error": err, "derived_bound": bound, "fraction_of_bound": round(err / bound, 4), "chain": plan.chain,
            "grid": plan.grid}


def bench_shape(n, p, reps, warmup, dev):
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    g = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(g, seed=7)
    g = g.reshape(-1)
    w = torch.ones(n, dtype=torch.float32, device=dev)
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    work = torch.empty(ops.rownorm_workspace(n, p), dtype=torch.uint8, device=dev)
    tenth = np.arange(n) % 10 == 0
    patterns = {"clip_0pct": np.ones(n, np.float32), "clip_10pct": np.where(tenth, 0.5, 1.0).astype(np.float32),
                "clip_100pct": np.full(n, 0.5, np.float32)}
    if n == 100:
        patterns["clip_10pct_zero"] = np.where(tenth, 0.0, 1.0).astype(np.float32)
    scales = {k: torch.from_numpy(v).to(dev) for k, v in patterns.items()}
    launched = {}

    def note(name):
        if name not in launched:
            launched[name] = ops.last_launch()[:2]

    def mean():
        ops.reduce_stack(x, w, na.MODE_W32_DIV64, float(n), n_cols=p, out64=o64)
        note("mean")

    def rownorm():
        ops.rownorm2_stack(x, center=g, n_cols=p, out=d2, workspace=work)
        note("rownorm")

    def clip_sum(name):
        def run():
            ops.clip_sum_stack(x, g, scales[name], acc, n_cols=p)
            note(name)
            ops.fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc, float(n), p, out64=o64)
        return run

    variants = {"mean": mean, "rownorm": rownorm, **{k: clip_sum(k) for k in patterns}}
    check_against_ref(x, g, n, scales, acc, work)
    times = {k: [] for k in variants}
    events = []
    for rep in range(warmup + reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if rep >= warmup:
                events.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1))
    base = statistics.median(times["mean"])
    norm_ms = statistics.median(times["rownorm"])
    out = {"clients": n, "cols": p, "byte_floor_ms": round(n * p * 4 / PEAK * 1e3, 4), "variants": {},
           "norm_error": norm_error(x, g, n, p, work)}
    for name in variants:
        ms = statistics.median(times[name])
        rows_read = n if name in ("mean", "rownorm") else int((patterns[name] > 0).sum())
        if name == "mean":
            lane_ops = 2.0 * n  # multiply, add
        elif name == "rownorm":
            lane_ops = 2.0 * n  # subtract, fused multiply-add
        else:
            s = patterns[name]
            lane_ops = float(((s > 0) & (s < 1)).sum()) * 4 + float(((s >= 1) | (s <= 0)).sum())
        rec = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
               "kernel": launched[name][0], "grid": launched[name][1], "GBps": round(rows_read * p * 4 / (ms * 1e-3) / 1e9, 1),
               "frac_of_8TBps": round(rows_read * p * 4 / (ms * 1e-3) / PEAK, 4), "time_vs_mean": round(ms / base, 4),
               "byte_floor_ms": round(rows_read * p * 4 / PEAK * 1e3, 4), "valu_ms": round(lane_ops * p / VALU * 1e3, 4)}
        if name.startswith("clip_"):
            rec["round_ms"] = round(ms + norm_ms, 4)  # the norms' pass and this one
            rec["round_vs_mean"] = round((ms + norm_ms) / base, 4)
        out["variants"][name] = rec
    del x, o64, acc, g
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=f"100x{NS},64x{NS},10x{NS}")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    res = {"tool": "tools/bench_clip.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "mode": "W32_DIV64, out64; clip = fa_clip_sum_f32 + fa_fold_finish, rownorm = fa_rownorm2_f32 (both kernels), "
                   "mean = fa_reduce_f32, same stack",
           "shapes": []}
    for shape in a.shapes.split(","):
        n, p = (int(v) for v in shape.lower().split("x"))
        res["shapes"].append(bench_shape(n, p, a.reps, a.warmup, dev))
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
