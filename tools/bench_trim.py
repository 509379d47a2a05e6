"""The robust rules (fa_trim_sum + fa_fold_finish) against the weighted mean (fa_reduce_f32) on the
SAME client stack (measurement tool, not a gate).

    python tools/bench_trim.py [--shapes 100x25610152,10x25610152,64x25610152] [--reps 20] [--warmup 3]
                               [--out profiles/trim/bench_trim.json]

One process, values generated on the device (fa_fill_uniform_f32), FA_MODE_W32_DIV64 with the
float64 result.  Per shape the variants are timed in turn within every repetition (alternating, so
drift hits all alike), each between two device events, 3 warm-up rounds, median of 20:

    mean            fa_reduce_f32 over the whole stack: the line to compare against
    trimmed_10pct   fa_trim_sum with trim = floor(0.1 N), then fa_fold_finish with denom N - 2 trim
    median          fa_trim_sum with trim = (N - 1) // 2, then fa_fold_finish

Prints and writes one JSON document: per shape and variant ms (median, min, max), the kernel
instantiation and grid fa_last_launch named, GB/s on the client bytes N*P*4, and the ratio of its
time to the mean's.  Before anything is timed the trimmed sums of the first 4,096 columns are
compared with numpy's sort on the host.
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

from flearn_amd import _native as na  # noqa: E402
from flearn_amd import ops  # noqa: E402

NS = 25610152
PEAK = 8e12  # bytes/s, MI355X HBM3E
DEFAULT_OUT = REPO / "profiles" / "trim" / "bench_trim.json"


def check_against_numpy(x, n, trim, acc):
    """Finite data without ties of +-0: totalOrder is np.sort's order, the sum is sequential."""
    cols = min(4096, x.shape[1])
    ops.trim_sum_stack(na.ACC_F32, x, trim, acc, n_cols=cols)
    kept = np.sort(x[:, :cols].cpu().numpy(), axis=0)[trim : n - trim]
    want = kept[0].copy()
    for row in kept[1:]:
        want = want + row
    if acc[:cols].cpu().numpy().tobytes() != want.tobytes():
        sys.exit(f"fa_trim_sum differs from numpy at N = {n}, trim = {trim}")


def bench_shape(n, p, reps, warmup, dev):
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    w = torch.ones(n, dtype=torch.float32, device=dev)
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    launched = {}

    def robust(name, trim):
        def run():
            ops.trim_sum_stack(na.ACC_F32, x, trim, acc, n_cols=p)
            if name not in launched:
                launched[name] = ops.last_launch()[:2]
            ops.fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc, float(n - 2 * trim), p, out64=o64)
        return run

    def mean():
        ops.reduce_stack(x, w, na.MODE_W32_DIV64, float(n), n_cols=p, out64=o64)
        if "mean" not in launched:
            launched["mean"] = ops.last_launch()[:2]

    t10, tmed = n // 10, (n - 1) // 2
    variants = {"mean": (mean, None), "trimmed_10pct": (robust("trimmed_10pct", t10), t10),
                "median": (robust("median", tmed), tmed)}
    for trim in {t10, tmed}:
        check_against_numpy(x, n, trim, acc)
    times = {k: [] for k in variants}
    events = []
    for rep in range(warmup + reps):
        for name, (fn, _) in variants.items():
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
    out = {"clients": n, "cols": p, "variants": {}}
    for name, (_, trim) in variants.items():
        ms = statistics.median(times[name])
        out["variants"][name] = {
            "trim": trim, "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "kernel": launched[name][0], "grid": launched[name][1], "GBps": round(n * p * 4 / (ms * 1e-3) / 1e9, 1),
            "frac_of_8TBps": round(n * p * 4 / (ms * 1e-3) / PEAK, 4), "time_vs_mean": round(ms / base, 4)}
    del x, o64, acc
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=f"100x{NS},10x{NS},64x{NS}")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_trim.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    res = {"tool": "tools/bench_trim.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "mode": "W32_DIV64, out64; robust = fa_trim_sum + fa_fold_finish, mean = fa_reduce_f32, same stack",
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
