"""fa_reduce_f16 against fa_reduce_f32 on the north-star layout (measurement tool).

    python tools/bench_half.py [--clients 100] [--cols 25610152] [--reps 20] [--warmup 3]

One process, values generated on the device (fa_fill_uniform_f32, cast to float16 on the device).
Variants, timed in turn within every repetition (alternating, so drift hits all alike), each
launch between two device events, 3 warm-up rounds, median of 20:

    h16_numpy_out64 / h16_numpy_out16   FA_MODE_H16_NUMPY, float64 result / float16 result only
    h16_torch_out64 / h16_torch_out16   FA_MODE_H16_TORCH, the same two outputs
    f32_same_elems                      fa_reduce_f32 (W32_DIV64, out64) on the same element count:
                                        twice the bytes — condition (a): h16 must not be slower
    f32_same_bytes                      fa_reduce_f32 on half the columns: the same bytes — (b)

Prints one JSON line: per variant ms/step (median, min, max), GiB/s of the algorithmic bytes
(N*P*s_in + P*s_out) and the fraction of 8 TB/s; and whether condition (a) holds, median against
median.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from flearn_amd import _native as na  # noqa: E402
from flearn_amd import aggregator as agg  # noqa: E402

NS = 25610152
PEAK = 8e12  # bytes/s, MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=100)
    ap.add_argument("--cols", type=int, default=NS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_half.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    n, p = a.clients, a.cols
    pb = p // 2  # (b): the same bytes in fp32
    pitch16 = -(-p // 128) * 128
    pitch32 = -(-p // 64) * 64
    pitchb = -(-pb // 64) * 64

    x32 = torch.empty((n, pitch32), dtype=torch.float32, device=dev)
    agg.fill_uniform(x32, seed=2024)
    x16 = torch.empty((n, pitch16), dtype=torch.float16, device=dev)
    for r in range(n):  # row by row: no second fp32-sized temporary
        x16[r, :p].copy_(x32[r, :p])
    xb = torch.empty((n, pitchb), dtype=torch.float32, device=dev)
    agg.fill_uniform(xb, seed=2025)
    w32 = torch.full((n,), 0.3, dtype=torch.float32, device=dev)  # fl32(0.3): the torch row's weight
    w16 = torch.full((n,), 0.3, dtype=torch.float16, device=dev).float()  # fl16(0.3) widened
    denom = float(n) * 0.3
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    o16 = torch.empty(p, dtype=torch.float16, device=dev)

    variants = {
        "h16_numpy_out64": (lambda: agg.reduce_stack_f16(x16, w16, na.MODE_H16_NUMPY, denom, n_cols=p, out64=o64),
                            n * p * 2 + p * 8),
        "h16_numpy_out16": (lambda: agg.reduce_stack_f16(x16, w16, na.MODE_H16_NUMPY, denom, n_cols=p, out16=o16),
                            n * p * 2 + p * 2),
        "h16_torch_out64": (lambda: agg.reduce_stack_f16(x16, w32, na.MODE_H16_TORCH, denom, n_cols=p, out64=o64),
                            n * p * 2 + p * 8),
        "h16_torch_out16": (lambda: agg.reduce_stack_f16(x16, w32, na.MODE_H16_TORCH, denom, n_cols=p, out16=o16),
                            n * p * 2 + p * 2),
        "f32_same_elems": (lambda: agg.reduce_stack(x32, w32, na.MODE_W32_DIV64, denom, n_cols=p, out64=o64),
                           n * p * 4 + p * 8),
        "f32_same_bytes": (lambda: agg.reduce_stack(xb, w32, na.MODE_W32_DIV64, denom, n_cols=pb, out64=o64),
                           n * pb * 4 + pb * 8),
    }
    times = {k: [] for k in variants}
    events = []
    for rep in range(a.warmup + a.reps):
        for name, (fn, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if rep >= a.warmup:
                events.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1))
    res = {"clients": n, "cols": p, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "variants": {}}
    for name, (_, nbytes) in variants.items():
        ms = statistics.median(times[name])
        res["variants"][name] = {
            "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "bytes": nbytes, "GiBps": round(nbytes / (ms * 1e-3) / 2**30, 1),
            "frac_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 4)}
    v = res["variants"]
    res["condition_a_h16_not_slower_than_f32_same_elems"] = bool(
        v["h16_numpy_out64"]["ms"] <= v["f32_same_elems"]["ms"] and v["h16_numpy_out16"]["ms"] <= v["f32_same_elems"]["ms"])
    res["rate_vs_f32_same_bytes"] = {k: round(v[k]["GiBps"] / v["f32_same_bytes"]["GiBps"], 4)
                                     for k in v if k.startswith("h16_")}
    print(json.dumps(res))
    return 0 if res["condition_a_h16_not_slower_than_f32_same_elems"] else 1


if __name__ == "__main__":
    sys.exit(main())
