"""The wide robust rules (fa_trim_sum_wide + fa_fold_finish, 129 .. 1024 clients) against the weighted
mean (fa_reduce_f32) on the SAME client stack (measurement tool, not a gate).

    python tools/bench_trim_wide.py [--shapes 129x4194304,...] [--reps 20] [--warmup 3]
                                    [--out profiles/trimwide/bench_trim_wide.json]

tools/bench_trim.py's protocol: one process, values generated on the device, FA_MODE_W32_DIV64 with
the float64 result, the variants timed in turn within every repetition between two device events, 3
warm-up rounds, median of 20.  The default shapes are N = 129, 256, 512 and 1000 at 4 M columns,
N = 1000 at LeNet5's 45,454 padded columns (the cross-device shape), and N = 128, where the variant
`median_default_entry` (fa_trim_sum) runs beside `median` (fa_trim_sum_wide): the same kernel.

Per shape and variant: ms (median, min, max), the kernel and grid fa_last_launch named, the ratio to
the mean's time, the fraction of 8 TB/s on the client bytes N*P*4, and for merge_trim_kernel the ratio
to the time its vector instructions alone take — VALU[NP] instructions per thread and piece (counted
in the compiled gfx950 code), 4 waves per piece, 4 cycles per wave instruction,
1,024 SIMDs, 2.4 GHz.  Before anything is timed the sums of the first 4,096 columns are compared with
tests/robust_ref.py.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]

import robust_ref as rr  # noqa: E402
from flearn_amd import _native as na  # noqa: E402
from flearn_amd import ops  # noqa: E402

PEAK = 8e12  # bytes/s, MI355X HBM3E
VALU = {256: 5668, 512: 8116, 1024: 11049}  # v_* instructions of merge_trim_kernel<NP,true>, one pass of the piece loop
SIMDS, CLOCK, CYCLES = 1024, 2.4e9, 4
DEFAULT_SHAPES = "129x4194304,256x4194304,512x4194304,1000x4194304,1000x45454,128x4194304"
DEFAULT_OUT = REPO / "profiles" / "trimwide" / "bench_trim_wide.json"


def valu_ms(n, p):
    """The issue time of the kernel's vector instructions alone, every SIMD busy."""
    np_ = next(q for q in VALU if q >= n)
    pieces = -(-p // (256 * 128 // np_))
    return pieces * 4 * VALU[np_] * CYCLES / SIMDS / CLOCK * 1e3


def bench_shape(n, p, reps, warmup, dev):
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    w = torch.ones(n, dtype=torch.float32, device=dev)
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    launched = {}

    def robust(name, trim, wide=True):
        def run():
            ops.trim_sum_stack(na.ACC_F32, x, trim, acc, n_cols=p, wide=wide)
            launched.setdefault(name, ops.last_launch()[:2])
            ops.fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc, float(n - 2 * trim), p, out64=o64)
        return run

    def mean():
        ops.reduce_stack(x, w, na.MODE_W32_DIV64, float(n), n_cols=p, out64=o64)
        launched.setdefault("mean", ops.last_launch()[:2])

    t10, tmed = n // 10, (n - 1) // 2
    variants = {"mean": (mean, None), "trimmed_10pct": (robust("trimmed_10pct", t10), t10),
                "median": (robust("median", tmed), tmed)}
    if n <= na.TRIM_MAX_CLIENTS:
        variants["median_default_entry"] = (robust("median_default_entry", tmed, wide=False), tmed)
    cols = min(4096, p)
    for trim in (t10, tmed):
        ops.trim_sum_stack(na.ACC_F32, x, trim, acc, n_cols=cols, wide=True)
        if not rr.same_bits(acc[:cols].cpu().numpy(), rr.trimmed_sum(x[:, :cols].cpu().numpy(), trim)):
            sys.exit(f"fa_trim_sum_wide differs from robust_ref at N = {n}, trim = {trim}")
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
    times = {k: [e0.elapsed_time(e1) for name, e0, e1 in events if name == k] for k in variants}
    base = statistics.median(times["mean"])
    out = {"clients": n, "cols": p, "variants": {}}
    for name, (_, trim) in variants.items():
        ms = statistics.median(times[name])
        v = {"trim": trim, "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
             "kernel": launched[name][0], "grid": launched[name][1], "time_vs_mean": round(ms / base, 3),
             "frac_of_8TBps": round(n * p * 4 / (ms * 1e-3) / PEAK, 4)}
        if v["kernel"].startswith("merge_trim_kernel"):
            v["valu_ms"] = round(valu_ms(n, p), 4)
            v["time_vs_valu"] = round(ms / valu_ms(n, p), 3)
        out["variants"][name] = v
    del x, o64, acc
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_trim_wide.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    res = {"tool": "tools/bench_trim_wide.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "mode": "W32_DIV64, out64; robust = fa_trim_sum_wide + fa_fold_finish, mean = fa_reduce_f32, same stack",
           "valu_model": {"valu_per_thread_and_piece": VALU, "simds": SIMDS, "clock_hz": CLOCK, "cycles_per_wave_instruction": CYCLES},
           "shapes": []}
    for shape in a.shapes.split(","):
        n, p = (int(v) for v in shape.lower().split("x"))
        res["shapes"].append(bench_shape(n, p, a.reps, a.warmup, dev))
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
