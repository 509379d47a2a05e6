"""The wide client Gram matrix (fa_gram_f32_wide, 129 .. 1024 clients) against three lines on the SAME
client stack (measurement tool, not a gate: no time here is a pass/fail criterion).

    python tools/bench_gram_wide.py [--shapes 256x4194304,512x4194304,1000x4194304,1000x45454] [--reps 10]
                                    [--warmup 2] [--out profiles/gramwide/bench_gram_wide.json]

One process, values generated on the device (fa_fill_uniform_f32).  Per shape the variants are timed in
turn within every repetition (alternating, so drift hits all alike), each between two device events,
median of the repetitions after the warm-up rounds:

    mean        fa_reduce_f32 over the whole stack (FA_MODE_W32_DIV64, float64 result)
    gram_wide   fa_gram_f32_wide with a centre row (pair kernel + float64 finish)
    gram_128    fa_gram_f32 on the first 128 rows of the same stack, same centre; `scaled_ms` is its time
                times the ratio of the MFMA flop the two kernels issue
    matmul      torch.matmul(y, y.T) in fp32 on the stack centred beforehand (y is made once, outside
                the timing): the plain library baseline, without the engine's arithmetic contract

Prints and writes one JSON document: per shape and variant ms (median, min, max), for the Gram variants
the MFMA flop issued (the real 32 x 32 tiles of every panel pair over the window rounded up to whole
chunks) per second, and for all the client bytes N * P * 4 per second.  Before anything is timed the
wide Gram of the first 4,096 columns is compared with numpy's float64 product against its derived bound.
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

MFMA_PEAK = 157.3e12  # flop/s, fp32-input MFMA
PEAK = 8e12  # bytes/s, MI355X HBM3E
LC, KC_WIDE, KC_128 = 1024, 64, 128  # kGramLc, kGramWideKc, gram_kc(128)
DEFAULT_SHAPES = "256x4194304,512x4194304,1000x4194304,1000x45454"
DEFAULT_OUT = REPO / "profiles" / "gramwide" / "bench_gram_wide.json"


def wide_flop(n, p):
    tiles, total = -(-n // 32), 0
    for i in range(-(-n // 128)):
        for j in range(i, -(-n // 128)):
            a, b = min(4, tiles - 4 * i), min(4, tiles - 4 * j)
            total += a * (a + 1) // 2 if i == j else a * b
    return total * 32 * 32 * 2 * (-(-p // KC_WIDE) * KC_WIDE)


def check_against_numpy(x, c):
    cols = min(4096, x.shape[1])
    got = ops.gram_stack(x, center=c, n_cols=cols, wide=True).cpu().numpy()
    y = (x[:, :cols].cpu().numpy() - c[:cols].cpu().numpy()[None, :]).astype(np.float32).astype(np.float64)
    chain, u = LC + -(-cols // LC), 2.0 ** -24
    tol = (chain * u / (1 - chain * u) + 2048 * 2.0 ** -52) * (np.abs(y) @ np.abs(y).T)
    if not (np.abs(got - y @ y.T) <= tol).all() or got.tobytes() != np.ascontiguousarray(got.T).tobytes():
        sys.exit(f"fa_gram_f32_wide differs from numpy beyond its bound at N = {x.shape[0]}")
    return float(np.max(np.abs(got - y @ y.T) / tol))


def bench_shape(n, p, reps, warmup, dev):
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    c = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(c, seed=7)
    c = c.view(-1)
    y = x[:, :p] - c[None, :p]
    w = torch.ones(n, dtype=torch.float32, device=dev)
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    g = torch.empty((n, n), dtype=torch.float64, device=dev)
    work = torch.empty(ops.gram_workspace(n, p, wide=True), dtype=torch.uint8, device=dev)
    work128 = torch.empty(ops.gram_workspace(128, p), dtype=torch.uint8, device=dev)
    launched = {}

    def note(name):
        if name not in launched:
            launched[name] = ops.last_launch()[:2]

    def mean():
        ops.reduce_stack(x, w, na.MODE_W32_DIV64, float(n), n_cols=p, out64=o64)
        note("mean")

    def gram_wide():
        ops.gram_stack(x, center=c, n_cols=p, out=g, workspace=work, wide=True)
        note("gram_wide")

    def gram_128():
        ops.gram_stack(x, center=c, n_clients=128, n_cols=p, out=g, workspace=work128)
        note("gram_128")

    variants = {"mean": mean, "gram_wide": gram_wide, "gram_128": gram_128, "matmul": lambda: torch.matmul(y, y.T)}
    ratio = check_against_numpy(x, c)
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
    times = {k: [] for k in variants}
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1))
    flop = {"gram_wide": wide_flop(n, p), "gram_128": 10 * 32 * 32 * 2 * (-(-p // KC_128) * KC_128)}
    out = {"clients": n, "cols": p, "check_4096_cols_max_err_over_bound": float(f"{ratio:.3e}"), "variants": {}}
    for name in variants:
        ms = statistics.median(times[name])
        rows = 128 if name == "gram_128" else n
        rec = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
               "client_GBps": round(rows * p * 4 / (ms * 1e-3) / 1e9, 1)}
        if name in launched:
            rec["kernel"], rec["grid"] = launched[name]
        if name in flop:
            rec["issued_mfma_flop"] = flop[name]
            rec["issued_TFs"] = round(flop[name] / (ms * 1e-3) / 1e12, 2)
            rec["frac_of_157TF"] = round(flop[name] / (ms * 1e-3) / MFMA_PEAK, 4)
        if name == "gram_128":
            rec["scaled_ms"] = round(ms * flop["gram_wide"] / flop["gram_128"], 4)
        if name == "matmul":
            rec["useful_TFs"] = round(2.0 * n * n * p / (ms * 1e-3) / 1e12, 2)
        out["variants"][name] = rec
    out["floor_mfma_ms"] = round(flop["gram_wide"] / MFMA_PEAK * 1e3, 4)
    out["floor_client_bytes_ms"] = round(n * p * 4 / PEAK * 1e3, 4)
    del x, y, o64, work, work128
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gram_wide.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    res = {"tool": "tools/bench_gram_wide.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
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
