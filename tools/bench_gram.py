"""The client Gram matrix (fa_gram_f32) against the weighted mean (fa_reduce_f32) on the SAME client
stack (measurement tool, not a gate: no time here is a pass/fail criterion).

    python tools/bench_gram.py [--shapes 100x25610152,64x25610152,10x25610152] [--reps 20] [--warmup 3]
                               [--out profiles/gram/bench_gram.json]

One process, values generated on the device (fa_fill_uniform_f32).  Per shape the variants are timed
in turn within every repetition (alternating, so drift hits all alike), each between two device
events, 3 warm-up rounds, median of 20:

    mean           fa_reduce_f32 over the whole stack (FA_MODE_W32_DIV64, float64 result): the line
                   to compare against
    gram           fa_gram_f32 without a centre (tile kernel + float64 finish)
    gram_centred   fa_gram_f32 with a centre row

Prints and writes one JSON document: per shape and variant ms (median, min, max), the kernel
instantiation and grid fa_last_launch named, GB/s on the client bytes N*P*4, the ratio of its time
to the mean's, and two derived floors beside each Gram time: the MFMA flop the kernel issues (the
upper 32 x 32 tiles of the padded NP x NP matrix, 2 flop per product, over the window rounded up to
whole LDS chunks) at 157.3 TF, and the client bytes at 8 TB/s; `time_vs_floor` is the time over the
larger of the two.  Before anything is timed the Gram of the first 4,096 columns is compared with
numpy's float64 product of the same float32 values, against the kernel's derived error bound; the
largest |error| / bound of that check is recorded per variant (`check_4096_cols_max_err_over_bound`).
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
MFMA_PEAK = 157.3e12  # flop/s, fp32-input MFMA
LC = 1024  # kGramLc (csrc/fa_geometry.hpp)
DEFAULT_OUT = REPO / "profiles" / "gram" / "bench_gram.json"


def padded(n):
    return -(-n // 32) * 32


def chunk_cols(np_):  # gram_kc (csrc/fa_geometry.hpp)
    return 512 if np_ <= 32 else 256 if np_ <= 64 else 128


def issued_flop(n, p):
    t = padded(n) // 32
    kc = chunk_cols(padded(n))
    return t * (t + 1) // 2 * 32 * 32 * 2 * (-(-p // kc) * kc)


def check_against_numpy(x, c, n):
    """{variant: the largest |error| / bound over the entries} of the first 4,096 columns' Gram."""
    cols = min(4096, x.shape[1])
    ratios = {}
    for centre in (None, c):
        got = ops.gram_stack(x, center=centre, n_cols=cols).cpu().numpy()
        grid = ops.last_launch()[1]
        y = x[:, :cols].cpu().numpy()
        if centre is not None:
            y = (y - centre[:cols].cpu().numpy()[None, :]).astype(np.float32)
        y = y.astype(np.float64)
        chain = LC + -(-cols // LC)
        u = 2.0 ** -24
        tol = (chain * u / (1 - chain * u) + grid * 2.0 ** -52) * (np.abs(y) @ np.abs(y).T)
        if not (np.abs(got - y @ y.T) <= tol).all() or got.tobytes() != np.ascontiguousarray(got.T).tobytes():
            sys.exit(f"fa_gram_f32 differs from numpy beyond its bound at N = {n}, centred = {centre is not None}")
        ratios["gram" if centre is None else "gram_centred"] = float(np.max(np.abs(got - y @ y.T) / tol))
    return ratios


def bench_shape(n, p, reps, warmup, dev):
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    c = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(c, seed=7)
    c = c.view(-1)
    w = torch.ones(n, dtype=torch.float32, device=dev)
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    g = torch.empty((n, n), dtype=torch.float64, device=dev)
    work = torch.empty(ops.gram_workspace(n, p), dtype=torch.uint8, device=dev)
    launched = {}

    def gram(name, centre):
        def run():
            ops.gram_stack(x, center=centre, n_cols=p, out=g, workspace=work)
            if name not in launched:
                launched[name] = ops.last_launch()[:2]
        return run

    def mean():
        ops.reduce_stack(x, w, na.MODE_W32_DIV64, float(n), n_cols=p, out64=o64)
        if "mean" not in launched:
            launched["mean"] = ops.last_launch()[:2]

    variants = {"mean": mean, "gram": gram("gram", None), "gram_centred": gram("gram_centred", c)}
    ratios = check_against_numpy(x, c, n)
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
    floor_mfma, floor_bytes = issued_flop(n, p) / MFMA_PEAK * 1e3, n * p * 4 / PEAK * 1e3
    out = {"clients": n, "cols": p, "padded_clients": padded(n), "issued_mfma_flop": issued_flop(n, p),
           "floor_mfma_ms": round(floor_mfma, 4), "floor_bytes_ms": round(floor_bytes, 4), "variants": {}}
    for name in variants:
        ms = statistics.median(times[name])
        rec = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
               "kernel": launched[name][0], "grid": launched[name][1], "GBps": round(n * p * 4 / (ms * 1e-3) / 1e9, 1),
               "frac_of_8TBps": round(n * p * 4 / (ms * 1e-3) / PEAK, 4), "time_vs_mean": round(ms / base, 4)}
        if name != "mean":
            rec["time_vs_floor"] = round(ms / max(floor_mfma, floor_bytes), 4)
            rec["issued_TFs"] = round(issued_flop(n, p) / (ms * 1e-3) / 1e12, 2)
            rec["check_4096_cols_max_err_over_bound"] = float(f"{ratios[name]:.3e}")
        out["variants"][name] = rec
    del x, o64, work
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
        sys.exit("bench_gram.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    res = {"tool": "tools/bench_gram.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "mode": "gram = fa_gram_f32 (tile kernel + float64 finish), mean = fa_reduce_f32 W32_DIV64 out64, same stack; "
                   "floors: issued MFMA flop / 157.3 TF, client bytes / 8 TB/s",
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
