"""bfloat16 uploads (fa_fold_bf16) against the fp32 fold (fa_fold) on the device, and the BF16AVG
round against the AVG round from host memory (measurement tool, not a gate).

    python tools/bench_bf16.py [--shape 100x25610176] [--reps 20] [--warmup 3] [--host-clients 100] [--host-reps 5]
                               [--parts device,host] [--grids 256] [--alt-lib build/libfa_bf16_scalar.so]
                               [--out profiles/bf16/bench_bf16.json]

One process.  device: bit patterns and fp32 values generated on the device; the variants are timed in
turn within every repetition (alternating, so drift hits all alike), each between two device events,
3 warm-up rounds, median of 20:

    bf16              fa_fold_bf16 over the whole stack, opening the sum
    bf16_chain25      the same rows in chunks of 25 through acc_in
    bf16_grid<G>      (--grids) bf16 under fa_set_reduce_grid(G)
    bf16_alt          (--alt-lib) fa_fold_bf16 of another build of csrc/fa_bf16.hip alone, linked as a shared
                      library of its own (the unit compiled without packed fp32 operations, say)
    f32_same_elems    (a) fa_fold (FA_ACC_F32) over an fp32 stack of the same element count: 2x the bytes
    f32_same_bytes    (b) fa_fold over a window of that stack of the same BYTE count: half the columns

Reported per variant: ms (median, min, max), the instantiation and grid fa_last_launch named, GiB/s and
the fraction of 8 TB/s on the algorithmic bytes (bf16: 2*N*P + 4*P).  Before anything is timed the
first 4,096 columns of every bf16 variant are checked against tests/bf16_ref.py.

host: N ResNet-18 state dicts (flearn_amd.layouts) as numpy uploads and as bfloat16 wire entries;
BF16AVG().server against AVG().server in the same process, alternating, wall time with the device
drained, median; the H2D bytes of each and the host time of the row pack separately.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import bf16_ref as br  # noqa: E402
from flearn_amd import _native as na  # noqa: E402
from flearn_amd import bf16, bf16round, layouts, ops  # noqa: E402

PEAK = 8e12  # bytes/s, MI355X HBM3E
GIB = float(1 << 30)
DEFAULT_OUT = REPO / "profiles" / "bf16" / "bench_bf16.json"


def alt_entry(path):
    """fa_fold_bf16 of another shared library, with the product's prototype."""
    fn = ctypes.CDLL(str(path)).fa_fold_bf16
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    fn.argtypes, fn.restype = [P, I64, ctypes.c_int32, P, P, P, I64, I64, P], ctypes.c_int
    return fn


def bench_device(n, p, reps, warmup, dev, grids=(), alt=None):
    pitch = -(-p // 64) * 64
    u = torch.randint(-(1 << 15), 1 << 15, (n, pitch), dtype=torch.int16, device=dev)
    u &= ~torch.tensor(0x4000, dtype=torch.int16, device=dev)  # exponents below 2^1: finite values, no NaN
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    w = torch.rand(n, dtype=torch.float32, device=dev) + 0.5
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    half = (p // 2) // 64 * 64
    launched = {}

    def note(name):
        launched.setdefault(name, ops.last_launch()[:2])

    def fold(cols=p, rows=n):
        ops.fold_bf16_stack(u, w, None, acc, n_cols=cols, n_clients=rows)
        note("bf16")

    def chain(cols=p, rows=n):
        for lo in range(0, rows, 25):
            hi = min(rows, lo + 25)
            ops.fold_bf16_stack(u[lo:hi], w[lo:hi], acc if lo else None, acc, n_cols=cols)
        note("bf16_chain25")

    def forced(grid):
        def run(cols=p, rows=n):
            prev = ops.set_reduce_grid(grid)
            try:
                ops.fold_bf16_stack(u, w, None, acc, n_cols=cols, n_clients=rows)
            finally:
                ops.set_reduce_grid(prev)
            note(f"bf16_grid{grid}")
        return run

    def other(cols=p, rows=n):
        rc = alt(u.data_ptr(), u.stride(0), rows, w.data_ptr(), None, acc.data_ptr(), 0, cols, na.stream_handle(dev))
        if rc:
            sys.exit(f"the alternative library's fa_fold_bf16 returned {rc}")
        launched.setdefault("bf16_alt", (None, None))

    def f32(cols, name):
        def run():
            ops.fold_stack(na.ACC_F32, x, w, None, acc, n_cols=cols)
            note(name)
        return run

    bfs = {"bf16": fold, "bf16_chain25": chain, **{f"bf16_grid{g}": forced(g) for g in grids}, **({"bf16_alt": other} if alt else {})}
    cols, rows = min(4096, p), min(n, 30)
    want = br.fold(None, u[:rows, :cols].cpu().numpy().view(np.uint16), w[:rows].cpu().numpy())
    for name, fn in bfs.items():
        fn(cols, rows)
        if not br.same_bits(acc[:cols].cpu().numpy(), want):
            sys.exit(f"{name} differs from bf16_ref")
    launched.clear()
    variants = {**bfs, "f32_same_elems": f32(p, "f32_same_elems"), "f32_same_bytes": f32(half, "f32_same_bytes")}
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
    b = 2 * n * p + 4 * p
    algo = {k: b for k in bfs}
    algo.update({"bf16_chain25": b + (-(-n // 25) - 1) * 8 * p, "f32_same_elems": 4 * n * p + 4 * p,
                 "f32_same_bytes": 4 * n * half + 4 * half})
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"clients": n, "cols": p, "same_bytes_cols": half, "variants": {}}
    for name in variants:
        ms = med[name]
        out["variants"][name] = {
            "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "kernel": launched[name][0], "grid": launched[name][1], "algorithmic_bytes": algo[name],
            "GiBps": round(algo[name] / (ms * 1e-3) / GIB, 1), "frac_of_8TBps": round(algo[name] / (ms * 1e-3) / PEAK, 4)}
    for k in variants:
        if k != "f32_same_elems":
            out[f"{k}_vs_f32_same_elems"] = round(med[k] / med["f32_same_elems"], 4)
    out["bf16_vs_f32_same_bytes"] = round(med["bf16"] / med["f32_same_bytes"], 4)
    del u, x, acc
    torch.cuda.empty_cache()
    return out


def bench_host(n, reps):
    from flearn_amd import AVG, BF16AVG

    layout = layouts.get("resnet18")
    base = np.random.default_rng(1).standard_normal(layouts.fp32_elems(layout)).astype(np.float32)
    plain = [layouts.synthetic_state_dict(layout, base * np.float32(1.0 + 1e-3 * i), counter=i) for i in range(n)]
    t0 = time.perf_counter()
    narrow = [bf16.encode_state_dict(m) for m in plain]
    encode_ms = (time.perf_counter() - t0) * 1e3 / n
    ups = {"avg": [{"agg_weight": 1.0, "params": m} for m in plain],
           "avg_bf16": [{"agg_weight": 1.0, "params": m} for m in narrow]}
    strat = {"avg": AVG(output="float32"), "avg_bf16": BF16AVG(output="float32")}
    pack_ms = []
    inner = bf16round._pack_chunk

    def timed_pack(*a):
        t = time.perf_counter()
        r = inner(*a)
        pack_ms.append((time.perf_counter() - t) * 1e3)
        return r

    bf16round._pack_chunk = timed_pack
    times = {k: [] for k in strat}
    try:
        for rep in range(reps + 1):
            for name, s in strat.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                s.server(ups[name], rep)
                torch.cuda.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t) * 1e3)
    finally:
        bf16round._pack_chunk = inner
    lb = strat["avg_bf16"].engine.last_bf16
    f32_bytes = 4 * n * strat["avg"].engine.last_plan.groups["f32"].stride
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"clients": n, "model": "resnet18", "reps": reps, "output": "float32",
            "avg_ms": round(med["avg"], 2), "avg_bf16_ms": round(med["avg_bf16"], 2),
            "avg_bf16_vs_avg": round(med["avg_bf16"] / med["avg"], 4),
            "h2d_bytes_avg": f32_bytes, "h2d_bytes_avg_bf16": lb["bytes_in"],
            "bf16_pack_ms": round(statistics.median(pack_ms[1:] or pack_ms), 2),
            "client_encode_ms_per_upload": round(encode_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100x25610176")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-clients", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--parts", default="device,host")
    ap.add_argument("--grids", default="", help="device: also time bf16 under these forced grids (fa_set_reduce_grid)")
    ap.add_argument("--alt-lib", default="", help="device: also time fa_fold_bf16 of this shared library")
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bf16.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    parts = a.parts.split(",")
    res = {"tool": "tools/bench_bf16.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev)}
    if "device" in parts:
        n, p = (int(v) for v in a.shape.lower().split("x"))
        res["device_sum"] = bench_device(n, p, a.reps, a.warmup, dev, [int(v) for v in a.grids.split(",") if v],
                                         alt_entry(a.alt_lib) if a.alt_lib else None)
    if "host" in parts:
        res["host_round"] = bench_host(a.host_clients, a.host_reps)
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
