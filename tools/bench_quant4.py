"""Int4 block-quantized uploads (fa_deq_fold_q4) against the int8 sum (fa_deq_fold_q8) and the fp32 fold
(fa_fold) over the same elements on the device, and the QuantizedAVG(bits=4) round against
QuantizedAVG() and AVG() rounds from host memory (measurement tool, not a gate).

    python tools/bench_quant4.py [--shape 100x25610152] [--reps 20] [--warmup 3] [--host-clients 100]
                                 [--host-reps 5] [--parts device,host] [--grids 256,384,512,768]
                                 [--out profiles/quant4/bench_quant4.json]

One process.  device: codes, scales and fp32 values generated on the device; the variants are timed in
turn within every repetition (alternating, so drift hits all alike), each between two device events,
3 warm-up rounds, median of 20:

    q4                fa_deq_fold_q4 over the whole uint8 stack (two codes per byte), opening the sum
    q4_center         the same with a centre (delta uploads)
    q4_chain25        the same rows in chunks of 25 through acc_in
    q4_grid<G>        (--grids) q4 under fa_set_reduce_grid(G)
    q8_same_elems     fa_deq_fold_q8 over an int8 stack of the same element count: twice the bytes
    f32_same_elems    fa_fold (FA_ACC_F32) over an fp32 stack of the same element count: 8x the bytes

The goal: q4 takes no longer than q8_same_elems in the same run; the ratio is
reported either way.  Per variant: ms (median, min, max), the instantiation and grid fa_last_launch
named, GiB/s and the fraction of 8 TB/s on the algorithmic bytes (q4: N*P/2 + 4*N*P/128 + 4*P).
Before anything is timed the first 4,096 columns are checked against tests/quant4_ref.py.

host: N ResNet-18 state dicts (flearn_amd.layouts) as numpy uploads; AVG, QuantizedAVG() and
QuantizedAVG(bits=4) .server in the same process, alternating, wall time with the device drained,
median; the H2D bytes of each and the host time of the code pack (quantround._pack_chunk) separately.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tools"))

import quant4_ref as q4r  # noqa: E402
from bench_quant import resnet18_uploads  # noqa: E402
from flearn_amd import _native as na  # noqa: E402
from flearn_amd import ops, quant, quantround  # noqa: E402

PEAK = 8e12  # bytes/s, MI355X HBM3E
GIB = float(1 << 30)
DEFAULT_OUT = REPO / "profiles" / "quant4" / "bench_quant4.json"


def check_against_ref(q, s, w, g, acc):
    cols, n = min(4096, 2 * q.shape[1]), min(q.shape[0], 12)
    hq, hs, hw, hg = q[:n, : cols // 2 + 1].cpu().numpy(), s[:n].cpu().numpy(), w[:n].cpu().numpy(), g[:cols].cpu().numpy()
    for name, c, hc in (("q4", None, None), ("q4_center", g, hg)):
        ops.deq_fold_q4_stack(q, s, w, None, acc, center=c, n_cols=cols, n_clients=n)
        if not q4r.same_bits(acc[:cols].cpu().numpy(), q4r.deq_fold4(None, hq, hs, hw, cols, hc)):
            sys.exit(f"fa_deq_fold_q4 differs from quant4_ref ({name})")


def bench_device(n, p, reps, warmup, dev, grids=()):
    pitch = -(-p // 2048) * 2048
    q4 = torch.randint(0, 256, (n, pitch // 2), dtype=torch.uint8, device=dev)
    s4 = torch.rand((n, pitch // 128), dtype=torch.float32, device=dev) * 0.01 + 1e-6
    q8 = torch.randint(-128, 128, (n, pitch), dtype=torch.int8, device=dev)
    s8 = torch.rand((n, pitch // 1024), dtype=torch.float32, device=dev) * 0.01
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    g = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(g, seed=7)
    g = g.reshape(-1)
    w = torch.rand(n, dtype=torch.float32, device=dev) + 0.5
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    launched = {}

    def timed(name, fn):
        def run():
            fn()
            launched.setdefault(name, ops.last_launch()[:2])
        return run

    def chain():
        for lo in range(0, n, 25):
            hi = min(n, lo + 25)
            ops.deq_fold_q4_stack(q4[lo:hi], s4[lo:hi], w[lo:hi], acc if lo else None, acc, n_cols=p)

    def forced(grid):
        prev = ops.set_reduce_grid(grid)
        try:
            ops.deq_fold_q4_stack(q4, s4, w, None, acc, n_cols=p)
        finally:
            ops.set_reduce_grid(prev)

    variants = {"q4": lambda: ops.deq_fold_q4_stack(q4, s4, w, None, acc, n_cols=p),
                "q4_center": lambda: ops.deq_fold_q4_stack(q4, s4, w, None, acc, center=g, n_cols=p),
                "q4_chain25": chain,
                "q8_same_elems": lambda: ops.deq_fold_stack(q8, s8, w, None, acc, n_cols=p),
                "f32_same_elems": lambda: ops.fold_stack(na.ACC_F32, x, w, None, acc, n_cols=p),
                **{f"q4_grid{gr}": (lambda gr=gr: forced(gr)) for gr in grids}}
    variants = {k: timed(k, f) for k, f in variants.items()}
    check_against_ref(q4, s4, w, g, acc)
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
    q4_bytes = n * (p // 2) + 4 * n * (-(-p // 128)) + 4 * p
    algo = {"q4": q4_bytes, "q4_center": q4_bytes + 4 * p, "q4_chain25": q4_bytes + (-(-n // 25) - 1) * 8 * p,
            "q8_same_elems": n * p + 4 * n * (-(-p // 1024)) + 4 * p, "f32_same_elems": 4 * n * p + 4 * p,
            **{f"q4_grid{gr}": q4_bytes for gr in grids}}
    out = {"clients": n, "cols": p, "variants": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in variants:
        ms = med[name]
        out["variants"][name] = {
            "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "kernel": launched[name][0], "grid": launched[name][1], "algorithmic_bytes": algo[name],
            "GiBps": round(algo[name] / (ms * 1e-3) / GIB, 1), "frac_of_8TBps": round(algo[name] / (ms * 1e-3) / PEAK, 4),
            "byte_floor_ms": round(algo[name] / PEAK * 1e3, 4)}
    out["q4_vs_q8_same_elems"] = round(med["q4"] / med["q8_same_elems"], 4)
    out["q4_vs_f32_same_elems"] = round(med["q4"] / med["f32_same_elems"], 4)
    out["q4_center_vs_q4"] = round(med["q4_center"] / med["q4"], 4)
    out["q4_chain25_vs_q4"] = round(med["q4_chain25"] / med["q4"], 4)
    out["goal_q4_no_slower_than_q8_same_elems"] = bool(med["q4"] <= med["q8_same_elems"])
    return out


def bench_host(n, reps):
    from flearn_amd import AVG, QuantizedAVG

    plain = resnet18_uploads(n)
    ups = {"avg": plain, "avg_q8": [quant.quantize_state_dict(m) for m in plain],
           "avg_q4": [quant.quantize_state_dict(m, bits=4) for m in plain]}
    ups = {k: [{"agg_weight": 1.0, "params": m} for m in v] for k, v in ups.items()}
    strat = {"avg": AVG(output="float32"), "avg_q8": QuantizedAVG(output="float32"),
             "avg_q4": QuantizedAVG(output="float32", bits=4)}
    pack_ms = {"avg_q8": [], "avg_q4": []}
    inner = quantround._pack_chunk
    current = [None]

    def timed_pack(*a):
        t = time.perf_counter()
        r = inner(*a)
        pack_ms[current[0]].append((time.perf_counter() - t) * 1e3)
        return r

    quantround._pack_chunk = timed_pack
    times = {k: [] for k in strat}
    try:
        for rep in range(reps + 1):
            for name, s in strat.items():
                current[0] = name
                torch.cuda.synchronize()
                t = time.perf_counter()
                s.server(ups[name], rep)
                torch.cuda.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t) * 1e3)
    finally:
        quantround._pack_chunk = inner
    f32_bytes = 4 * n * strat["avg"].engine.last_plan.groups["f32"].stride
    med = {k: statistics.median(v) for k, v in times.items()}
    h2d = {"avg": f32_bytes, "avg_q8": strat["avg_q8"].engine.last_quant["bytes_in"],
           "avg_q4": strat["avg_q4"].engine.last_quant["bytes_in"]}
    return {"clients": n, "model": "resnet18", "reps": reps, "output": "float32",
            **{f"{k}_ms": round(v, 2) for k, v in med.items()},
            "avg_q4_vs_avg": round(med["avg_q4"] / med["avg"], 4), "avg_q4_vs_avg_q8": round(med["avg_q4"] / med["avg_q8"], 4),
            "h2d_bytes": h2d, "h2d_ms_at_55GBps": {k: round(v / 55e9 * 1e3, 2) for k, v in h2d.items()},
            "pack_ms": {k: round(statistics.median(v[1:] or v), 2) for k, v in pack_ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100x25610152")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-clients", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--parts", default="device,host")
    ap.add_argument("--grids", default="", help="device: also time q4 under these forced grids (fa_set_reduce_grid), e.g. 256,512")
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_quant4.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    parts = a.parts.split(",")
    res = {"tool": "tools/bench_quant4.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev)}
    if "device" in parts:
        n, p = (int(v) for v in a.shape.lower().split("x"))
        res["device_sum"] = bench_device(n, p, a.reps, a.warmup, dev, [int(v) for v in a.grids.split(",") if v])
        torch.cuda.empty_cache()
    if "host" in parts:
        res["host_round"] = bench_host(a.host_clients, a.host_reps)
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
