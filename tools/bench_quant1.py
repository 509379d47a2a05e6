"""1-bit sign uploads (fa_deq_fold_q1) against the int4 sum (fa_deq_fold_q4) and the fp32 fold (fa_fold)
over the same elements on the device, and the QuantizedAVG(bits=1) round against QuantizedAVG(bits=4) and
AVG() rounds from host memory (measurement tool, not a gate).

    python tools/bench_quant1.py [--shape 100x25610176] [--reps 20] [--warmup 3] [--host-clients 100]
                                 [--host-reps 5] [--parts device,host] [--grids 256,512,768] [--lib PATH]
                                 [--out profiles/quant1/bench_quant1.json]

One process.  device: codes, scales and fp32 values generated on the device; the variants are timed in
turn within every repetition, in list order in even repetitions and in reverse order in odd ones (so
neither drift nor a neighbour's cache state favours one), each between two device events, 3 warm-up
rounds, median of 20:

    q1                fa_deq_fold_q1 over the whole uint8 stack (eight codes per byte), opening the sum
    q1_center         the same with a centre (delta uploads)
    q1_chain25        the same rows in chunks of 25 through acc_in
    q1_grid<G>        (--grids) q1 under fa_set_reduce_grid(G)
    q4_same_elems     fa_deq_fold_q4 over a uint8 stack of the same element count: four times the code bytes
    f32_same_elems    fa_fold (FA_ACC_F32) over an fp32 stack of the same element count: 32x the code bytes

--lib loads another build of the library (the unit rebuilt with -DFA_Q1_DEPTH=8 / 16 / 32: the pipeline
depth is a compile-time constant); one run per build, the q4 and fp32 variants are each run's yardstick.
Per variant: ms (median, min, max), the instantiation and grid fa_last_launch named, GiB/s and the
fraction of 8 TB/s on the algorithmic bytes (q1: N*P/8 + 4*N*P/128 + 4*P).  Before anything is timed the
first 4,096 columns are checked against tests/quant1_ref.py.

host: N ResNet-18 state dicts (flearn_amd.layouts) as numpy uploads; AVG, QuantizedAVG(bits=4) and
QuantizedAVG(bits=1) .server in the same process, in both orders, wall time with the device drained,
median; the H2D bytes of each.
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

import quant1_ref as q1r  # noqa: E402
from bench_quant import resnet18_uploads  # noqa: E402
from flearn_amd import _native as na  # noqa: E402

PEAK = 8e12  # bytes/s, MI355X HBM3E
GIB = float(1 << 30)
DEFAULT_OUT = REPO / "profiles" / "quant1" / "bench_quant1.json"


def check_against_ref(ops, q, s, w, g, acc):
    cols, n = min(4096, 8 * q.shape[1]), min(q.shape[0], 12)
    hq, hs, hw, hg = q[:n, : cols // 8].cpu().numpy(), s[:n].cpu().numpy(), w[:n].cpu().numpy(), g[:cols].cpu().numpy()
    for name, c, hc in (("q1", None, None), ("q1_center", g, hg)):
        ops.deq_fold_q1_stack(q, s, w, None, acc, center=c, n_cols=cols, n_clients=n)
        if not q1r.same_bits(acc[:cols].cpu().numpy(), q1r.deq_fold1(None, hq, hs, hw, cols, hc)):
            sys.exit(f"fa_deq_fold_q1 differs from quant1_ref ({name})")


def bench_device(ops, n, p, reps, warmup, dev, grids=()):
    pitch = -(-p // 2048) * 2048
    q1 = torch.randint(0, 256, (n, pitch // 8), dtype=torch.uint8, device=dev)
    q4 = torch.randint(0, 256, (n, pitch // 2), dtype=torch.uint8, device=dev)
    s = torch.rand((n, pitch // 128), dtype=torch.float32, device=dev) * 0.01 + 1e-6
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    g = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(g, seed=7)
    g = g.reshape(-1)
    w = torch.rand(n, dtype=torch.float32, device=dev) + 0.5
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    launched = {}

    def chain():
        for lo in range(0, n, 25):
            hi = min(n, lo + 25)
            ops.deq_fold_q1_stack(q1[lo:hi], s[lo:hi], w[lo:hi], acc if lo else None, acc, n_cols=p)

    def forced(grid):
        prev = ops.set_reduce_grid(grid)
        try:
            ops.deq_fold_q1_stack(q1, s, w, None, acc, n_cols=p)
        finally:
            ops.set_reduce_grid(prev)

    variants = {"q1": lambda: ops.deq_fold_q1_stack(q1, s, w, None, acc, n_cols=p),
                "q1_center": lambda: ops.deq_fold_q1_stack(q1, s, w, None, acc, center=g, n_cols=p),
                "q1_chain25": chain,
                "q4_same_elems": lambda: ops.deq_fold_q4_stack(q4, s, w, None, acc, n_cols=p),
                "f32_same_elems": lambda: ops.fold_stack(na.ACC_F32, x, w, None, acc, n_cols=p),
                **{f"q1_grid{gr}": (lambda gr=gr: forced(gr)) for gr in grids}}
    check_against_ref(ops, q1, s, w, g, acc)
    times = {k: [] for k in variants}
    events = []
    for rep in range(warmup + reps):
        order = list(variants) if rep % 2 == 0 else list(variants)[::-1]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            variants[name]()
            e1.record()
            launched.setdefault(name, ops.last_launch()[:2])
            if rep >= warmup:
                events.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1))
    scale_bytes = 4 * n * (-(-p // 128))
    q1_bytes = n * (p // 8) + scale_bytes + 4 * p
    algo = {"q1": q1_bytes, "q1_center": q1_bytes + 4 * p, "q1_chain25": q1_bytes + (-(-n // 25) - 1) * 8 * p,
            "q4_same_elems": n * (p // 2) + scale_bytes + 4 * p, "f32_same_elems": 4 * n * p + 4 * p,
            **{f"q1_grid{gr}": q1_bytes for gr in grids}}
    out = {"clients": n, "cols": p, "variants": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in variants:
        ms = med[name]
        out["variants"][name] = {
            "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "kernel": launched[name][0], "grid": launched[name][1], "algorithmic_bytes": algo[name],
            "GiBps": round(algo[name] / (ms * 1e-3) / GIB, 1), "frac_of_8TBps": round(algo[name] / (ms * 1e-3) / PEAK, 4),
            "ns_per_row_chunk": round(ms * 1e6 / (n * -(-p // 2048)), 3)}
    out["q1_vs_q4_same_elems"] = round(med["q1"] / med["q4_same_elems"], 4)
    out["q1_vs_f32_same_elems"] = round(med["q1"] / med["f32_same_elems"], 4)
    out["q1_center_vs_q1"] = round(med["q1_center"] / med["q1"], 4)
    out["q1_chain25_vs_q1"] = round(med["q1_chain25"] / med["q1"], 4)
    out["expectation_q1_below_q4_same_elems"] = bool(med["q1"] < med["q4_same_elems"])
    return out


def bench_host(n, reps):
    from flearn_amd import AVG, QuantizedAVG, quant

    plain = resnet18_uploads(n)
    ups = {"avg": plain, "avg_q4": [quant.quantize_state_dict(m, bits=4) for m in plain],
           "avg_q1": [quant.quantize_state_dict(m, bits=1) for m in plain]}
    ups = {k: [{"agg_weight": 1.0, "params": m} for m in v] for k, v in ups.items()}
    strat = {"avg": AVG(output="float32"), "avg_q4": QuantizedAVG(output="float32", bits=4),
             "avg_q1": QuantizedAVG(output="float32", bits=1)}
    times = {k: [] for k in strat}
    for rep in range(reps + 1):
        for name in list(strat) if rep % 2 == 0 else list(strat)[::-1]:
            torch.cuda.synchronize()
            t = time.perf_counter()
            strat[name].server(ups[name], rep)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t) * 1e3)
    f32_bytes = 4 * n * strat["avg"].engine.last_plan.groups["f32"].stride
    med = {k: statistics.median(v) for k, v in times.items()}
    h2d = {"avg": f32_bytes, "avg_q4": strat["avg_q4"].engine.last_quant["bytes_in"],
           "avg_q1": strat["avg_q1"].engine.last_quant["bytes_in"]}
    return {"clients": n, "model": "resnet18", "reps": reps, "output": "float32",
            **{f"{k}_ms": round(v, 2) for k, v in med.items()},
            **{f"{k}_ms_min_max": [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
            "avg_q1_vs_avg": round(med["avg_q1"] / med["avg"], 4), "avg_q1_vs_avg_q4": round(med["avg_q1"] / med["avg_q4"], 4),
            "h2d_bytes": h2d, "h2d_ms_at_55GBps": {k: round(v / 55e9 * 1e3, 2) for k, v in h2d.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100x25610176")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-clients", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--parts", default="device,host")
    ap.add_argument("--grids", default="", help="device: also time q1 under these forced grids (fa_set_reduce_grid), e.g. 256,512")
    ap.add_argument("--lib", default="", help="another build of libflearn_amd.so to load (the depth sweep)")
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_quant1.py needs the GPU: a timing from anywhere else says nothing")
    if a.lib:
        na.LIB_PATH = Path(a.lib).resolve()
    from flearn_amd import ops

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    parts = a.parts.split(",")
    res = {"tool": "tools/bench_quant1.py", "lib": a.lib or "in-tree", "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(dev)}
    if "device" in parts:
        n, p = (int(v) for v in a.shape.lower().split("x"))
        res["device_sum"] = bench_device(ops, n, p, a.reps, a.warmup, dev, [int(v) for v in a.grids.split(",") if v])
        torch.cuda.empty_cache()
    if "host" in parts:
        res["host_round"] = bench_host(a.host_clients, a.host_reps)
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
