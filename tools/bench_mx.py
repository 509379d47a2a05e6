"""Measure the Microscaling dequantize-and-sum (fa_deq_fold_mx) on the GPU.

device: N x P columns of random MXFP4 and MXFP8 codes with scale bytes 117 ... 137, summed by
ops.deq_fold_mx_stack; beside them the int4 sum (fa_deq_fold_q4) of the same elements, FP4's yardstick, the int8
sum (fa_deq_fold_q8), FP8's, and the fp32 fold, plus a centred run, a chain of 25-row chunks and forced grids
(--grids) for both element types.  All variants alternate in both orders in one process; device time from
events, median with min and max.  --lib loads another build of the library (the unit rebuilt with
-DFA_MX_DEPTH4= / -DFA_MX_DEPTH8=: the pipeline depth is a compile-time constant).  Reported per variant: ms, the
kernel and grid launched, and the fraction of 8 TB/s on the algorithmic bytes (codes + one scale byte per 32 +
the fp32 result).  Before anything is timed the first 4,096 columns are checked against tests/mx_ref.py.

host: N ResNet-18 state dicts (flearn_amd.layouts) as numpy uploads; AVG, QuantizedAVG(bits=4), (bits=8) and
their format="mx" counterparts .server in the same process, in both orders, wall time with the device drained,
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

import mx_ref as mxr  # noqa: E402
from bench_quant import resnet18_uploads  # noqa: E402
from flearn_amd import _native as na  # noqa: E402

PEAK = 8e12  # bytes/s, MI355X HBM3E
GIB = float(1 << 30)
DEFAULT_OUT = REPO / "profiles" / "mx" / "bench_mx.json"


def check_against_ref(ops, q, s, w, g, acc, elem):
    cols, n = 4096, min(q.shape[0], 12)
    hq, hs, hw, hg = q[:n, : cols * elem // 8].cpu().numpy(), s[:n].cpu().numpy(), w[:n].cpu().numpy(), g[:cols].cpu().numpy()
    for c, hc in ((None, None), (g, hg)):
        ops.deq_fold_mx_stack(q, s, w, None, acc, center=c, n_cols=cols, n_clients=n, elem=elem)
        if not mxr.same_bits(acc[:cols].cpu().numpy(), mxr.deq_fold(None, hq, hs, hw, cols, elem, hc)):
            sys.exit(f"fa_deq_fold_mx differs from mx_ref (elem {elem}, centre {c is not None})")


def bench_device(ops, n, p, reps, warmup, dev, grids=()):
    pitch = -(-p // 2048) * 2048
    codes = {4: torch.randint(0, 256, (n, pitch // 2), dtype=torch.uint8, device=dev),
             8: torch.randint(0, 127, (n, pitch), dtype=torch.uint8, device=dev)}  # the int4 and int8 sums read the same bytes
    e8 = torch.randint(117, 138, (n, pitch // 32), dtype=torch.uint8, device=dev)
    s4 = torch.rand((n, pitch // 128), dtype=torch.float32, device=dev) * 0.01 + 1e-6
    s8 = torch.rand((n, pitch // 1024), dtype=torch.float32, device=dev) * 0.01 + 1e-6
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    g = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(g, seed=7)
    g = g.reshape(-1)
    w = torch.rand(n, dtype=torch.float32, device=dev) + 0.5
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    launched = {}

    def mx(elem, **kw):
        return lambda: ops.deq_fold_mx_stack(codes[elem], e8, w, None, acc, n_cols=p, elem=elem, **kw)

    def chain(elem):
        for lo in range(0, n, 25):
            hi = min(n, lo + 25)
            ops.deq_fold_mx_stack(codes[elem][lo:hi], e8[lo:hi], w[lo:hi], acc if lo else None, acc, n_cols=p, elem=elem)

    def forced(elem, grid):
        prev = ops.set_reduce_grid(grid)
        try:
            mx(elem)()
        finally:
            ops.set_reduce_grid(prev)

    variants = {"q4_same_elems": lambda: ops.deq_fold_q4_stack(codes[4], s4, w, None, acc, n_cols=p),
                "q8_same_elems": lambda: ops.deq_fold_stack(codes[8].view(torch.int8), s8, w, None, acc, n_cols=p),
                "f32_same_elems": lambda: ops.fold_stack(na.ACC_F32, x, w, None, acc, n_cols=p)}
    for elem in (4, 8):
        variants.update({f"mx{elem}": mx(elem), f"mx{elem}_center": mx(elem, center=g), f"mx{elem}_chain25": (lambda elem=elem: chain(elem)),
                         **{f"mx{elem}_grid{gr}": (lambda elem=elem, gr=gr: forced(elem, gr)) for gr in grids}})
        check_against_ref(ops, codes[elem], e8, w, g, acc, elem)
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

    def algo(name):
        if name.startswith("mx"):
            elem = int(name[2])
            b = n * p * elem // 8 + n * (-(-p // 32)) + 4 * p
            return b + 4 * p * name.endswith("center") + (-(-n // 25) - 1) * 8 * p * name.endswith("chain25")
        return {"q4": n * (p // 2) + 4 * n * (-(-p // 128)), "q8": n * p + 4 * n * (-(-p // 1024)), "f3": 4 * n * p}[name[:2]] + 4 * p

    out = {"clients": n, "cols": p, "variants": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in variants:
        ms = med[name]
        out["variants"][name] = {
            "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "kernel": launched[name][0], "grid": launched[name][1], "algorithmic_bytes": algo(name),
            "GiBps": round(algo(name) / (ms * 1e-3) / GIB, 1), "frac_of_8TBps": round(algo(name) / (ms * 1e-3) / PEAK, 4)}
    out["mx4_vs_q4_same_elems"] = round(med["mx4"] / med["q4_same_elems"], 4)
    out["mx8_vs_q8_same_elems"] = round(med["mx8"] / med["q8_same_elems"], 4)
    out["mx4_vs_f32_same_elems"] = round(med["mx4"] / med["f32_same_elems"], 4)
    out["mx8_vs_f32_same_elems"] = round(med["mx8"] / med["f32_same_elems"], 4)
    return out


def bench_host(n, reps):
    from flearn_amd import AVG, QuantizedAVG, quant

    plain = resnet18_uploads(n)
    kinds = {"avg_q4": (4, "int"), "avg_q8": (8, "int"), "avg_mx4": (4, "mx"), "avg_mx8": (8, "mx")}
    ups = {"avg": plain, **{k: [quant.quantize_state_dict(m, bits=b, format=f) for m in plain] for k, (b, f) in kinds.items()}}
    ups = {k: [{"agg_weight": 1.0, "params": m} for m in v] for k, v in ups.items()}
    strat = {"avg": AVG(output="float32"), **{k: QuantizedAVG(output="float32", bits=b, format=f) for k, (b, f) in kinds.items()}}
    times = {k: [] for k in strat}
    for rep in range(reps + 1):
        for name in list(strat) if rep % 2 == 0 else list(strat)[::-1]:
            torch.cuda.synchronize()
            t = time.perf_counter()
            strat[name].server(ups[name], rep)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    h2d = {"avg": 4 * n * strat["avg"].engine.last_plan.groups["f32"].stride,
           **{k: strat[k].engine.last_quant["bytes_in"] for k in kinds}}
    return {"clients": n, "model": "resnet18", "reps": reps, "output": "float32",
            **{f"{k}_ms": round(v, 2) for k, v in med.items()},
            **{f"{k}_ms_min_max": [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}, "h2d_bytes": h2d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100x25610176")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-clients", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--parts", default="device,host")
    ap.add_argument("--grids", default="", help="device: also time both element types under these forced grids (fa_set_reduce_grid), e.g. 256,512")
    ap.add_argument("--lib", default="", help="another build of libflearn_amd.so to load (the depth sweep)")
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mx.py needs the GPU: a timing from anywhere else says nothing")
    if a.lib:
        na.LIB_PATH = Path(a.lib).resolve()
    from flearn_amd import ops

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    parts = a.parts.split(",")
    res = {"tool": "tools/bench_mx.py", "lib": a.lib or "in-tree", "reps": a.reps, "warmup": a.warmup,
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
