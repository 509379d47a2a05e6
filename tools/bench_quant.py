"""Int8 block-quantized uploads (fa_deq_fold_q8) against the fp32 fold (fa_fold) on the device, the
QuantizedAVG round against the AVG round from host memory, and the wire decode of quantized against
fp32 uploads (measurement tool, not a gate).

    python tools/bench_quant.py [--shape 100x25610152] [--reps 20] [--warmup 3] [--host-clients 100]
                                [--host-reps 5] [--wire-clients 20] [--parts device,host,wire] [--grids 256,512]
                                [--out profiles/quant/bench_quant.json]

One process.  device: codes, scales and fp32 values generated on the device; the variants are timed in
turn within every repetition (alternating, so drift hits all alike), each between two device events,
3 warm-up rounds, median of 20:

    q8                fa_deq_fold_q8 over the whole int8 stack, opening the sum
    q8_center         the same with a centre (delta uploads)
    q8_chain25        the same rows in chunks of 25 through acc_in
    q8_grid<G>        (--grids) q8 under fa_set_reduce_grid(G): what another grid rule would give
    f32_same_elems    (a) fa_fold (FA_ACC_F32) over an fp32 stack of the same element count: 4x the bytes
    f32_same_bytes    (b) fa_fold over a window of that stack of the same BYTE count: a quarter of the columns

The required condition: q8 takes less time than (a) in the same run.  Reported
per variant: ms (median, min, max), the instantiation and grid fa_last_launch named, GiB/s and the
fraction of 8 TB/s on the algorithmic bytes (q8: N*P + 4*N*P/1024 + 4*P), and q8's ratio to (b).
Before anything is timed the first 4,096 columns are checked against tests/quant_ref.py.

host: N ResNet-18 state dicts (flearn_amd.layouts) as numpy uploads; QuantizedAVG().server against
AVG().server in the same process, alternating, wall time with the device drained, median; the H2D
bytes of each and the host time of the code pack (quantround._pack_chunk) separately.
wire: Encrypt().decode of quantized against fp32 ResNet-18 uploads, per upload, reported only.
"""
from __future__ import annotations

import argparse
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

import quant_ref as qr  # noqa: E402
from flearn_amd import _native as na  # noqa: E402
from flearn_amd import layouts, ops, quant, quantround  # noqa: E402

PEAK = 8e12  # bytes/s, MI355X HBM3E
GIB = float(1 << 30)
DEFAULT_OUT = REPO / "profiles" / "quant" / "bench_quant.json"


def check_against_ref(q, s, w, g, acc):
    cols = min(4096, q.shape[1])
    n = min(q.shape[0], 12)
    hq, hs, hw, hg = q[:n, :cols].cpu().numpy(), s[:n].cpu().numpy(), w[:n].cpu().numpy(), g[:cols].cpu().numpy()
    for name, c, hc in (("q8", None, None), ("q8_center", g, hg)):
        ops.deq_fold_stack(q, s, w, None, acc, center=c, n_cols=cols, n_clients=n)
        if not qr.same_bits(acc[:cols].cpu().numpy(), qr.deq_fold(None, hq, hs, hw, hc)):
            sys.exit(f"fa_deq_fold_q8 differs from quant_ref ({name})")


def bench_device(n, p, reps, warmup, dev, grids=()):
    pitch = -(-p // 1024) * 1024
    nb = pitch // 1024
    q = torch.randint(-128, 128, (n, pitch), dtype=torch.int8, device=dev)
    s = torch.rand((n, nb), dtype=torch.float32, device=dev) * 0.01
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    g = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(g, seed=7)
    g = g.reshape(-1)
    w = torch.rand(n, dtype=torch.float32, device=dev) + 0.5
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    quarter = (p // 4) // 64 * 64
    launched = {}

    def note(name):
        if name not in launched:
            launched[name] = ops.last_launch()[:2]

    def q8(center):
        def run():
            ops.deq_fold_stack(q, s, w, None, acc, center=center, n_cols=p)
            note("q8" if center is None else "q8_center")
        return run

    def q8_chain():
        for lo in range(0, n, 25):
            hi = min(n, lo + 25)
            ops.deq_fold_stack(q[lo:hi], s[lo:hi], w[lo:hi], acc if lo else None, acc, n_cols=p)
        note("q8_chain25")

    def f32(cols, name):
        def run():
            ops.fold_stack(na.ACC_F32, x, w, None, acc, n_cols=cols)
            note(name)
        return run

    def q8_forced(grid):
        def run():
            prev = ops.set_reduce_grid(grid)
            try:
                ops.deq_fold_stack(q, s, w, None, acc, n_cols=p)
            finally:
                ops.set_reduce_grid(prev)
            note(f"q8_grid{grid}")
        return run

    variants = {"q8": q8(None), "q8_center": q8(g), "q8_chain25": q8_chain,
                "f32_same_elems": f32(p, "f32_same_elems"), "f32_same_bytes": f32(quarter, "f32_same_bytes"),
                **{f"q8_grid{gr}": q8_forced(gr) for gr in grids}}
    check_against_ref(q, s, w, g, acc)
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
    q8_bytes = n * p + 4 * n * (-(-p // 1024)) + 4 * p
    algo = {"q8": q8_bytes, "q8_center": q8_bytes + 4 * p, "q8_chain25": q8_bytes + (-(-n // 25) - 1) * 8 * p,
            "f32_same_elems": 4 * n * p + 4 * p, "f32_same_bytes": 4 * n * quarter + 4 * quarter,
            **{f"q8_grid{gr}": q8_bytes for gr in grids}}
    out = {"clients": n, "cols": p, "same_bytes_cols": quarter, "variants": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in variants:
        ms = med[name]
        out["variants"][name] = {
            "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "kernel": launched[name][0], "grid": launched[name][1], "algorithmic_bytes": algo[name],
            "GiBps": round(algo[name] / (ms * 1e-3) / GIB, 1), "frac_of_8TBps": round(algo[name] / (ms * 1e-3) / PEAK, 4),
            "byte_floor_ms": round(algo[name] / PEAK * 1e3, 4)}
    out["q8_vs_f32_same_elems"] = round(med["q8"] / med["f32_same_elems"], 4)
    out["q8_vs_f32_same_bytes"] = round(med["q8"] / med["f32_same_bytes"], 4)
    out["q8_center_vs_q8"] = round(med["q8_center"] / med["q8"], 4)
    out["q8_chain25_vs_q8"] = round(med["q8_chain25"] / med["q8"], 4)
    out["required_q8_faster_than_f32_same_elems"] = bool(med["q8"] < med["f32_same_elems"])
    del q, s, x, g, acc
    torch.cuda.empty_cache()
    return out


def resnet18_uploads(n):
    layout = layouts.get("resnet18")
    elems = layouts.fp32_elems(layout)
    base = np.random.default_rng(1).standard_normal(elems).astype(np.float32)
    return [layouts.synthetic_state_dict(layout, base * np.float32(1.0 + 1e-3 * i), counter=i) for i in range(n)]


def bench_host(n, reps):
    from flearn_amd import AVG, QuantizedAVG

    plain = resnet18_uploads(n)
    t0 = time.perf_counter()
    quantized = [quant.quantize_state_dict(m) for m in plain]
    quantize_ms = (time.perf_counter() - t0) * 1e3 / n
    ups = {"avg": [{"agg_weight": 1.0, "params": m} for m in plain],
           "avg_q8": [{"agg_weight": 1.0, "params": m} for m in quantized]}
    strat = {"avg": AVG(output="float32"), "avg_q8": QuantizedAVG(output="float32")}
    pack_ms = []
    inner = quantround._pack_chunk

    def timed_pack(*a):
        t = time.perf_counter()
        r = inner(*a)
        pack_ms.append((time.perf_counter() - t) * 1e3)
        return r

    quantround._pack_chunk = timed_pack
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
        quantround._pack_chunk = inner
    lq = strat["avg_q8"].engine.last_quant
    f32_bytes = 4 * n * strat["avg"].engine.last_plan.groups["f32"].stride
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"clients": n, "model": "resnet18", "reps": reps, "output": "float32",
            "avg_ms": round(med["avg"], 2), "avg_q8_ms": round(med["avg_q8"], 2),
            "avg_q8_vs_avg": round(med["avg_q8"] / med["avg"], 4),
            "h2d_bytes_avg": f32_bytes, "h2d_bytes_avg_q8": lq["bytes_in"],
            "h2d_ms_at_55GBps": {"avg": round(f32_bytes / 55e9 * 1e3, 2), "avg_q8": round(lq["bytes_in"] / 55e9 * 1e3, 2)},
            "q8_pack_ms": round(statistics.median(pack_ms[1:] or pack_ms), 2),
            "client_quantize_ms_per_upload": round(quantize_ms, 2)}


def bench_wire(n):
    from flearn_amd import Encrypt

    enc = Encrypt()
    plain = resnet18_uploads(n)
    out = {"clients": n, "model": "resnet18"}
    for name, params in (("fp32", plain), ("q8", [quant.quantize_state_dict(m) for m in plain])):
        blobs = [enc.encode({"agg_weight": 1.0, "params": p}) for p in params]
        t = time.perf_counter()
        for b in blobs:
            enc.decode(b)
        out[f"{name}_decode_ms_per_upload"] = round((time.perf_counter() - t) * 1e3 / n, 2)
        out[f"{name}_encoded_bytes_per_upload"] = len(blobs[0])
        del blobs
    out["q8_vs_fp32"] = round(out["q8_decode_ms_per_upload"] / out["fp32_decode_ms_per_upload"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100x25610152")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-clients", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--wire-clients", type=int, default=20)
    ap.add_argument("--parts", default="device,host,wire")
    ap.add_argument("--grids", default="", help="device: also time q8 under these forced grids (fa_set_reduce_grid), e.g. 256,512")
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_quant.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    parts = a.parts.split(",")
    res = {"tool": "tools/bench_quant.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev)}
    if "device" in parts:
        n, p = (int(v) for v in a.shape.lower().split("x"))
        res["device_sum"] = bench_device(n, p, a.reps, a.warmup, dev, [int(v) for v in a.grids.split(",") if v])
    if "host" in parts:
        res["host_round"] = bench_host(a.host_clients, a.host_reps)
    if "wire" in parts:
        res["wire"] = bench_wire(a.wire_clients)
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
