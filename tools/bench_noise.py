"""The Gaussian noise of a DP-FedAvg round (fa_gauss_add_f32) beside the clipped round it is added to
(fa_rownorm2_f32, fa_clip_sum_f32 + fa_fold_finish) and the weighted mean (fa_reduce_f32), on the SAME
client stack (measurement tool, not a gate).

    python tools/bench_noise.py [--shapes 10x25610152,100x25610152] [--reps 20] [--warmup 3]
                                [--out profiles/noise/bench_noise.json]

One process, values generated on the device (fa_fill_uniform_f32), FA_MODE_W32_DIV64 with the
float64 result.  Per shape the variants are timed in turn within every repetition (alternating, so
drift hits all alike), each between two device events, 3 warm-up rounds, median of 20:

    mean         fa_reduce_f32 over the whole stack: the line to compare against
    rownorm      fa_rownorm2_f32 (both kernels): the clipped round's first pass
    clip         fa_clip_sum_f32 with every tenth row at scale 0.5, then fa_fold_finish
    gauss_add    fa_gauss_add_f32 alone, over the accumulator
    clip_noise   fa_clip_sum_f32, fa_gauss_add_f32, fa_fold_finish: the noised round's second pass

Prints and writes one JSON document: per shape and variant ms (median, min, max) and the kernel and
grid fa_last_launch named; for gauss_add its byte floor (8 B per column at 8 TB/s), its instruction
floor (per quad 20 64-bit integer multiplies at quarter rate, 8 transcendentals at quarter rate and
about 60 plain vector instructions, on 256 CUs x 4 SIMDs at 2.4 GHz) and the ratio to the larger; and
the noised round (rownorm + clip_noise) against the clipped round (rownorm + clip).  "z_error" is
the largest |z - z_ref| over the 2^20-column sample of tests/noise_ref.py, whose Z_ERROR constant is
twice that, rounded up.  Before anything is timed the first 4,096 columns are checked against
tests/noise_ref.py and tests/clip_ref.py.
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
sys.path.insert(0, str(REPO / "tests"))

import clip_ref as cr  # noqa: E402
import noise_ref as nr  # noqa: E402
from flearn_amd import _native as na  # noqa: E402
from flearn_amd import ops  # noqa: E402

NS = 25610152
PEAK = 8e12  # bytes/s, MI355X HBM3E
SIMD_HZ = 256 * 4 * 2.4e9  # wave instructions issued per second at one per cycle and SIMD
QUAD_CYCLES = 20 * 16 + 8 * 8 + 60 * 4  # issue cycles of one wave's quad: see the docstring
DEFAULT_OUT = REPO / "profiles" / "noise" / "bench_noise.json"
SEED, SEQ = nr.SAMPLE["seed"], nr.SAMPLE["sequence"]
SIGMA = 0.37


def z_error(dev):
    n = nr.SAMPLE["n"]
    acc = torch.zeros(n, dtype=torch.float32, device=dev)
    ops.gauss_add(acc, 1.0, SEED, SEQ)
    z = acc.cpu().numpy().astype(np.float64)
    err = np.abs(z - nr.normals(SEED, SEQ, 0, n))
    if not err.max() <= nr.Z_ERROR:
        sys.exit(f"fa_gauss_add_f32 is {err.max():.3g} from noise_ref, past Z_ERROR = {nr.Z_ERROR:.3g}")
    return {"columns": n, "seed": hex(SEED), "sequence": SEQ, "measured_max": float(err.max()), "column": int(err.argmax()),
            "test_constant": nr.Z_ERROR, "mean": float(z.mean()), "var": float(z.var()), "max_abs_z": float(np.abs(z).max())}


def check_against_ref(x, g, scale, acc):
    cols = min(4096, x.shape[1])
    hx, hg = x[:, :cols].cpu().numpy(), g[:cols].cpu().numpy()
    ops.clip_sum_stack(x, g, scale, acc, n_cols=cols)
    total = acc[:cols].cpu().numpy()
    if total.tobytes() != cr.clipped_sum(hx, hg, scale.cpu().numpy()).tobytes():
        sys.exit("fa_clip_sum_f32 differs from clip_ref")
    zero = torch.zeros(cols, dtype=torch.float32, device=x.device)
    ops.gauss_add(zero, 1.0, SEED, SEQ)
    z = zero.cpu().numpy()
    if not np.abs(z.astype(np.float64) - nr.normals(SEED, SEQ, 0, cols)).max() <= nr.Z_ERROR:
        sys.exit("fa_gauss_add_f32 differs from noise_ref")
    ops.gauss_add(acc, SIGMA, SEED, SEQ, n_cols=cols)
    if acc[:cols].cpu().numpy().tobytes() != nr.add(total, SIGMA, z).tobytes():
        sys.exit("fa_gauss_add_f32's add is not fl32(acc + fl32(sigma * z))")


def bench_shape(n, p, reps, warmup, dev):
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    g = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(g, seed=7)
    g = g.reshape(-1)
    w = torch.ones(n, dtype=torch.float32, device=dev)
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    work = torch.empty(ops.rownorm_workspace(n, p), dtype=torch.uint8, device=dev)
    scale = torch.from_numpy(np.where(np.arange(n) % 10 == 0, 0.5, 1.0).astype(np.float32)).to(dev)
    launched = {}

    def note(name):
        if name not in launched:
            launched[name] = ops.last_launch()[:2]

    def mean():
        ops.reduce_stack(x, w, na.MODE_W32_DIV64, float(n), n_cols=p, out64=o64)
        note("mean")

    def rownorm():
        ops.rownorm2_stack(x, center=g, n_cols=p, out=d2, workspace=work)
        note("rownorm")

    def clip():
        ops.clip_sum_stack(x, g, scale, acc, n_cols=p)
        note("clip")
        ops.fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc, float(n), p, out64=o64)

    def gauss_add():
        ops.gauss_add(acc, SIGMA, SEED, SEQ, n_cols=p)
        note("gauss_add")

    def clip_noise():
        ops.clip_sum_stack(x, g, scale, acc, n_cols=p)
        ops.gauss_add(acc, SIGMA, SEED, SEQ, n_cols=p)
        note("clip_noise")
        ops.fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc, float(n), p, out64=o64)

    variants = {"mean": mean, "rownorm": rownorm, "clip": clip, "gauss_add": gauss_add, "clip_noise": clip_noise}
    check_against_ref(x, g, scale, acc)
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
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"clients": n, "cols": p, "variants": {}}
    for name in variants:
        out["variants"][name] = {"ms": round(med[name], 4), "ms_min": round(min(times[name]), 4),
                                 "ms_max": round(max(times[name]), 4), "kernel": launched[name][0], "grid": launched[name][1],
                                 "time_vs_mean": round(med[name] / med["mean"], 4)}
    byte_floor = p * 8 / PEAK * 1e3
    alu_floor = -(-p // 4) / 64 * QUAD_CYCLES / SIMD_HZ * 1e3
    ga = out["variants"]["gauss_add"]
    ga.update(byte_floor_ms=round(byte_floor, 4), instruction_floor_ms=round(alu_floor, 4),
              vs_larger_floor=round(med["gauss_add"] / max(byte_floor, alu_floor), 3),
              GBps=round(p * 8 / (med["gauss_add"] * 1e-3) / 1e9, 1))
    clipped, noised = med["rownorm"] + med["clip"], med["rownorm"] + med["clip_noise"]
    out["clipped_round_ms"] = round(clipped, 4)
    out["noised_round_ms"] = round(noised, 4)
    out["noised_vs_clipped_round"] = round(noised / clipped, 4)
    out["noise_cost_ms"] = round(med["clip_noise"] - med["clip"], 4)
    del x, o64, acc, g
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=f"10x{NS},100x{NS}")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_noise.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    res = {"tool": "tools/bench_noise.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "mode": "W32_DIV64, out64; clip = fa_clip_sum_f32 (every tenth row at scale 0.5) + fa_fold_finish, clip_noise = "
                   "fa_clip_sum_f32 + fa_gauss_add_f32 + fa_fold_finish, rownorm = fa_rownorm2_f32 (both kernels), mean = "
                   "fa_reduce_f32, same stack",
           "z_error": z_error(dev), "shapes": []}
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
