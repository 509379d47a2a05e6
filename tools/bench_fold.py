"""The fold chain (fa_fold per chunk + fa_fold_finish) against fa_reduce_f32 (measurement tool).

    python tools/bench_fold.py [--clients 100] [--cols 25610152] [--reps 20] [--warmup 3] [--out FILE]

One process, values generated on the device (fa_fill_uniform_f32), plain mean, FA_MODE_W32_DIV64
with the float64 result.  Variants, timed in turn within every repetition (alternating, so drift
hits all alike), each between two device events, 3 warm-up rounds, median of 20:

    reduce_one_launch        fa_reduce_f32 over the whole stack: the line to compare against
    fold_k<K>_inplace        ceil(N / K) fa_fold launches of K clients, the accumulator in place,
    fold_k<K>_double         ... or double-buffered (read one, write the other), then fa_fold_finish

for K in {10, 25, 50, 100}.  Prints (and with --out writes) one JSON line: per variant ms (median,
min, max), GB/s on its own algorithmic bytes — N*P*4 + 2*P*s_acc*ceil(N/K) + P*s_acc + outputs (the
first fold reads no accumulator, which the formula counts as if it did, as the issue states it) —
the fraction of 8 TB/s and the ratio of its time to the single launch's.
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
from flearn_amd.streaming import fold_finish, fold_stack  # noqa: E402

NS = 25610152
PEAK = 8e12  # bytes/s, MI355X HBM3E
CHUNKS = (10, 25, 50, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=100)
    ap.add_argument("--cols", type=int, default=NS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fold.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    n, p = a.clients, a.cols
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    agg.fill_uniform(x, seed=2024)
    w = torch.full((n,), 0.3, dtype=torch.float32, device=dev)
    denom = float(n) * 0.3
    o64 = torch.empty(p, dtype=torch.float64, device=dev)
    acc = [torch.empty(pitch, dtype=torch.float32, device=dev) for _ in range(2)]

    def chain(k, double):
        def run():
            cur, j = None, 0
            for i0 in range(0, n, k):
                out = acc[j % 2] if double else acc[0]
                fold_stack(na.ACC_F32, x[i0 : i0 + k], w[i0 : i0 + k], cur, out, n_cols=p)
                cur, j = out, j + 1
            fold_finish(na.ACC_F32, na.MODE_W32_DIV64, cur, denom, p, out64=o64)
        return run

    s_acc, outputs = 4, p * 8
    variants = {"reduce_one_launch": (lambda: agg.reduce_stack(x, w, na.MODE_W32_DIV64, denom, n_cols=p, out64=o64),
                                      n * p * 4 + outputs, 1)}
    for k in CHUNKS:
        if k > n:
            continue
        launches = -(-n // k)
        nbytes = n * p * 4 + 2 * p * s_acc * launches + p * s_acc + outputs
        variants[f"fold_k{k}_inplace"] = (chain(k, False), nbytes, launches + 1)
        variants[f"fold_k{k}_double"] = (chain(k, True), nbytes, launches + 1)

    # the results agree bit for bit before anything is timed
    variants["reduce_one_launch"][0]()
    want = o64.clone()
    for name, (fn, _, _) in variants.items():
        o64.zero_()
        fn()
        if not torch.equal(o64.view(torch.int64), want.view(torch.int64)):
            sys.exit(f"{name}: result differs from the single launch")

    times = {k: [] for k in variants}
    events = []
    for rep in range(a.warmup + a.reps):
        for name, (fn, _, _) in variants.items():
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
           "mode": "W32_DIV64 mean, out64", "variants": {}}
    base = statistics.median(times["reduce_one_launch"])
    for name, (_, nbytes, launches) in variants.items():
        ms = statistics.median(times[name])
        res["variants"][name] = {
            "ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "launches": launches, "bytes": nbytes, "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1),
            "frac_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 4), "time_vs_one_launch": round(ms / base, 4),
            "bytes_vs_one_launch": round(nbytes / (n * p * 4 + outputs), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
