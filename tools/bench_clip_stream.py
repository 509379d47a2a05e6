"""The streamed clipped round (fa_clip_fold_f32, StreamedNormClip) against its one-launch and
unclipped counterparts (measurement tool, not a gate).

    python tools/bench_clip_stream.py [--shape 100x25610152] [--chunks 100,50,25,16] [--reps 20] [--warmup 3]
                                      [--rounds lenet5x1000,resnet18x300] [--round-chunks 16,64] [--round-reps 3]
                                      [--out profiles/clipstream/bench_clip_stream.json]

Kernel part: one process, values generated on the device (fa_fill_uniform_f32).  The variants are
timed in turn within every repetition (alternating, so drift hits all alike), each between two
device events, 3 warm-up rounds, median of 20, at 0 / 10 / 100 % of the rows clipped (scale 0.5):

    clip_sum          one fa_clip_sum_f32 launch over the whole stack: the yardstick (existing kernel)
    clip_sum_again    the same launch once more per repetition: the spread of the yardstick itself
    fold_K            fa_clip_fold_f32 in chunks of K rows chained through the accumulator
                      (K = N: one opening launch)

Beside each time stands the byte floor at 8 TB/s from the shapes: N*P*4 client bytes, per chunk P*4
of centre and P*4 of stored sums, and P*4 of accumulator read by every chunk but the first.  Before
anything is timed the first 4,096 columns of every chain are checked against tests/clip_ref.py.

Round part: uploads in host memory (numpy, drawn from 10 distinct state_dicts so the host holds 10
models), StreamedNormClip.server() against AVG(chunk_clients=K).server() on the same uploads, one
warm-up round, median of --round-reps; for the first configuration also the same round with the
one-chunk lag of the clip fold switched off (ClippedRoundAccumulator(lag=False)).  device_bytes is
what the round holds on the device, beside what one [N, stride] stack would need.
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

import clip_ref as cr  # noqa: E402
from flearn_amd import AVG, StreamedNormClip, layouts  # noqa: E402
from flearn_amd import _native as na  # noqa: E402
from flearn_amd import clipstream, ops  # noqa: E402

NS = 25610152
PEAK = 8e12  # bytes/s, MI355X HBM3E
DEFAULT_OUT = REPO / "profiles" / "clipstream" / "bench_clip_stream.json"


def chain(x, g, s, acc, n, k, p):
    """Rows [0, n) in chunks of k through fa_clip_fold_f32; returns the number of launches."""
    acc_in, c = None, 0
    for a in range(0, n, k):
        b = min(a + k, n)
        ops.clip_fold_stack(x[a:b], g, s[a:b], acc_in, acc, n_cols=p)
        acc_in, c = acc, c + 1
    return c


def byte_floor_ms(n, p, chunks):
    return (n * p * 4 + chunks * 2 * p * 4 + (chunks - 1) * p * 4) / PEAK * 1e3


def bench_kernel(n, p, ks, reps, warmup, dev):
    pitch = -(-p // 64) * 64
    x = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(x, seed=2024)
    g = torch.empty((1, pitch), dtype=torch.float32, device=dev)
    ops.fill_uniform(g, seed=7)
    g = g.reshape(-1)
    acc = torch.empty(pitch, dtype=torch.float32, device=dev)
    tenth = np.arange(n) % 10 == 0
    patterns = {"0pct": np.ones(n, np.float32), "10pct": np.where(tenth, 0.5, 1.0).astype(np.float32),
                "100pct": np.full(n, 0.5, np.float32)}
    scales = {k: torch.from_numpy(v).to(dev) for k, v in patterns.items()}
    cols = min(4096, p)
    hx, hg = x[:, :cols].cpu().numpy(), g[:cols].cpu().numpy()
    for name, s in scales.items():  # every chain against clip_ref before anything is timed
        want = cr.clipped_sum(hx, hg, patterns[name]).tobytes()
        for k in ks:
            chain(x, g, s, acc, n, k, cols)
            if acc[:cols].cpu().numpy().tobytes() != want:
                sys.exit(f"fa_clip_fold_f32 in chunks of {k} differs from clip_ref at N = {n}, {name}")
    launched = {}
    variants = {}
    for name, s in scales.items():
        def clip_sum(s=s, name=name):
            ops.clip_sum_stack(x, g, s, acc, n_cols=p)
            launched.setdefault(f"clip_sum/{name}", ops.last_launch()[:2])
        variants[f"clip_sum/{name}"] = (clip_sum, 1)
        variants[f"clip_sum_again/{name}"] = (clip_sum, 1)
        for k in ks:
            def fold(s=s, k=k, key=f"fold_{k}/{name}"):
                chain(x, g, s, acc, n, k, p)
                launched.setdefault(key, ops.last_launch()[:2])
            variants[f"fold_{k}/{name}"] = (fold, -(-n // k))
    times = {k: [] for k in variants}
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
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1))
    out = {"clients": n, "cols": p, "variants": {}}
    for name, (_, chunks) in variants.items():
        ms = statistics.median(times[name])
        base = statistics.median(times["clip_sum/" + name.split("/")[1]])
        floor = byte_floor_ms(n, p, chunks)
        out["variants"][name] = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                                 "chunks": chunks, "kernel": launched[name.replace("_again", "")][0],
                                 "grid": launched[name.replace("_again", "")][1], "byte_floor_ms": round(floor, 4),
                                 "frac_of_8TBps": round(floor / ms, 4), "time_vs_clip_sum": round(ms / base, 4)}
    del x, acc, g
    torch.cuda.empty_cache()
    return out


def host_uploads(layout, n, distinct=10):
    rng = np.random.default_rng(5)
    elems = layouts.fp32_elems(layout)
    g = layouts.synthetic_state_dict(layout, rng.standard_normal(elems).astype(np.float32))
    base = [layouts.synthetic_state_dict(layout, (rng.standard_normal(elems) * 0.02 * (1 + i)).astype(np.float32), i)
            for i in range(distinct)]
    for b in base:
        for k in b:
            if b[k].dtype == np.float32:
                b[k] += g[k]
    return g, [{"agg_weight": 1, "params": base[i % distinct]} for i in range(n)]


def timed(fn, reps):
    fn()  # warm-up: buffers, pinned staging, plans
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ts), 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2)}


def bench_rounds(spec, ks, reps, lag_too):
    name, n = spec.lower().split("x")
    n = int(n)
    layout = layouts.get(name)
    g, ups = host_uploads(layout, n)
    f32 = [k for k in g if g[k].dtype == np.float32]
    d2 = sum(float(((ups[5]["params"][k].astype(np.float64) - g[k]) ** 2).sum()) for k in f32)
    tau = float(np.sqrt(d2))  # distinct upload 5 of 10 sits on the radius: four rows in ten are clipped
    out = {"model": name, "clients": n, "distinct_uploads": 10, "tau": tau, "chunks": {}}
    for k in ks:
        s = StreamedNormClip(tau, output="float32", chunk_clients=k)
        s.init_global(g)
        rec = {"clipped_ms": timed(lambda: (s.init_global(g), s.server(ups, 0)), reps)}
        rec["clipped_rows"] = int(s.engine.last_clip["clipped"].size)
        acc = s.engine.begin_clipped_round(tau, g, chunk_clients=k)
        rec["device_bytes"] = acc.device_bytes
        rec["one_stack_bytes"] = n * s.engine.last_plan.groups["f32"].stride * 4
        if lag_too and k == ks[0]:
            def no_lag(agg=s.engine):
                acc = clipstream.ClippedRoundAccumulator(agg, tau, g, None, None, k, lag=False)
                for u in ups:
                    acc.add(u)
                return acc.finish()
            rec["clipped_no_lag_ms"] = timed(no_lag, reps)
            rec["lag_vs_no_lag"] = round(rec["clipped_ms"]["ms"] / rec["clipped_no_lag_ms"]["ms"], 4)
        a = AVG(output="float32", chunk_clients=k)
        rec["avg_ms"] = timed(lambda: a.server(ups, 0), reps)
        rec["clipped_vs_avg"] = round(rec["clipped_ms"]["ms"] / rec["avg_ms"]["ms"], 4)
        out["chunks"][str(k)] = rec
        del s, a
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default=f"100x{NS}")
    ap.add_argument("--chunks", default="100,50,25,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", default="lenet5x1000,resnet18x300", help="model x clients, comma separated; '' for none")
    ap.add_argument("--round-chunks", default="16,64")
    ap.add_argument("--round-reps", type=int, default=3)
    ap.add_argument("--out", default=str(DEFAULT_OUT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip_stream.py needs the GPU: a timing from anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    na.lib()
    res = {"tool": "tools/bench_clip_stream.py", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "kernel": None, "rounds": []}
    if a.shape:
        n, p = (int(v) for v in a.shape.lower().split("x"))
        res["kernel"] = bench_kernel(n, p, [int(k) for k in a.chunks.split(",")], a.reps, a.warmup, dev)
    for i, spec in enumerate(s for s in a.rounds.split(",") if s):
        res["rounds"].append(bench_rounds(spec, [int(k) for k in a.round_chunks.split(",")], a.round_reps, i == 0))
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
