"""Device time of the sparse ordered sum (fa_sparse_fold_f32, both launches) against the fp32 fold of the
densified stack, in one process: device events, warm-ups, the median of 20, the variants alternating.

    python tools/bench_sparse.py [--clients 100] [--cols 25600000] [--ratios 0.001,0.01,0.1] [--lib PATH] [--out FILE]

--lib loads another build of the library (the unit rebuilt with -DFA_SPARSE_WC=... / -DFA_SPARSE_DEPTH=...:
the sweep of DESIGN.md section 23).  Prints one JSON line and, with --out, writes it there.  The floors:
bytes = the pair stack plus the 4 * P-byte store (and the 4 * P-byte centre read) at 8 TB/s."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from flearn_amd import _native as na  # noqa: E402

REPS, WARM = 20, 3


def pairs_of(n, cols, k, dev):
    """n rows of k strictly ascending columns, one per stride of cols / k, and N(0, 1) values."""
    step = cols / k
    base = torch.arange(k, device=dev, dtype=torch.float64) * step
    col = (base[None, :] + torch.rand(n, k, device=dev, dtype=torch.float64) * max(step - 1, 0)).floor().to(torch.int64)
    val = torch.randn(n, k, device=dev, dtype=torch.float32)
    ks = (k + 1) & ~1
    out = torch.zeros(n, ks, 2, dtype=torch.int32, device=dev)
    out[:, :, 0] = -1  # 0xFFFFFFFF
    out[:, :k, 0] = col.to(torch.int32)
    out[:, :k, 1] = val.view(torch.int32)
    return out


def timed(variants):
    ev = {name: [] for name in variants}
    for r in range(WARM + REPS):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= WARM:
                ev[name].append(a.elapsed_time(b))
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=100)
    ap.add_argument("--cols", type=int, default=25_600_000)
    ap.add_argument("--ratios", default="0.001,0.01,0.1")
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--no-dense", action="store_true")
    a = ap.parse_args()
    if a.lib:
        na.LIB_PATH = Path(a.lib).resolve()
    from flearn_amd import ops

    dev = torch.device("cuda")
    n, cols = a.clients, a.cols
    w = torch.rand(n, device=dev) + 0.5
    acc = torch.empty(cols, dtype=torch.float32, device=dev)
    g = torch.randn(cols, dtype=torch.float32, device=dev)
    ws = torch.empty(ops.sparse_workspace(n, cols), dtype=torch.uint8, device=dev)
    variants, meta = {}, {}
    for ratio in (float(r) for r in a.ratios.split(",")):
        k = max(1, int(ratio * cols))
        p = pairs_of(n, cols, k, dev)
        variants[f"sparse_{ratio}"] = lambda p=p: ops.sparse_fold_stack(p, w, None, acc, workspace=ws)
        variants[f"sparse_{ratio}_center"] = lambda p=p: ops.sparse_fold_stack(p, w, None, acc, center=g, wsum=50.0, workspace=ws)
        meta[f"sparse_{ratio}"] = {"k": k, "floor_ms": (p.numel() * 4 + 4 * cols) / 8e12 * 1e3,
                                   "floor_center_ms": (p.numel() * 4 + 8 * cols) / 8e12 * 1e3}
    if not a.no_dense:
        dense = torch.empty(n, cols, dtype=torch.float32, device=dev)
        ops.fill_uniform(dense, 7)
        variants["fold_f32_dense"] = lambda: ops.fold_stack(na.ACC_F32, dense, w, None, acc)
    res = timed(variants)
    ops.sparse_fold_stack(next(iter(variants.values())).__defaults__[0], w, None, acc, workspace=ws)
    line = {"device": torch.cuda.get_device_name(0), "clients": n, "cols": cols, "kernel": ops.last_launch(), "lib": a.lib,
            "reps": REPS, "results": res, "meta": meta}
    print(json.dumps(line))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
