"""Capture float16 golden vectors from the REFERENCE implementation (wnma3mz/flearn v0.0.5).

Same rules and file format as make_golden.py (whose Case it uses): runs only where the reference
is importable, stores inputs + the reference's outputs as data, copies nothing from it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_half.py

Cases (tests/golden/half_*.npz): the five rows of DESIGN.md section 10's table — numpy float16
uploads x Python float / np.float16 / np.float32 / np.float64 weights, torch float16 uploads x
Python float weights — each at N in {1, 3, 10} with keys of 1, 9 and 513 elements; Python int and
bool weights; a model.half() LeNet-style layout with an int64 counter (numpy and torch uploads);
BN / LG key filters; sums that overflow to inf; the weak weight 70000 (inf as a half, NaN result);
subnormal-heavy values; and what load_state_dict of the result leaves in a half module.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True

from make_golden import REF, Case, upload  # noqa: E402

ROWS = {
    "pyfloat": float,
    "np16": np.float16,
    "np32": np.float32,
    "np64": np.float64,
}
HALF_LENET = [
    ("conv1.weight", (6, 1, 5, 5)),
    ("conv1.bias", (6,)),
    ("bn1.weight", (6,)),
    ("bn1.bias", (6,)),
    ("bn1.running_mean", (6,)),
    ("bn1.running_var", (6,)),
    ("bn1.num_batches_tracked", ()),
    ("fc1.weight", (31, 96)),
    ("fc1.bias", (31,)),
    ("fc2.weight", (10, 31)),
    ("fc2.bias", (10,)),
]


def half_values(rng, shape, scale=1.0):
    """Normal values with subnormals, signed zeros and a few large magnitudes mixed in."""
    x = (rng.standard_normal(shape) * scale).astype(np.float16)
    k = rng.integers(0, 12, size=shape)
    x = np.where(k == 0, (rng.standard_normal(shape) * 3e-6).astype(np.float16), x)
    x = np.where(k == 1, np.float16(-0.0), x)
    x = np.where(k == 2, (rng.standard_normal(shape) * 900).astype(np.float16), x)
    return np.ascontiguousarray(x.astype(np.float16))


def model_clients(rng, n, scale=1.0):
    out = []
    for i in range(n):
        d = {}
        for k, s in HALF_LENET:
            d[k] = np.array(7 + 3 * i, dtype=np.int64) if s == () else half_values(rng, s, scale)
        out.append(d)
    return out


def to_torch(clients):
    import torch

    return [{k: torch.from_numpy(np.array(v, copy=True)) for k, v in c.items()} for c in clients]


def capture(name, strategy, clients, ws, torch_inputs=False, call="AVG().server(lst, 0)", extra=None, **meta):
    c = Case(name, call=call, **({"input_kind": "torch"} if torch_inputs else {}), **meta)
    c.inputs(clients, list(clients[0]), store=True)
    c.weights(ws)
    with np.errstate(all="ignore"):
        out = strategy.server(upload(to_torch(clients) if torch_inputs else clients, ws), 0)["w_glob"]
    c.output(out)
    if extra is not None:
        extra(c, out)
    c.save()
    return out


def main():
    if not (REF / "flearn").is_dir():
        print(f"reference not found at {REF}; golden capture skipped")
        return 0
    sys.path.insert(0, str(REF))
    import torch
    from flearn.common.strategy import AVG, BN, LG

    rng = np.random.default_rng(20261019)
    base = [0.3, 1.7, 0.9, 2.3, 0.11, 1.0, 0.55, 2.9, 0.7, 1.3]

    # 1. the table's rows x N x P
    for n in (1, 3, 10):
        clients = [{f"p{p}": half_values(rng, (p,)) for p in (1, 9, 513)} for _ in range(n)]
        for row, typ in ROWS.items():
            capture(f"half_{row}_n{n}", AVG(), clients, [typ(w) for w in base[:n]])
        capture(f"half_torch_n{n}", AVG(), clients, base[:n], torch_inputs=True)
    clients = [{f"p{p}": half_values(rng, (p,)) for p in (1, 9, 513)} for _ in range(3)]
    capture("half_pyint_n3", AVG(), clients, [3, 1, 7])
    capture("half_pybool_n3", AVG(), clients, [True, False, True])
    capture("half_torch_pyint_n3", AVG(), clients, [3, 1, 7], torch_inputs=True)

    # 2. a model.half() layout with its int64 counter, and load_state_dict into a half module
    def loaded(c, out):
        res = {}
        for k, v in out.items():
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
            if t.is_floating_point():
                p = torch.zeros(t.shape, dtype=torch.float16)
                p.copy_(t)  # what Module.load_state_dict does per parameter
                res[k] = p.numpy()
        c.output(res, prefix="loaded")

    mc = model_clients(rng, 4)
    ws = [1.0, 2.0, 0.5, 1.5]
    capture("half_model_n4", AVG(), mc, ws, extra=loaded)
    capture("half_model_torch_n4", AVG(), mc, ws, torch_inputs=True, extra=loaded)
    capture("half_model_pyint_n4", AVG(), mc, [3, 1, 4, 2])
    capture("half_bn_n4", BN(), mc, ws, call="BN().server(lst, 0)")
    shared = ["fc2.weight", "fc2.bias"]
    capture("half_lg_n4", LG(shared), mc, ws, call="LG(shared_key_layers).server(lst, 0)", shared_key_layers=shared)

    # 3. range edges
    over = [{"x": np.full(16, 30.0, dtype=np.float16)} for _ in range(7)]
    capture("half_overflow_n7", AVG(), over, [600] * 7)
    capture("half_overflow_torch_n7", AVG(), over, [600.0] * 7, torch_inputs=True)
    capture("half_w70000_n3", AVG(), [{"x": half_values(rng, (40,))} for _ in range(3)], [70000, 1.0, 1.0])
    sub = [{"x": (rng.standard_normal(2048) * 1e-4).astype(np.float16)} for _ in range(5)]
    capture("half_subnormal_n5", AVG(), sub, [0.11, 0.7, 0.05, 0.9, 0.33])
    capture("half_subnormal_torch_n5", AVG(), sub, [0.11, 0.7, 0.05, 0.9, 0.33], torch_inputs=True)
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
