"""GPU: rounds of top-k sparse uploads through TopKAVG and Aggregator.ensemble_sparse on a model with a key
smaller than k (sent whole), one smaller than a window, one that spans windows, and an int64 counter.
The weights sum to 8, so the server step applied to a reference sum S is the engine's own one-client round of
S / 8 with weight 8 (fl32(8 * S / 8) = S): the divide, the fused update and the output modes are compared
through it, bytes for bytes."""
import math

import numpy as np
import pytest

import sparse_ref as ref
from flearn_amd import TopKAVG, layouts, sparse
from flearn_amd.aggregator import Aggregator, ServerOptimizer
from flearn_amd.sparseround import weight_sum
from test_gpu_quant_round import _host, same, upload

pytestmark = pytest.mark.gpu

LAYOUT = [("tiny", (33,), "f32"), ("b", (300,), "f32"), ("wide", (100, 50), "f32"), ("steps", (), "i64")]
FLOATS = layouts.fp32_elems(LAYOUT)
K = 40
W = [0.5, 1.0, 2.25, 0.25, 4.0]  # sum 8
U = 2.0 ** -24


def model(seed, counter=1, around=None):
    sd = layouts.synthetic_state_dict(LAYOUT, np.random.default_rng(seed).standard_normal(FLOATS).astype(np.float32), counter=counter)
    if around is None:
        return sd
    return {k: (around[k] + np.float32(1e-2) * v).astype(np.float32) if v.dtype == np.float32 else v for k, v in sd.items()}


def ref_sums(ups, centre):
    """The rule's sum per fp32 key (sparse_ref.fold over the key's own columns)."""
    w32 = np.array(W, np.float32)
    return {k: ref.fold([(u[k]["idx"], u[k]["val"]) for u in ups], w32, math.prod(sparse.entry_shape(v)),
                        0, None if centre is None else centre[k].reshape(-1), weight_sum(w32)).reshape(sparse.entry_shape(v))
            for k, v in ups[0].items() if sparse.is_entry(v)}


def floats(d):
    return {k: v for k, v in d.items() if _host(v).dtype.kind == "f"}


def test_non_delta_round_is_avg_over_the_densified_uploads(cuda):
    ups = [sparse.sparsify_state_dict(model(20 + i, i), k=K) for i in range(len(W))]
    assert [u["tiny"]["idx"].size for u in ups] == [33] * len(W) and ups[0]["wide"]["idx"].size == K
    s = TopKAVG(delta=False, k=K)
    got = s.server(upload(ups, W), 0)["w_glob"]
    same(got, Aggregator().ensemble(W, [sparse.densify_state_dict(u) for u in ups]), "non-delta")
    assert s.engine.last_sparse == {"bytes_in": 8 * len(W) * (33 + 2 * K + 1), "bytes_fp32": 4 * len(W) * s.engine.last_plan.groups["f32"].stride,
                                    "delta": False, "nnz": len(W) * (33 + 2 * K), "kstride": 33 + 2 * K + 1}


@pytest.mark.parametrize("chunk,op,output", [(None, None, "reference"), (2, None, "reference"), (None, "avgm", "reference"),
                                             (2, "avgm", "float32"), (None, None, "device")])
def test_delta_round_is_the_rule_and_within_its_bound(chunk, op, output, cuda):
    centre = model(11)
    ups = [sparse.sparsify_state_dict(model(30 + i, i, centre), center=centre, k=K) for i in range(len(W))]
    opt, twin = (ServerOptimizer(op), ServerOptimizer(op)) if op else (None, None)
    for o in filter(None, (opt, twin)):
        o.init_global(floats(centre))
    s = TopKAVG(server_opt=opt, k=K, chunk_clients=chunk, output=output)
    s.init_global(centre)
    got = s.server(upload(ups, W), 0)["w_glob"]
    sums = ref_sums(ups, centre)
    want = Aggregator(output=output).ensemble([8.0], [{k: v / np.float32(8) for k, v in sums.items()}], server_opt=twin)
    same({k: got[k] for k in sums}, want, f"{chunk} {op} {output}")
    assert s.engine.last_sparse["delta"] is True and _host(got["steps"]) == _host(Aggregator().ensemble(W, [{"steps": u["steps"]} for u in ups])["steps"])
    if op is None:
        # |result - exact mean of the densified uploads| <= gamma(N + 4) * (|g| + sum a_i |u_i| / A)
        n = len(W)
        gamma = (n + 4) * U / (1 - (n + 4) * U)
        for k, g in floats(centre).items():
            dense = [sparse.densify_entry(u[k], g).astype(np.float64) for u in ups]
            exact = sum(a * d for a, d in zip(W, dense)) / 8.0
            mag = np.abs(g.astype(np.float64)) + sum(a * np.abs(d - g) for a, d in zip(W, dense)) / 8.0
            err = np.abs(_host(got[k]).astype(np.float64) - exact)
            print(k, "max error / bound:", float((err / (gamma * mag + 1e-300)).max()))
            assert (err <= gamma * mag + 2.0 ** -140).all()


def test_error_feedback_loses_nothing_over_two_rounds(cuda):
    c = TopKAVG(k=K)
    x0, x1, g = model(40), model(41), model(42)
    trainer = type("Trainer", (), {"weight": x0})()
    p0 = c.client(trainer)["params"]
    assert not p0["wide"]["delta"] and p0["steps"] == x0["steps"]
    for k, u in floats(x0).items():
        assert ref.same_bits(sparse.densify_entry(p0[k]) + c._residual[k], u)
    e0 = {k: v.copy() for k, v in c._residual.items()}
    assert np.count_nonzero(e0["wide"]) == 5000 - K and not e0["tiny"].any()
    c._received, trainer.weight = floats(g), x1  # what client_receive keeps of a w_glob
    p1 = c.client(trainer)["params"]
    assert p1["wide"]["delta"]
    for k, x in floats(x1).items():
        assert ref.same_bits(sparse.densify_entry(dict(p1[k], delta=False)) + c._residual[k], (x + e0[k]) - g[k])
