"""GPU: rounds of 1-bit sign uploads through QuantizedAVG(bits=1) and Aggregator.ensemble_quantized, on a
two-tensor model (one of two chunks, one ragged: 129 elements) with an int64 counter.  The oracle is the
engine itself on the dequantized uploads — Aggregator.ensemble over quant.dequantize_state_dict of the same
uploads — compared key by key: type, dtype and bytes (test_gpu_quant_round.same)."""
import numpy as np
import pytest

from flearn_amd import AVG, QuantizedAVG, layouts, quant
from flearn_amd.aggregator import Aggregator, ServerOptimizer
from test_gpu_quant_round import _host, same, upload

pytestmark = pytest.mark.gpu

LAYOUT = [("w", (40, 70), "f32"), ("odd", (129,), "f32"), ("steps", (), "i64")]
FLOATS = layouts.fp32_elems(LAYOUT)
W = [0.5, 1.0, 2.25, 0.125, 3.0, 1.5, 0.75]


def models(n, seed, around=None):
    """n state dicts on LAYOUT: random, or `around` (a w_glob) plus a small update; counters differ."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        sd = layouts.synthetic_state_dict(LAYOUT, rng.standard_normal(FLOATS).astype(np.float32), counter=10 * i + seed)
        if around is not None:
            sd = {k: (_host(around[k]).astype(np.float32) + np.float32(1e-3) * v).astype(np.float32) if v.dtype == np.float32 else v
                  for k, v in sd.items()}
        out.append(sd)
    return out


@pytest.mark.parametrize("op", [None, "avgm", "adam"])
@pytest.mark.parametrize("chunk", [None, 3])
@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("output", ["reference", "float32", "device"])
def test_two_rounds_are_avg_over_the_dequantized_uploads(output, delta, chunk, op, cuda):
    g = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in models(1, 11)[0].items()}
    centre = {k: v.astype(np.float32) if v.dtype == np.float64 else v for k, v in g.items()}
    opt, twin = (ServerOptimizer(op), ServerOptimizer(op)) if op else (None, None)
    for o in filter(None, (opt, twin)):
        o.init_global({k: v for k, v in centre.items() if v.dtype == np.float32})
    s, eng = QuantizedAVG(server_opt=opt, delta=delta, output=output, chunk_clients=chunk, bits=1), Aggregator(output=output)
    s.init_global(g)
    for r in range(2):
        c = centre if delta else None
        qs = [quant.quantize_state_dict(m, center=c, bits=1) for m in models(len(W), 50 + r, around=centre)]
        got = s.server(upload(qs, W), r)["w_glob"]
        same(got, eng.ensemble(W, [quant.dequantize_state_dict(q, center=c) for q in qs], server_opt=twin), f"round {r}")
        if op:
            same(opt.state_dict()["v_t"], twin.state_dict()["v_t"], f"round {r} v_t")
        g32 = s.engine.last_plan.groups["f32"]
        assert g32.stride == 4096 and [sg.offset for sg in g32.segments] == [0, 2816]  # 128-column boundaries, a 2048 stride
        assert s.engine.last_quant == {"bytes_in": len(W) * 4096 // 8 + 4 * len(W) * 32, "delta": delta, "blocks": len(W) * 32,
                                       "bytes_fp32": 4 * len(W) * layouts.padded_f32_stride(LAYOUT), "bits": 1}
        centre = {k: _host(v).astype(np.float32) if _host(v).dtype.kind == "f" else _host(v) for k, v in got.items()}


def test_a_plain_round_takes_avg_s_path(cuda):
    ms = models(len(W), 3)
    s = QuantizedAVG(bits=1)
    same(s.server(upload(ms, W), 0)["w_glob"], AVG().server(upload(ms, W), 0)["w_glob"], "plain")
    assert s.engine.last_quant is None
