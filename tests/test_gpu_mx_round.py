"""GPU: rounds of Microscaling uploads through QuantizedAVG(bits=b, format="mx") and
Aggregator.ensemble_quantized, on tensors of 1, 33, 300 and 2500 elements with an int64 counter.  The oracle is
the engine itself on the dequantized uploads — Aggregator.ensemble over quant.dequantize_state_dict of the same
uploads — compared key by key: type, dtype and bytes (test_gpu_quant_round.same)."""
import numpy as np
import pytest

from flearn_amd import QuantizedAVG, layouts, quant
from flearn_amd.aggregator import Aggregator, ServerOptimizer
from test_gpu_quant_round import _host, same, upload

pytestmark = pytest.mark.gpu

LAYOUT = [("one", (1,), "f32"), ("b", (33,), "f32"), ("w", (30, 10), "f32"), ("wide", (50, 50), "f32"), ("steps", (), "i64")]
FLOATS = layouts.fp32_elems(LAYOUT)
W = [0.5, 1.0, 2.25, 0.125, 3.0]
OFFSETS = [0, 32, 96, 416]  # 32-column boundaries
STRIDE = 4096  # 416 + 2500 columns, up to a multiple of 2048


def models(n, seed, around):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        sd = layouts.synthetic_state_dict(LAYOUT, rng.standard_normal(FLOATS).astype(np.float32), counter=10 * i + seed)
        out.append({k: (_host(around[k]).astype(np.float32) + np.float32(1e-2) * v).astype(np.float32) if v.dtype == np.float32 else v
                    for k, v in sd.items()})
    return out


@pytest.mark.parametrize("delta,chunk,op", [(False, None, None), (False, 2, None), (True, None, None), (True, 2, None),
                                            (True, None, "avgm")])
@pytest.mark.parametrize("bits", [4, 8])
def test_two_rounds_are_avg_over_the_dequantized_uploads(bits, delta, chunk, op, cuda):
    g = {k: v.astype(np.float64) if v.dtype == np.float32 else v
         for k, v in layouts.synthetic_state_dict(LAYOUT, np.random.default_rng(11).standard_normal(FLOATS).astype(np.float32), counter=1).items()}
    centre = {k: v.astype(np.float32) if v.dtype == np.float64 else v for k, v in g.items()}
    opt, twin = (ServerOptimizer(op), ServerOptimizer(op)) if op else (None, None)
    for o in filter(None, (opt, twin)):
        o.init_global({k: v for k, v in centre.items() if v.dtype == np.float32})
    s, eng = QuantizedAVG(server_opt=opt, delta=delta, chunk_clients=chunk, bits=bits, format="mx"), Aggregator()
    s.init_global(g)
    for r in range(2):
        c = centre if delta else None
        qs = [quant.quantize_state_dict(m, center=c, bits=bits, format="mx") for m in models(len(W), 50 + r, centre)]
        got = s.server(upload(qs, W), r)["w_glob"]
        same(got, eng.ensemble(W, [quant.dequantize_state_dict(q, center=c) for q in qs], server_opt=twin), f"round {r}")
        g32 = s.engine.last_plan.groups["f32"]
        assert g32.stride == STRIDE and [sg.offset for sg in g32.segments] == OFFSETS
        assert s.engine.last_quant == {"bytes_in": len(W) * STRIDE * bits // 8 + len(W) * STRIDE // 32, "delta": delta,
                                       "blocks": len(W) * STRIDE // 32, "bits": bits, "format": "mx",
                                       "bytes_fp32": 4 * len(W) * layouts.padded_f32_stride(LAYOUT)}
        centre = {k: _host(v).astype(np.float32) if _host(v).dtype.kind == "f" else _host(v) for k, v in got.items()}
