"""GPU: rounds of int4 block-quantized uploads through QuantizedAVG(bits=4) and
Aggregator.ensemble_quantized, on the LeNet5 layout plus a 3-element tensor, a 129-element tensor and
an int64 counter.  The oracle is the engine itself on the dequantized uploads — AVG().server /
Aggregator.ensemble over quant.dequantize_state_dict of the same uploads — compared key by key: type,
dtype and bytes (test_gpu_quant_round.same)."""
import numpy as np
import pytest

import quant4_ref as q4r
from flearn_amd import AVG, Encrypt, QuantizedAVG, layouts, quant, setup_strategy
from flearn_amd.aggregator import Aggregator, ServerOptimizer
from test_gpu_quant_round import _host, same, upload

pytestmark = pytest.mark.gpu

OUTPUTS = ("reference", "float32", "device")
LAYOUT = layouts.get("lenet5") + [("tiny", (3,), "f32"), ("odd", (129,), "f32"), ("steps", (), "i64")]
FLOATS = layouts.fp32_elems(LAYOUT)
WEIGHTS = {"pyfloat": [0.5, 1.0, 2.25, 0.125, 3.0], "np32": [np.float32(w) for w in (0.5, 1.0, 2.25, 0.125, 3.0)]}


def models(n, seed, around=None, step=0.05):
    """n state dicts on LAYOUT: random, or `around` (a w_glob) plus a small update; counters differ."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        sd = layouts.synthetic_state_dict(LAYOUT, rng.standard_normal(FLOATS).astype(np.float32), counter=10 * i + seed)
        if around is not None:
            sd = {k: (_host(around[k]).astype(np.float32) + np.float32(step) * v).astype(np.float32) if v.dtype == np.float32 else v
                  for k, v in sd.items()}
        out.append(sd)
    return out


@pytest.fixture(scope="module", params=[5, 17])
def round_(request):
    """(weights by kind, the 4-bit uploads, the same uploads dequantized) of 5 and of 17 clients."""
    n = request.param
    qs = [quant.quantize_state_dict(m, bits=4) for m in models(n, n)]
    w = {k: (v * 4)[:n] for k, v in WEIGHTS.items()}
    return w, qs, [quant.dequantize_state_dict(q) for q in qs]


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("wkind", sorted(WEIGHTS))
def test_round_is_avg_over_the_dequantized_uploads(wkind, output, round_, cuda):
    ws, qs, deq = round_
    w = ws[wkind]
    s = setup_strategy("avg_q4", None, output=output)
    got = s.server(upload(qs, w), 0)["w_glob"]
    same(got, AVG(output=output).server(upload(deq, w), 0)["w_glob"], f"{wkind} {output}")
    assert s.engine.last_quant["bits"] == 4 and s.engine.last_quant["delta"] is False


def test_engine_entry_chunks_layout_and_audit(round_, cuda):
    ws, qs, deq = round_
    w, n = ws["pyfloat"], len(qs)
    want = Aggregator().ensemble(w, deq)
    for k in (None, 1, 2, 9):
        eng = Aggregator(chunk_clients=k)
        same(eng.ensemble_quantized(w, qs), want, f"chunk_clients={k}")
        g32 = eng.last_plan.groups["f32"]
        assert g32.stride % 2048 == 0 and all(s.offset % 128 == 0 for s in g32.segments)
        assert g32.stride == -(-sum(-(-s.numel // 128) * 128 for s in g32.segments) // 2048) * 2048
        assert eng.last_quant == {"bytes_in": n * g32.stride // 2 + 4 * n * g32.stride // 128,
                                  "bytes_fp32": 4 * n * layouts.padded_f32_stride(LAYOUT), "delta": False,
                                  "blocks": n * g32.stride // 128, "bits": 4}
        same(eng.ensemble_quantized(w, qs), want, f"again, chunk_clients={k}")  # reused plan and buffers
    sub = ["odd", "steps", "conv1.bias"]
    same(Aggregator().ensemble_quantized(w, qs, key_lst=sub), Aggregator().ensemble(w, deq, sub), "key_lst")


@pytest.mark.parametrize("op", [None, "avgm"])
def test_delta_and_server_optimiser_over_two_rounds(op, cuda):
    w = WEIGHTS["pyfloat"]
    g = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in models(1, 11)[0].items()}
    centre = {k: v.astype(np.float32) if v.dtype == np.float64 else v for k, v in g.items()}
    opt, twin = (ServerOptimizer(op), ServerOptimizer(op)) if op else (None, None)
    for o in filter(None, (opt, twin)):
        o.init_global({k: v for k, v in centre.items() if v.dtype == np.float32})
    s, eng = QuantizedAVG(server_opt=opt, bits=4), Aggregator()
    s.init_global(g)
    for r in range(2):
        ms = models(5, 50 + r, around=centre, step=1e-3)
        qs = [quant.quantize_state_dict(m, center=centre, bits=4) for m in ms]
        got = s.server(upload(qs, w), r)["w_glob"]
        assert s.engine.last_quant["delta"] is True and s.engine.last_quant["bits"] == 4
        yhat = [quant.dequantize_state_dict(q, center=centre) for q in qs]
        assert yhat[0]["odd"].tobytes() == q4r.dequantize(qs[0]["odd"]["q4"], 129, qs[0]["odd"]["scale"], centre["odd"]).tobytes()
        same(got, eng.ensemble(w, yhat, server_opt=twin), f"{op} round {r}")
        if op:
            same(opt.state_dict()["v_t"], twin.state_dict()["v_t"], f"{op} round {r} v_t")
        centre = {k: _host(v).astype(np.float32) if _host(v).dtype.kind == "f" else _host(v) for k, v in got.items()}


def test_wire_decoded_uploads_and_refusals(round_, cuda):
    ws, qs, deq = round_
    w = ws["pyfloat"]
    want = AVG().server(upload(deq, w), 0)["w_glob"]
    enc = Encrypt()
    s = QuantizedAVG(encrypt=enc, bits=4)
    same(s.server([enc.decode(enc.encode(u)) for u in upload(qs, w)], 0)["w_glob"], want, "wire")
    mixed = [dict(q) for q in qs]
    mixed[1] = quant.quantize_state_dict(quant.dequantize_state_dict(qs[1]))  # one q8 client
    with pytest.raises(ValueError, match="all q8 or all q4"):
        s.engine.ensemble_quantized(w, mixed)
    same(s.server(upload(qs, w), 1)["w_glob"], want, "after a refusal")
