"""GPU: rounds of int8 block-quantized uploads through QuantizedAVG and Aggregator.ensemble_quantized,
on the LeNet5 layout plus a 3-element tensor, a 1025-element tensor and an int64 counter.  The oracle
is the engine itself on the dequantized uploads — AVG().server / Aggregator.ensemble over
quant.dequantize_state_dict of the same uploads — compared key by key: type, dtype and bytes."""
import numpy as np
import pytest
import torch

import quant_ref as qr
from flearn_amd import AVG, QuantizedAVG, layouts, quant, setup_strategy
from flearn_amd.aggregator import Aggregator, ServerOptimizer

pytestmark = pytest.mark.gpu

OUTPUTS = ("reference", "float32", "device")
N = 5
LAYOUT = layouts.get("lenet5") + [("tiny", (3,), "f32"), ("odd", (1025,), "f32"), ("steps", (), "i64")]
FLOATS = layouts.fp32_elems(LAYOUT)


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def models(n, seed, around=None, step=0.05):
    """n state dicts on LAYOUT: random, or `around` (a w_glob) plus a small update; counters differ."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        flat = rng.standard_normal(FLOATS).astype(np.float32)
        sd = layouts.synthetic_state_dict(LAYOUT, flat, counter=10 * i + seed)
        if around is not None:
            for k, v in sd.items():
                if v.dtype == np.float32:
                    sd[k] = (_host(around[k]).astype(np.float32) + np.float32(step) * v).astype(np.float32)
        out.append(sd)
    return out


def upload(params, weights):
    return [{"agg_weight": a, "params": p} for a, p in zip(weights, params)]


def same(got, want, where):
    assert list(got) == list(want), f"{where}: key order"
    for k in want:
        g, w = got[k], want[k]
        assert type(g) is type(w), f"{where}: {k} {type(g)} {type(w)}"
        if isinstance(g, torch.Tensor):
            assert g.is_cuda == w.is_cuda, f"{where}: {k}"
        assert _host(g).dtype == _host(w).dtype and _host(g).shape == _host(w).shape, f"{where}: {k}"
        assert _host(g).tobytes() == _host(w).tobytes(), f"{where}: {k}"


WEIGHTS = {"pyfloat": [0.5, 1.0, 2.25, 0.125, 3.0], "np32": [np.float32(w) for w in (0.5, 1.0, 2.25, 0.125, 3.0)],
           "pyint": [3, 1, 4, 1, 5]}


@pytest.fixture(scope="module")
def plain():
    return models(N, 1)


@pytest.fixture(scope="module")
def quantized(plain):
    return [quant.quantize_state_dict(m) for m in plain]


@pytest.fixture(scope="module")
def dequantized(quantized):
    return [quant.dequantize_state_dict(q) for q in quantized]


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("wkind", sorted(WEIGHTS))
def test_round_is_avg_over_the_dequantized_uploads(wkind, output, plain, quantized, dequantized, cuda):
    w = WEIGHTS[wkind]
    got = QuantizedAVG(output=output).server(upload(quantized, w), 0)["w_glob"]
    want = AVG(output=output).server(upload(dequantized, w), 0)["w_glob"]
    same(got, want, f"{wkind} {output}")
    if output == "reference":
        assert _host(got["fc1.weight"]).dtype == (np.float32 if wkind == "np32" else np.float64)
        assert _host(got["steps"]).dtype == np.float64
        # the numpy restatement: the running fp32 sum of fl32(a_i * fl32(s * q)), divided as the engine divides
        k = "odd"
        codes = np.stack([q[k]["q8"] for q in quantized])
        acc = qr.deq_fold(None, codes, np.stack([q[k]["scale"] for q in quantized]), np.array(w, dtype=np.float32))
        ref = acc / np.float32(np.sum(w)) if wkind == "np32" else acc.astype(np.float64) / float(np.sum(w))
        assert _host(got[k]).tobytes() == ref.tobytes()
    # the quantization itself stays within its bound of the clients' models
    err = max(np.abs(d["fc1.weight"] - p["fc1.weight"]).max() / q["fc1.weight"]["scale"].max()
              for d, p, q in zip(dequantized, plain, quantized))
    assert err <= 0.5 + 2.0 ** -16


@pytest.mark.parametrize("output", OUTPUTS)
def test_engine_entry_chunks_and_audit(output, quantized, dequantized, cuda):
    w = WEIGHTS["pyfloat"]
    want = Aggregator(output=output).ensemble(w, dequantized)
    for k in (None, 1, 2, 5, 9):
        eng = Aggregator(output=output, chunk_clients=k)
        same(eng.ensemble_quantized(w, quantized), want, f"chunk_clients={k} {output}")
        g32 = eng.last_plan.groups["f32"]
        assert g32.stride % 1024 == 0 and all(s.offset % 1024 == 0 for s in g32.segments)
        assert g32.stride == sum(-(-max(s.numel, 1) // 1024) * 1024 for s in g32.segments)
        assert eng.last_quant == {"bytes_in": N * g32.stride + 4 * N * g32.stride // 1024,
                                  "bytes_fp32": 4 * N * layouts.padded_f32_stride(LAYOUT), "delta": False,
                                  "blocks": N * g32.stride // 1024}
        same(eng.ensemble_quantized(w, quantized), want, f"again, chunk_clients={k} {output}")  # reused plan and buffers
    sub = ["odd", "steps", "conv1.bias"]
    same(Aggregator(output=output).ensemble_quantized(w, quantized, key_lst=sub),
         Aggregator(output=output).ensemble(w, dequantized, sub), f"key_lst {output}")


def test_seventeen_clients_and_the_stack_s_actual_size(cuda):
    n = 17
    ms = models(n, 3)
    qs = [quant.quantize_state_dict(m) for m in ms]
    w = [float(i % 4 + 1) for i in range(n)]
    eng = Aggregator()
    got = eng.ensemble_quantized(w, qs)
    same(got, Aggregator().ensemble(w, [quant.dequantize_state_dict(q) for q in qs]), "17 clients")
    stride = eng.last_plan.groups["f32"].stride
    dq = eng.packer.device_bucket(("q8", 0), (n, stride), torch.int8, eng.device)
    ds = eng.packer.device_bucket(("q8s", 0), (n, stride // 1024), torch.float32, eng.device)
    actual = dq.numel() * dq.element_size() + ds.numel() * ds.element_size()
    assert eng.last_quant["bytes_in"] == actual == n * stride + 4 * n * (stride // 1024)
    assert eng.last_quant["bytes_in"] * 3 < eng.last_quant["bytes_fp32"]  # a quarter, but for this small model's 1024-column padding
    # what the device holds is the uploads' codes, padding code 0 under scale 0
    host = dq.cpu().numpy()
    for s in eng.last_plan.groups["f32"].segments:
        assert (host[:, s.offset : s.offset + s.numel] == np.stack([q[s.key]["q8"].reshape(-1) for q in qs])).all()
        assert (host[:, s.offset + s.numel : s.offset - (-max(s.numel, 1) // 1024) * 1024] == 0).all()


@pytest.mark.parametrize("op", ["avgm", "adam"])
@pytest.mark.parametrize("wkind", ["pyfloat", "np32"])
def test_server_optimiser_over_two_rounds(op, wkind, cuda):
    w = WEIGHTS[wkind]
    g0 = models(1, 7)[0]
    opt, twin = ServerOptimizer(op), ServerOptimizer(op)
    opt.init_global({k: v for k, v in g0.items() if v.dtype == np.float32})
    twin.init_global({k: v for k, v in g0.items() if v.dtype == np.float32})
    s, eng = QuantizedAVG(server_opt=opt, delta=False), Aggregator()
    for r in range(2):
        qs = [quant.quantize_state_dict(m) for m in models(N, 40 + r, around=g0)]
        got = s.server(upload(qs, w), r)["w_glob"]
        want = eng.ensemble(w, [quant.dequantize_state_dict(q) for q in qs], server_opt=twin)
        same(got, want, f"{op} {wkind} round {r}")
        a, b = opt.state_dict(), twin.state_dict()
        for part in ("w_glob", "v_t"):
            same(a[part], b[part], f"{op} {wkind} round {r} {part}")


@pytest.mark.parametrize("output", OUTPUTS)
def test_delta_rounds(output, cuda):
    w = WEIGHTS["pyfloat"]
    g = models(1, 11)[0]
    g = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in g.items()}  # what a float64 w_glob looks like
    g32 = {k: v.astype(np.float32) if v.dtype == np.float64 else v for k, v in g.items()}
    s, ref = QuantizedAVG(output=output), AVG(output=output)
    s.init_global(g)
    centre = g32
    for r in range(2):
        ms = models(N, 50 + r, around=centre, step=1e-3)
        qs = [quant.quantize_state_dict(m, center=centre) for m in ms]
        assert all(q["odd"]["delta"] is True for q in qs)
        got = s.server(upload(qs, w), r)["w_glob"]
        assert s.engine.last_quant["delta"] is True
        yhat = [quant.dequantize_state_dict(q, center=centre) for q in qs]
        for y, q in zip(yhat, qs):  # fl32(g + fl32(s * q))
            assert y["odd"].tobytes() == qr.dequantize(q["odd"]["q8"], q["odd"]["scale"], centre["odd"]).tobytes()
        same(got, ref.server(upload(yhat, w), r)["w_glob"], f"delta round {r} {output}")
        # the update is small: delta codes resolve it far finer than codes of the model itself would
        assert qs[0]["fc1.weight"]["scale"].max() < quant.quantize_state_dict(ms[0])["fc1.weight"]["scale"].max() / 50
        # the next round's centre, on both sides: this round's w_glob as fp32
        centre = {k: _host(v).astype(np.float32) if _host(v).dtype.kind == "f" else _host(v) for k, v in got.items()}
        for k in ("odd", "fc1.weight"):
            assert _host(s._prev_glob[k]).tobytes() == centre[k].tobytes()
    # a client that follows the strategy's own protocol produces exactly these uploads
    class Trainer:
        def __init__(self, sd):
            self.weight, self.model = sd, self

        def load_state_dict(self, sd):
            pass

    c = QuantizedAVG()
    c.client_receive(Trainer(dict(ms[0])), {"w_glob": {k: _host(v) for k, v in got.items()}})
    mine = c.client(Trainer(dict(ms[1])), 1.0)["params"]
    want = quant.quantize_state_dict(ms[1], center=centre)
    assert (mine["odd"]["q8"] == want["odd"]["q8"]).all() and mine["odd"]["scale"].tobytes() == want["odd"]["scale"].tobytes()


def test_plain_uploads_take_avg_s_path(plain, cuda):
    w = WEIGHTS["pyfloat"]
    for kw in ({}, {"chunk_clients": 2}, {"output": "float32"}):
        s = QuantizedAVG(**kw)
        same(s.server(upload(plain, w), 0)["w_glob"], AVG(**kw).server(upload(plain, w), 0)["w_glob"], f"plain {kw}")
        assert s.engine.last_quant is None
    assert type(setup_strategy("avg_q8", None)) is QuantizedAVG


def test_torch_uploads_and_wire_decoded_uploads(quantized, dequantized, cuda):
    from flearn_amd import Encrypt

    w = WEIGHTS["pyfloat"]
    want = AVG().server(upload(dequantized, w), 0)["w_glob"]
    enc = Encrypt()
    wired = [enc.decode(enc.encode(u)) for u in upload(quantized, w)]
    same(QuantizedAVG(encrypt=enc).server(wired, 0)["w_glob"], want, "wire")
    as_t = [{k: ({**v, "q8": torch.from_numpy(v["q8"]), "scale": torch.from_numpy(v["scale"])} if quant.is_entry(v) else v)
             for k, v in q.items()} for q in quantized]
    same(QuantizedAVG().server(upload(as_t, w), 0)["w_glob"], want, "torch codes")


def test_refusals_leave_the_engine_usable(quantized, dequantized, cuda):
    w = WEIGHTS["pyfloat"]
    s = QuantizedAVG()
    bad = [dict(q) for q in quantized]
    bad[2]["odd"] = dict(bad[2]["odd"], scale=np.array([1.0, -1.0], dtype=np.float32))
    with pytest.raises(SystemExit):
        s.server(upload(bad, w), 0)
    on_device = [dict(q) for q in quantized]
    on_device[0]["odd"] = dict(on_device[0]["odd"], q8=torch.from_numpy(quantized[0]["odd"]["q8"]).to(cuda))
    with pytest.raises(TypeError, match="device-resident"):
        s.engine.ensemble_quantized(w, on_device)
    with pytest.raises(TypeError, match="float64"):
        s.engine.ensemble_quantized([np.float64(a) for a in w], quantized)
    same(s.server(upload(quantized, w), 1)["w_glob"], AVG().server(upload(dequantized, w), 1)["w_glob"], "after refusals")
