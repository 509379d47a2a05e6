"""GPU: rounds of bfloat16 uploads (BF16AVG, Aggregator.ensemble_bf16) against the engine on the same uploads
widened to fp32, key by key: type, dtype and bytes; one key also against the numpy restatement."""
import numpy as np
import pytest
import torch

import bf16_ref as br
from flearn_amd import AVG, BF16AVG, bf16
from flearn_amd.aggregator import Aggregator, ServerOptimizer

pytestmark = pytest.mark.gpu

N = 5
SHAPES = {"one": (1,), "seven": (7,), "b": (150,), "w1": (48, 50), "w2": (160, 300)}  # 1, 7, 150, 2400, 48 000
upload = lambda params, weights: [{"agg_weight": a, "params": p} for a, p in zip(weights, params)]  # noqa: E731
WEIGHTS = {"pyfloat": [0.5, 1.0, 2.25, 0.125, 3.0], "np32": [np.float32(w) for w in (0.5, 1.0, 2.25, 0.125, 3.0)]}


def models(seed, around=None):
    """N fp32 state dicts (random, or `around` plus a small update) with an int64 counter."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N):
        sd = {k: rng.standard_normal(s).astype(np.float32) for k, s in SHAPES.items()}
        if around is not None:
            sd = {k: (around[k] + np.float32(0.05) * v).astype(np.float32) for k, v in sd.items()}
        sd["steps"] = np.array(10 * i + seed, dtype=np.int64)
        out.append(sd)
    return out


def host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def same(got, want, where, types=True):
    assert list(got) == list(want), where
    for k in want:
        g, w = got[k], want[k]
        assert not types or type(g) is type(w), f"{where}: {k} {type(g)} {type(w)}"
        assert host(g).dtype == host(w).dtype and host(g).shape == host(w).shape, f"{where}: {k}"
        assert host(g).tobytes() == host(w).tobytes(), f"{where}: {k}"


@pytest.fixture(scope="module")
def wire():
    return [bf16.encode_state_dict(m) for m in models(1)]


@pytest.mark.parametrize("output", ["reference", "float32", "device"])
@pytest.mark.parametrize("wkind", sorted(WEIGHTS))
def test_round_is_avg_over_the_widened_uploads(wkind, output, wire, cuda):
    w, widened = WEIGHTS[wkind], [bf16.decode_state_dict(u) for u in wire]
    s = BF16AVG(output=output)
    got = s.server(upload(wire, w), 0)["w_glob"]
    same(got, AVG(output=output).server(upload(widened, w), 0)["w_glob"], f"{wkind} {output}")
    same(BF16AVG(output=output, chunk_clients=2).server(upload(wire, w), 0)["w_glob"], got, "chunk_clients=2")
    lb, g32 = s.engine.last_bf16, s.engine.last_plan.groups["f32"]
    assert g32.stride % 64 == 0 and all(seg.offset % 8 == 0 for seg in g32.segments)
    assert lb["bytes_in"] == 2 * N * g32.stride and 0 <= lb["bytes_fp32"] - 2 * lb["bytes_in"] <= 4 * N * 64 * len(SHAPES)
    if output == "reference":  # the numpy restatement, divided as the engine divides
        acc = br.fold(None, [u["w2"]["bf16"].reshape(-1) for u in wire], np.array(w, dtype=np.float32))
        ref = acc / np.float32(np.sum(w)) if wkind == "np32" else acc.astype(np.float64) / float(np.sum(w))
        assert host(got["w2"]).reshape(-1).tobytes() == ref.tobytes() and host(got["steps"]).dtype == np.float64


def test_wire_entries_cpu_tensors_and_device_tensors_give_the_same_bits(wire, cuda):
    w = WEIGHTS["pyfloat"]
    cpu = [{k: torch.from_numpy(v["bf16"].view(np.int16)).view(torch.bfloat16) if bf16.is_entry(v) else torch.from_numpy(v)
            for k, v in u.items()} for u in wire]
    dev = [{k: v.to(cuda) for k, v in u.items()} for u in cpu]
    want = Aggregator(output="float32").ensemble_bf16(w, wire)
    mixed = [cpu[0]] + [dict(d, steps=c["steps"]) for c, d in zip(cpu[1:], dev[1:])]  # the counters stay on the host
    for name, ups in (("cpu", cpu), ("device", dev), ("mixed", mixed)):
        for k in (None, 2):
            same(Aggregator(output="float32", chunk_clients=k).ensemble_bf16(w, ups), want, f"{name} {k}", types=False)
    with pytest.raises(TypeError):  # unchanged: the plain round refuses bfloat16
        Aggregator().ensemble(w, cpu)


@pytest.mark.parametrize("wkind", sorted(WEIGHTS))
def test_fused_avgm_over_two_rounds(wkind, cuda):
    w = WEIGHTS[wkind]
    g0 = {k: v for k, v in models(7)[0].items() if v.dtype == np.float32}
    opt, twin = ServerOptimizer("avgm"), ServerOptimizer("avgm")
    opt.init_global(g0)
    twin.init_global(g0)
    s, eng = BF16AVG(server_opt=opt), Aggregator()
    for r in range(2):
        ups = [bf16.encode_state_dict(m) for m in models(40 + r, around=g0)]
        got = s.server(upload(ups, w), r)["w_glob"]
        same(got, eng.ensemble(w, [bf16.decode_state_dict(u) for u in ups], server_opt=twin), f"round {r}")
        for part in ("w_glob", "v_t"):
            same(opt.state_dict()[part], twin.state_dict()[part], f"round {r} {part}")
