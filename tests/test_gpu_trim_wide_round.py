"""GPU: robust rounds of 300 clients through TrimmedMean(wide=True) / Median(wide=True)
(Aggregator.ensemble_trimmed -> fa_trim_sum_wide) against tests/robust_ref.py, bit for bit: the three
output modes, a server-fused AVGM step, a poisoned round and the refusals."""
import numpy as np
import pytest
import torch

import robust_ref as rr
from flearn_amd import Median, TrimmedMean, layouts, ops
from flearn_amd import _native as na
from flearn_amd.aggregator import ServerOptimizer

pytestmark = pytest.mark.gpu
N = 300


def upload(clients):
    return [{"agg_weight": 1.0, "params": c} for c in clients]


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.fixture(scope="module")
def clients():
    """300 synthetic LeNet5 clients with an int64 counter (the 8-byte kind's selection kernel)."""
    layout = layouts.get("lenet5") + [("steps", (), "i64")]
    flat = np.random.default_rng(300).standard_normal((N, layouts.fp32_elems(layout))).astype(np.float32)
    return [layouts.synthetic_state_dict(layout, flat[i], counter=i * i) for i in range(N)]


@pytest.fixture(scope="module")
def ref(clients):
    return {t: rr.ensemble(clients, t) for t in (30, rr.median_trim(N))}


@pytest.mark.parametrize("output", ["reference", "float32", "device"])
def test_plain_rounds(output, clients, ref, cuda):
    for s, t in ((TrimmedMean(0.1, output=output, wide=True), 30), (Median(output=output, wide=True), rr.median_trim(N))):
        got = s.server(upload(clients), 0)["w_glob"]
        assert list(got) == list(ref[t])
        for k, w in ref[t].items():
            w = np.asarray(w) if output == "reference" or k == "steps" else np.asarray(w).astype(np.float32)
            assert rr.same_bits(_host(got[k]), w), (type(s).__name__, output, k)


def test_server_fused_round(clients, cuda):
    """The expected step is the one-launch reduce kernel's over robust_ref's sums, as a one-row stack."""
    opt, k = ServerOptimizer("avgm"), "fc3.weight"
    prev = np.random.default_rng(9).standard_normal(clients[0][k].shape).astype(np.float32)
    opt.init_global({k: prev})
    got = TrimmedMean(30, server_opt=opt, wide=True).server(upload([{k: c[k]} for c in clients]), 0)["w_glob"][k]
    sums = rr.trimmed_sum(np.stack([c[k] for c in clients]), 30)
    m = -(-sums.size // 64) * 64
    pad = lambda a, dt: torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(m - a.size, dt)])).to(cuda)  # noqa: E731
    v = torch.zeros(m, dtype=torch.float64, device=cuda)
    out64, v_out = torch.empty_like(v), torch.empty_like(v)
    ops.reduce_stack(pad(sums, np.float32).view(1, m), torch.ones(1, dtype=torch.float32, device=cuda), na.MODE_W32_DIV64,
                     float(N - 60), out64=out64, op=opt.op, prev=pad(prev, np.float32), v=v, v_out=v_out, beta=opt.beta,
                     eta=opt.eta, tau=opt.tau, beta2=opt.beta2)
    assert rr.same_bits(got, out64.cpu().numpy()[: sums.size].reshape(sums.shape))
    assert rr.same_bits(opt.v_t()[k], v_out.cpu().numpy()[: sums.size].reshape(sums.shape))


def test_poisoned_median_and_refusals(clients, cuda):
    cl = [{"fc3.weight": c["fc3.weight"]} for c in clients]
    for i in range(60):  # 60 of 300: NaN, inf and scaled uploads
        cl[5 * i] = {"fc3.weight": (np.nan, np.inf, cl[5 * i]["fc3.weight"] * np.float32(1e6))[i % 3] + np.zeros((10, 84), np.float32)}
    got = Median(wide=True).server(upload(cl), 0)["w_glob"]["fc3.weight"]
    assert np.isfinite(got).all() and rr.same_bits(got, rr.median(np.stack([c["fc3.weight"] for c in cl])))
    small = upload([{"w": np.full(8, i, np.float32)} for i in range(1025)])
    with pytest.raises(SystemExit):
        Median(wide=True).server(small, 0)
    with pytest.raises(SystemExit):
        Median().server(small[:129], 0)
