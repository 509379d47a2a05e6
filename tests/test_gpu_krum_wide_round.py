"""GPU: Krum / multi-Krum rounds of 200 and 300 clients through the strategies (Krum, MultiKrum with
wide=True -> Aggregator.ensemble_krum -> fa_gram_f32_wide).  A small model with two fp32 tensors (185 and
10 elements: no multiple of 64) and an int64 counter; the honest uploads are a tight cluster around the
global model, upload 0 the tightest, and f planted uploads sit far away.  Every round first asserts on
the float64 reference that the m-th and (m+1)-th scores are at least 1e-3 of the m-th apart, so a
rounding-level difference cannot flip the selection; then the audit must name the reference's selection
and w_glob must be bit-identical to the engine's unit-weight mean over the selected uploads."""
import numpy as np
import pytest

import gram_ref as gr
import robust_ref as rr
from flearn_amd import AVG, Krum, MultiKrum
from flearn_amd.aggregator import Aggregator, ServerOptimizer

pytestmark = pytest.mark.gpu

F = 5
KEYS32 = ("w", "b")


def upload(clients):
    return [{"agg_weight": 0.5, "params": c} for c in clients]  # the weights are not used


def make_round(g, n, seed):
    """n uploads around g: noise of scale 0.1 for upload 0, 0.5 .. 0.8 for the others, and F uploads 100 away."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = np.float32(0.1 if i == 0 else 0.5 + 0.001 * i)
        c = {k: (np.asarray(g[k], np.float32) + s * rng.standard_normal(np.shape(g[k])).astype(np.float32)) for k in KEYS32}
        c["steps"] = np.array(10 * i + 1, np.int64)  # a counter that tells the clients apart
        out.append(c)
    for i in range(F):
        j = 7 + (n // F) * i  # spread over the panels
        out[j] = dict(out[j], **{k: out[j][k] + np.float32(100.0) for k in KEYS32})
    return out


def reference_selection(clients, m, center=None):
    """The m uploads of lowest score (ties to the lower index, upload order) from the exact float64 Gram
    of y = fl32(x - c), after the gap condition on the inputs."""
    x = np.stack([np.concatenate([c[k].reshape(-1) for k in KEYS32]) for c in clients])
    c = None if center is None else np.concatenate([np.asarray(center[k], np.float32).reshape(-1) for k in KEYS32])
    g = gr.gram(x, c)
    d = np.maximum(np.diagonal(g)[:, None] + np.diagonal(g)[None, :] - 2.0 * g, 0.0)
    np.fill_diagonal(d, np.inf)
    sc = np.sort(d, axis=1)[:, : len(clients) - F - 2].sum(axis=1)
    order = np.argsort(sc, kind="stable")
    a, b = sc[order[m - 1]], sc[order[m]]
    assert b - a >= 1e-3 * a, f"the inputs leave the selection ambiguous: scores {a} and {b}"
    return sorted(int(i) for i in order[:m])


def same(got, want, where):
    assert list(got) == list(want), f"{where}: key order"
    for k in want:
        assert rr.same_bits(np.asarray(got[k]), np.asarray(want[k])), f"{where}: {k}"


@pytest.fixture(scope="module")
def g0():
    rng = np.random.default_rng(0)
    return {"w": rng.standard_normal((37, 5)).astype(np.float32), "b": rng.standard_normal(10).astype(np.float32)}


@pytest.mark.parametrize("n", [200, 300])
@pytest.mark.parametrize("make,m_of", [(MultiKrum, lambda n: n - F), (Krum, lambda n: 1)])
def test_wide_rounds_select_the_reference_and_average_it(n, make, m_of, g0, cuda):
    m = m_of(n)
    s = make(F, wide=True)
    centre = None
    g = g0
    for r in range(2):  # round 1 is centred on the strategy's own copy of round 0's w_glob
        cl = make_round(g, n, 10 * n + r)
        sel = reference_selection(cl, m, centre)
        got = s.server(upload(cl), r)["w_glob"]
        audit = s.engine.last_krum
        assert audit["selected"].tolist() == sel and audit["centered"] is (r == 1) and audit["gram"].shape == (n, n)
        assert audit["gram"].tobytes() == np.ascontiguousarray(audit["gram"].T).tobytes()
        same(got, AVG().server([{"agg_weight": 1, "params": cl[i]} for i in sel], 0)["w_glob"], f"{make.__name__} round {r}")
        assert float(got["steps"]) == np.mean([10 * i + 1 for i in sel])
        g = centre = {k: np.asarray(got[k], np.float32) for k in KEYS32}
    assert m > 1 or sel == [0]  # Krum keeps the tightest upload


def test_wide_round_with_a_fused_server_step(g0, cuda):
    n, m = 200, 200 - F
    opt, opt_ref = ServerOptimizer("avgm"), ServerOptimizer("avgm")
    opt.init_global(g0)
    opt_ref.init_global(g0)
    cl = make_round(g0, n, 77)
    sel = reference_selection(cl, m)
    s = MultiKrum(F, server_opt=opt, wide=True)
    got = s.server(upload(cl), 0)["w_glob"]
    assert s.engine.last_krum["selected"].tolist() == sel
    same(got, Aggregator().ensemble([1] * m, [cl[i] for i in sel], server_opt=opt_ref), "fused avgm")
    assert all(rr.same_bits(opt.v_t()[k], opt_ref.v_t()[k]) for k in KEYS32)


def test_a_129_upload_round_without_wide_still_raises(g0, cuda):
    cl = make_round(g0, 129, 3)
    with pytest.raises(ValueError, match="128"):
        Aggregator().ensemble_krum(cl, F, 129 - F)
    with pytest.raises(SystemExit):  # client-data errors take server_exception's route
        MultiKrum(F).server(upload(cl), 0)
