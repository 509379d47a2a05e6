"""GPU: norm-clipped rounds through the strategy (NormClip -> Aggregator.ensemble_clipped).

Expected-value protocol, so that no case depends on which side of tau a norm falls within rounding:
the device's norms (engine.last_clip["norm2"]) are (1) held to the float64 reference within the
derived bound of the norm kernel, (2) fed to clip.clip_radius / clip_scales for the expected scales,
which clip_ref turns into (3) the expected clipped uploads; w_glob must then equal, bit for bit, the
unit-weight mean of those uploads — clip_ref's own fl64(acc) / N, and the engine's plain
ensemble([1] * N, clipped uploads) in every output mode."""
import math

import numpy as np
import pytest
import torch

import clip_ref as cr
import robust_ref as rr
from flearn_amd import AVG, NormClip, clip, device_state_dicts
from flearn_amd.aggregator import Aggregator, ServerOptimizer
from flearn_amd.bucketplan import key_runs
from golden_io import Golden

pytestmark = pytest.mark.gpu

OUTPUTS = ("reference", "float32", "device")
N = 10


def upload(clients, weight=1):
    return [{"agg_weight": weight, "params": c} for c in clients]


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def f32_keys(w):
    return [k for k in w if _host(w[k]).dtype == np.float32]


def make_round(g, seed, keys, n=N):
    """n uploads around g: update norms growing with the client index."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = np.float32(0.02 * (1 + i))
        out.append({k: (_host(g[k]).astype(np.float32) + s * rng.standard_normal(_host(g[k]).shape).astype(np.float32))
                    .astype(np.float32) for k in keys})
    return out


def same(got, want, where):
    assert list(got) == list(want), f"{where}: key order"
    for k in want:
        g, w = got[k], want[k]
        assert type(g) is type(w), f"{where}: {k} {type(g)} {type(w)}"
        if isinstance(g, torch.Tensor):
            assert g.is_cuda == w.is_cuda and g.dtype == w.dtype, f"{where}: {k}"
        assert rr.same_bits(_host(g), _host(w)), f"{where}: {k}"


def expected(engine, clients, centre, tau=None, quantile=None):
    """Steps (1)-(3) of the protocol: (scales, the clipped uploads as host dicts)."""
    audit = engine.last_clip
    assert sorted(audit) == ["centered", "clipped", "norm2", "replaced", "scale", "tau"] and audit["centered"] is True
    keys = f32_keys(clients[0])
    n = len(clients)
    g = {k: _host(centre[k]).astype(np.float32).reshape(-1) for k in keys}
    x = {k: np.stack([_host(c[k]).astype(np.float32).reshape(-1) for c in clients]) for k in keys}
    ref = sum(cr.norm2(x[k], g[k]) for k in keys)
    got = audit["norm2"]
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n,)
    # (1) one launch per run of keys on the natural grid, the runs added in float64: all terms are
    # non-negative, so the worst run's relative bound holds for the sum
    cus = torch.cuda.get_device_properties(engine.device).multi_processor_count
    runs = key_runs(engine.last_plan.groups["f32"])
    bound = max(cr.norm_bound(cr.launch_plan(n, c1 - c0, cus)) for c0, c1 in runs) + len(runs) * 2.0 ** -52
    finite = np.isfinite(ref)
    assert (np.isfinite(got) == finite).all()
    assert (np.abs(got[finite] - ref[finite]) <= bound * ref[finite]).all(), (got, ref, bound)
    # (2)
    radius = clip.clip_radius(got, tau, quantile)
    scale = clip.clip_scales(got, radius)
    assert audit["tau"] == radius == cr.radius(got, tau, quantile)
    assert audit["scale"].dtype == np.float32 and audit["scale"].tobytes() == scale.tobytes() == cr.scales(got, radius).tobytes()
    assert audit["clipped"].tolist() == [i for i in range(n) if scale[i] < 1]
    assert audit["replaced"].tolist() == [i for i in range(n) if scale[i] == 0]
    # (3)
    out = []
    for i, c in enumerate(clients):
        out.append({k: (cr.clipped_upload(x[k][i], g[k], scale[i]).reshape(_host(v).shape) if k in x else _host(v))
                    for k, v in c.items()})
    return scale, out, {k: cr.clipped_mean(x[k], g[k], scale).reshape(_host(clients[0][k]).shape) for k in keys}


@pytest.fixture(scope="module")
def lenet():
    return Golden("avg_lenet5_n10").clients()


@pytest.fixture(scope="module")
def keys(lenet):
    return list(lenet[0])


@pytest.fixture(scope="module")
def g0(lenet, keys):
    return {k: _host(lenet[0][k]).astype(np.float32) for k in keys}


@pytest.fixture(scope="module")
def clients(g0, keys):
    return make_round(g0, 1, keys)


def norms_of(clients, g0, keys):
    return np.sqrt(sum(cr.norm2(np.stack([c[k].reshape(-1) for c in clients]), g0[k].reshape(-1)) for k in keys))


@pytest.mark.parametrize("output", OUTPUTS)
def test_fixed_and_quantile_radii(output, clients, g0, keys, cuda):
    norms = norms_of(clients, g0, keys)
    mid = float(0.5 * (norms[4] + norms[5]))
    cases = [({"tau": mid}, 5), ({"tau": float(norms.max() * 2)}, 0), ({"tau": float(norms.min() / 2)}, N),
             ({"quantile": 0.5}, 5), ({"quantile": 1.0}, 0)]
    for kw, n_clipped in cases:
        s = NormClip(output=output, **kw)
        s.init_global(g0)
        got = s.server(upload(clients, 0.5), 0)["w_glob"]  # the weights are not used
        scale, yhat, mean = expected(s.engine, clients, g0, kw.get("tau"), kw.get("quantile"))
        assert int((scale < 1).sum()) == n_clipped and (scale > 0).all(), kw
        same(got, AVG(output=output).server(upload(yhat, 1), 0)["w_glob"], f"{kw} {output}")
        if output == "reference":
            for k in keys:
                assert rr.same_bits(_host(got[k]), mean[k]), k
        assert s.engine.last_plan.groups["f32"].numerics.denom == N


def test_poisoned_uploads_are_replaced_or_clipped(clients, g0, keys, cuda):
    """Three bad uploads among ten: NaN, inf and one scaled by 1e6.  Every element stays finite and
    ||w - g||_2 <= tau + allowance.  The allowance, with u = 2^-24: a kept upload has device norm
    <= tau, true norm <= tau * (1 + bound) (the norm kernel's derived bound); a clipped one is
    s * d with s = fl32(tau / norm) <= (tau / norm) * (1 + u) and a true norm within the same bound: so
    every exact clipped update has norm <= tau * (1 + bound + 2 u).  An element of w then lies behind
    N + 3 roundings (x - g, s * d, g + ., the N - 1 adds of the sum; the float64 divide is below u^2),
    each at most u times a magnitude of at most |g_k| + tau_k', where |yhat_ik - g_k| <= tau': as a
    vector over the P elements that is (N + 3) * u * (||g||_2 + tau' * sqrt(P))."""
    cl = [dict(c) for c in clients]
    cl[2] = {k: np.full_like(v, np.nan) for k, v in cl[2].items()}
    cl[5] = {k: np.full_like(v, np.inf) for k, v in cl[5].items()}
    cl[8] = {k: (g0[k] + np.float32(1e6) * (v - g0[k])).astype(np.float32) for k, v in cl[8].items()}
    norms = norms_of(clients, g0, keys)
    tau = float(0.5 * (norms[6] + norms[7]))
    s = NormClip(tau=tau)
    s.init_global(g0)
    got = s.server(upload(cl), 0)["w_glob"]
    scale, yhat, mean = expected(s.engine, cl, g0, tau)
    assert s.engine.last_clip["replaced"].tolist() == [2, 5]
    assert s.engine.last_clip["clipped"].tolist() == [2, 5, 7, 8, 9]
    assert all(np.isfinite(_host(v)).all() for v in got.values())
    for k in keys:
        assert rr.same_bits(_host(got[k]), mean[k]), k
    p = sum(g0[k].size for k in keys)
    gnorm = math.sqrt(sum(float((g0[k].astype(np.float64) ** 2).sum()) for k in keys))
    dist = math.sqrt(sum(float(((_host(got[k]) - g0[k].astype(np.float64)) ** 2).sum()) for k in keys))
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    bound = max(cr.norm_bound(cr.launch_plan(N, c1 - c0, cus)) for c0, c1 in key_runs(s.engine.last_plan.groups["f32"]))
    tau1 = tau * (1 + bound + 2 * cr.U)
    allowance = (tau1 - tau) + (N + 3) * cr.U * (gnorm + tau1 * math.sqrt(p))
    print(f"poisoned round: ||w - g|| = {dist:.6g}, tau = {tau:.6g}, allowance = {allowance:.3g}")
    assert dist <= tau + allowance
    # FedAVG's mean of the same uploads is poisoned
    assert not all(np.isfinite(_host(v)).all() for v in AVG().server(upload(cl), 0)["w_glob"].values())


def test_an_infinite_radius_is_the_unit_weight_mean(clients, g0, cuda):
    for output in OUTPUTS:
        s = NormClip(tau=math.inf, output=output)
        s.init_global(g0)
        got = s.server(upload(clients), 0)["w_glob"]
        assert s.engine.last_clip["clipped"].size == 0 and (s.engine.last_clip["scale"] == 1).all()
        same(got, Aggregator(output=output).ensemble([1] * N, clients), f"tau = inf {output}")


def test_centre_handling(clients, g0, keys, cuda):
    s = NormClip(tau=1e-3)
    first = s.server(upload(clients), 0)["w_glob"]  # no init_global: the undefended unit-weight mean
    assert s.engine.last_clip["centered"] is False and s.engine.last_clip["clipped"].size == 0
    same(first, Aggregator().ensemble([1] * N, clients), "first round")
    kept = {k: np.array(v) for k, v in first.items()}
    for v in first.values():  # the caller scribbles over what it was handed
        v[...] = np.nan
    # round 2 is centred on the strategy's own copy of round 1's float64 w_glob, as fl32
    centre = {k: kept[k].astype(np.float32) for k in keys}
    cl2 = make_round(centre, 4, keys)
    got = s.server(upload(cl2), 1)["w_glob"]
    scale, yhat, mean = expected(s.engine, cl2, centre, 1e-3)
    assert (scale < 1).all() and (scale > 0).all()
    for k in keys:
        assert rr.same_bits(_host(got[k]), mean[k]), k
    t = NormClip(tau=1e-3)
    t.init_global(g0)
    t.server(upload(clients), 0)
    assert t.engine.last_clip["centered"] is True and t.engine.last_clip["clipped"].size == N  # the first round clips


def test_weights_and_order_do_not_matter(clients, g0, cuda):
    norms = norms_of(clients, g0, list(g0))
    tau = float(0.5 * (norms[4] + norms[5]))
    s = NormClip(tau=tau)
    s.init_global(g0)
    a = s.server(upload(clients, 1), 0)["w_glob"]
    base = s.engine.last_clip["norm2"].copy()
    s.init_global(g0)
    b = s.server([{"agg_weight": float(i * i), "params": c} for i, c in enumerate(clients)], 0)["w_glob"]
    same(a, b, "agg_weight")
    rng = np.random.default_rng(0)
    for _ in range(2):
        perm = rng.permutation(N)
        s.init_global(g0)
        s.server(upload([clients[i] for i in perm]), 0)
        assert s.engine.last_clip["norm2"].tobytes() == base[perm].tobytes()  # a client's norm is its own


def test_upload_forms_and_outputs_agree(clients, g0, keys, cuda):
    norms = norms_of(clients, g0, keys)
    tau = float(0.5 * (norms[2] + norms[3]))
    for output in OUTPUTS:
        s = NormClip(tau=tau, output=output)
        s.init_global(g0)
        s.server(upload(clients), 0)
        scale, yhat, _ = expected(s.engine, clients, g0, tau)
        want = AVG(output=output).server(upload(yhat, 1), 0)["w_glob"]
        cpu = [{k: torch.from_numpy(v.copy()) for k, v in c.items()} for c in clients]
        want_t = AVG(output=output).server(upload([{k: torch.from_numpy(v.copy()) for k, v in c.items()} for c in yhat], 1),
                                           0)["w_glob"]
        dev = [{k: v.to(cuda) for k, v in c.items()} for c in cpu]
        slab = device_state_dicts(cpu[0], len(cpu), cuda)
        for d, c in zip(slab, cpu):
            for k, v in c.items():
                d[k].copy_(v)
        for form, ups in (("torch cpu", cpu), ("device", dev), ("slab", slab)):
            s.init_global(g0)
            same(s.server(upload(ups), 0)["w_glob"], want_t, f"{form} {output}")
            assert s.engine.last_clip["scale"].tobytes() == scale.tobytes()
        assert s.engine.packer.last_row_tables["f32"] == "slab"
        s.init_global(g0)
        same(s.server(upload(clients), 0)["w_glob"], want, f"host {output}")
        torch.cuda.synchronize()


def test_bn_model_counters_are_averaged_over_all_clients(cuda):
    bn = Golden("avg_bnmodel_pyint_n4").clients()
    names = list(bn[0])
    rng = np.random.default_rng(5)
    base = {k: _host(bn[0][k]) for k in names}
    cl = []
    for i in range(7):
        c = {}
        for k in names:
            v = base[k]
            if v.dtype == np.float32:
                c[k] = (v + np.float32(0.05 * (i + 1)) * rng.standard_normal(v.shape).astype(np.float32)).astype(np.float32)
            else:
                c[k] = (v + v.dtype.type(10 * i + 1)).astype(v.dtype)  # counters that tell the clients apart
        cl.append(c)
    for output in OUTPUTS:
        s = NormClip(quantile=0.5, output=output)
        s.init_global(base)
        got = s.server(upload(cl), 0)["w_glob"]
        scale, yhat, _ = expected(s.engine, cl, base, None, 0.5)
        assert int((scale < 1).sum()) == 3
        same(got, AVG(output=output).server(upload(yhat, 1), 0)["w_glob"], f"bn {output}")
        counter = next(k for k in names if k.endswith("num_batches_tracked"))
        assert float(_host(got[counter])) == np.mean([int(c[counter]) for c in cl])


@pytest.mark.parametrize("op", ["avgm", "adam"])
def test_server_optimiser_over_three_rounds(op, g0, keys, cuda):
    opt, opt_ref = ServerOptimizer(op), ServerOptimizer(op)
    opt.init_global(g0)
    opt_ref.init_global(g0)
    s, eng = NormClip(quantile=0.6, server_opt=opt), Aggregator()
    s.init_global(g0)
    centre = g0
    for r in range(3):
        cl = make_round(centre, 30 + r, keys)
        got = s.server(upload(cl), r)["w_glob"]
        scale, yhat, _ = expected(s.engine, cl, centre, None, 0.6)
        assert int((scale < 1).sum()) == 4
        same(got, eng.ensemble([1] * N, yhat, server_opt=opt_ref), f"{op} round {r}")
        assert all(rr.same_bits(opt.v_t()[k], opt_ref.v_t()[k]) for k in keys), r
        centre = {k: np.asarray(got[k]).astype(np.float32) for k in keys}  # what the strategy subtracts next
    assert any(np.abs(opt.v_t()[k]).max() > 0 for k in keys)


def test_refusals_take_server_exceptions_route(clients, g0, cuda):
    def strat(**kw):
        s = NormClip(tau=1.0, **kw)
        s.init_global(g0)
        return s

    from flearn_amd.serverstate import DynState

    half = [{k: v.astype(np.float16) for k, v in c.items()} for c in clients]
    doubles = [{k: v.astype(np.float64) for k, v in c.items()} for c in clients]
    extra = [dict(c, other=np.zeros(3, np.float32)) for c in clients]
    many = [clients[i % N] for i in range(129)]
    for s, ups in ((strat(), half), (strat(), doubles), (strat(), extra), (strat(), many),
                   (strat(server_opt=DynState(None)), clients), (strat(devices=[cuda, cuda]), clients),
                   (strat(chunk_clients=4), clients)):
        with pytest.raises(SystemExit):
            s.server(upload(ups), 0)
    with pytest.raises(ValueError, match="begin_round"):
        strat().begin_round(0)
    with pytest.raises(ValueError, match="group"):
        eng = Aggregator()
        eng._dist = True
        eng.ensemble_clipped(clients, 1.0, None, center=g0)
    ok = NormClip(tau=math.inf)
    ok.init_global(g0)
    with pytest.raises(SystemExit):
        ok.server(upload(half), 0)
    same(ok.server(upload(clients), 1)["w_glob"], Aggregator().ensemble([1] * N, clients), "the engine stays usable")
