"""GPU: Krum / multi-Krum rounds through the strategies (Krum, MultiKrum -> Aggregator.ensemble_krum).
LeNet5 layout, N = 10, f = 2: eight honest uploads g + s_i * noise with clearly different scales, one
upload of inf, one scaled by 100.  Every test first asserts ON THE CPU, in float64, that the scores'
order is safe against the Gram kernel's derived error bound (the m-th and (m+1)-th scores are further
apart than twice the bound propagated to them), so the selection is unambiguous and a failure is the
kernel's; then the audit record must name krum_ref's selection and w_glob must be bit-identical to
AVG().server on the selected uploads with agg_weight = 1."""
import math

import numpy as np
import pytest
import torch

import gram_ref as gr
import krum_ref as kr
import robust_ref as rr
from flearn_amd import AVG, Krum, MultiKrum, device_state_dicts
from flearn_amd.aggregator import Aggregator, ServerOptimizer
from golden_io import Golden

pytestmark = pytest.mark.gpu

OUTPUTS = ("reference", "float32", "device")
N, F, BAD_INF, BAD_SCALED = 10, 2, 4, 7


def upload(clients, weight=1):
    return [{"agg_weight": weight, "params": c} for c in clients]


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def flat(w, keys, dtype=np.float32):
    return np.concatenate([_host(w[k]).reshape(-1).astype(dtype) for k in keys])


def make_round(g, seed, keys):
    """Ten uploads around the global model g: scales 0.3, 0.4, ... for the honest ones."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N):
        s = np.float32(0.3 + 0.1 * i)
        out.append({k: (_host(g[k]).astype(np.float32) + s * rng.standard_normal(_host(g[k]).shape).astype(np.float32))
                    .astype(np.float32) for k in keys})
    out[BAD_INF] = {k: np.full_like(v, np.inf) for k, v in out[BAD_INF].items()}
    out[BAD_SCALED] = {k: (v * np.float32(100)).astype(np.float32) for k, v in out[BAD_SCALED].items()}
    return out


def reference_selection(clients, keys, f, m, center=None):
    """(selected, scores, gram, tol) from the exact float64 Gram of y = fl32(x - c), after the margin
    precondition.  tol bounds the kernel's error per entry: the Gram is the sum of one launch per run
    of keys, every launch's chain is at most LC + ceil((W + 512) / LC) for the whole width W and its
    grid at most 512, and S adds over the runs."""
    x = np.stack([flat(c, keys) for c in clients])
    c = None if center is None else flat(center, keys)
    finite = [i for i in range(len(clients)) if np.isfinite(x[i]).all()]
    width = x.shape[1]
    y = np.abs(gr.centred(x[finite], c).astype(np.float64))
    tol_f = (gr.gamma(gr.LC + -(-(width + 512) // gr.LC)) + gr.GRID_CAP * 2.0 ** -52) * (y @ y.T)
    n = len(clients)
    gram = np.full((n, n), np.inf)
    tol = np.zeros((n, n))
    gram[np.ix_(finite, finite)] = gr.gram(x[finite], c)
    tol[np.ix_(finite, finite)] = tol_f
    sel, sc = kr.select(gram, f, m)
    # the scores' intervals under the bound: the sum of the k smallest is monotone in every distance
    k = n - f - 2
    lo, hi = np.full(n, np.inf), np.full(n, np.inf)
    for i in finite:
        d = np.array([kr.distance(gram, i, j) for j in range(n) if j != i])
        e = np.array([tol[i, i] + tol[j, j] + 2 * tol[i, j] for j in range(n) if j != i])
        lo[i] = np.sort(np.maximum(d - e, 0.0))[:k].sum()
        hi[i] = np.sort(d + e)[:k].sum()
    order = sorted(range(n), key=lambda i: (sc[i], i))
    a, b = order[m - 1], order[m]
    bound = max(hi[a] - sc[a], sc[a] - lo[a], (hi[b] - sc[b]) if math.isfinite(sc[b]) else 0.0,
                (sc[b] - lo[b]) if math.isfinite(sc[b]) else 0.0)
    assert sc[b] - sc[a] > 2 * bound, f"the inputs leave the selection ambiguous: gap {sc[b] - sc[a]}, bound {bound}"
    assert max(hi[i] for i in order[:m]) < min(lo[i] for i in order[m:])
    return sel, np.array(sc), gram, tol


def same(got, want, where):
    assert list(got) == list(want), f"{where}: key order"
    for k in want:
        g, w = got[k], want[k]
        assert type(g) is type(w), f"{where}: {k} {type(g)} {type(w)}"
        if isinstance(g, torch.Tensor):
            assert g.is_cuda == w.is_cuda and g.dtype == w.dtype, f"{where}: {k}"
        assert rr.same_bits(_host(g), _host(w)), f"{where}: {k}"


def check_audit(engine, sel, sc, gram, tol, centered):
    audit = engine.last_krum
    assert sorted(audit) == ["centered", "gram", "scores", "selected"]
    assert audit["selected"].tolist() == sel and audit["centered"] is centered
    assert isinstance(audit["gram"], np.ndarray) and audit["gram"].dtype == np.float64
    ok = np.isfinite(gram)
    assert (~np.isfinite(audit["gram"][~ok])).all()
    assert (np.abs(audit["gram"][ok] - gram[ok]) <= tol[ok]).all()
    assert audit["gram"].tobytes() == np.ascontiguousarray(audit["gram"].T).tobytes()
    assert np.isinf(audit["scores"][BAD_INF]) and audit["scores"].argmax() == BAD_INF


@pytest.fixture(scope="module")
def lenet():
    return Golden("avg_lenet5_n10").clients()


@pytest.fixture(scope="module")
def keys(lenet):
    return list(lenet[0])


@pytest.fixture(scope="module")
def clients(lenet, keys):
    return make_round(lenet[0], 1, keys)


@pytest.fixture(scope="module")
def refs(clients, keys):
    """krum_ref's selections of the round, uncentred, by m (computed once)."""
    return {m: reference_selection(clients, keys, F, m) for m in (1, 3, N - F)}


@pytest.mark.parametrize("output", OUTPUTS)
def test_krum_and_multikrum_rounds(output, clients, refs, cuda):
    for make, m in ((lambda **k: Krum(F, **k), 1), (lambda **k: MultiKrum(F, **k), N - F), (lambda **k: MultiKrum(F, 3, **k), 3)):
        sel, sc, gram, tol = refs[m]
        assert BAD_INF not in sel and BAD_SCALED not in sel and len(sel) == m
        s = make(output=output)
        got = s.server(upload(clients, 0.5), 0)["w_glob"]  # the weights are not used
        check_audit(s.engine, sel, sc, gram, tol, False)
        want = AVG(output=output).server(upload([clients[i] for i in sel], 1), 0)["w_glob"]
        same(got, want, f"{type(s).__name__} m={m} {output}")
        assert all(np.isfinite(_host(v)).all() for v in got.values())
        assert s.engine.last_plan.groups["f32"].numerics.denom == m
    assert refs[1][0] == [0]  # Krum keeps the upload with the least noise


def test_upload_forms_give_the_same_bits(clients, refs, cuda):
    sel, sc, gram, tol = refs[3]
    for output in ("reference", "device"):
        s = MultiKrum(F, 3, output=output, center=None)
        cpu = [{k: torch.from_numpy(v.copy()) for k, v in c.items()} for c in clients]
        want = AVG(output=output).server(upload([cpu[i] for i in sel], 1), 0)["w_glob"]
        same(s.server(upload(cpu), 0)["w_glob"], want, f"torch cpu {output}")
        dev = [{k: v.to(cuda) for k, v in c.items()} for c in cpu]
        same(s.server(upload(dev), 1)["w_glob"], want, f"device uploads {output}")
        assert s.engine.packer.last_row_tables["f32"] in ("rows", "gather")
        check_audit(s.engine, sel, sc, gram, tol, False)
        slab = device_state_dicts(cpu[0], len(cpu), cuda)
        for d, c in zip(slab, cpu):
            for k, v in c.items():
                d[k].copy_(v)
        same(s.server(upload(slab), 2)["w_glob"], want, f"slab uploads {output}")
        assert s.engine.packer.last_row_tables["f32"] == "slab"
        check_audit(s.engine, sel, sc, gram, tol, False)
        torch.cuda.synchronize()


def test_bn_model_counters_follow_the_selection(cuda):
    """int64 / float64 buffers do not enter the distances and are averaged over the selected clients."""
    bn = Golden("avg_bnmodel_pyint_n4").clients()
    names = list(bn[0])
    f32 = [k for k in names if np.asarray(bn[0][k]).dtype == np.float32]
    rng = np.random.default_rng(5)
    cl = []
    for i in range(7):
        c = {}
        for k in names:
            v = np.asarray(bn[0][k])
            if v.dtype == np.float32:
                c[k] = (v + np.float32(0.3 + 0.2 * i) * rng.standard_normal(v.shape).astype(np.float32)).astype(np.float32)
            else:
                c[k] = (v + v.dtype.type(10 * i + 1)).astype(v.dtype)  # counters that tell the clients apart
        cl.append(c)
    cl[1] = {k: (v * v.dtype.type(100)) if v.dtype == np.float32 else v for k, v in cl[1].items()}
    sel, sc, gram, tol = reference_selection(cl, f32, 2, 3)
    assert len(sel) == 3 and 1 not in sel
    for output in OUTPUTS:
        s = MultiKrum(2, 3, output=output)
        got = s.server(upload(cl), 0)["w_glob"]
        assert s.engine.last_krum["selected"].tolist() == sel
        same(got, AVG(output=output).server(upload([cl[i] for i in sel], 1), 0)["w_glob"], f"bn {output}")
        counter = next(k for k in names if k.endswith("num_batches_tracked"))
        assert float(_host(got[counter])) == np.mean([int(cl[i][counter]) for i in sel])


def test_server_fused_avgm_over_two_rounds(lenet, keys, clients, cuda):
    """MultiKrum with a fused AVGM step against AVGM over the selected sub-lists; round 2 is centred
    on the strategy's own copy of round 1's w_glob."""
    g0 = {k: lenet[0][k] for k in keys}
    opt, opt_ref = ServerOptimizer("avgm"), ServerOptimizer("avgm")
    opt.init_global(g0)
    opt_ref.init_global(g0)
    s, eng = MultiKrum(F, 3, server_opt=opt), Aggregator()
    rounds = [clients]
    center = None
    for r in range(2):
        cl = rounds[r]
        sel, sc, gram, tol = reference_selection(cl, keys, F, 3, center)
        got = s.server(upload(cl), r)["w_glob"]
        check_audit(s.engine, sel, sc, gram, tol, r == 1)
        want = eng.ensemble([1] * 3, [cl[i] for i in sel], server_opt=opt_ref)
        same(got, want, f"fused round {r}")
        assert all(rr.same_bits(opt.v_t()[k], opt_ref.v_t()[k]) for k in keys), r
        center = {k: np.asarray(got[k]).astype(np.float32) for k in keys}  # what the strategy subtracts next
        rounds.append(make_round(got, 20 + r, keys))
    assert any(np.abs(opt.v_t()[k]).max() > 0 for k in keys)


def test_centred_rounds_and_the_strategys_own_copy(lenet, keys, cuda):
    s = MultiKrum(F, 3)
    cl = make_round(lenet[0], 3, keys)
    first = s.server(upload(cl), 0)["w_glob"]
    assert s.engine.last_krum["centered"] is False
    kept = {k: np.array(v) for k, v in first.items()}
    for v in first.values():  # the caller scribbles over what it was handed
        v[...] = np.nan
    cl2 = make_round(kept, 4, keys)
    centre = {k: kept[k].astype(np.float32) for k in keys}
    sel, sc, gram, tol = reference_selection(cl2, keys, F, 3, centre)
    got = s.server(upload(cl2), 1)["w_glob"]
    check_audit(s.engine, sel, sc, gram, tol, True)
    same(got, AVG().server(upload([cl2[i] for i in sel], 1), 0)["w_glob"], "centred round")
    # centred Grams are far more accurate: the bound is a small fraction of the smallest distance
    assert tol[np.ix_(sel, sel)].max() < 1e-3 * sc[sel].min()
    never = MultiKrum(F, 3, center=None)
    never.server(upload(cl), 0)
    never.server(upload(cl2), 1)
    assert never.engine.last_krum["centered"] is False and never.engine.last_krum["selected"].tolist() == sel


def test_another_upload_order_selects_the_same_set(clients, refs, cuda):
    sel = refs[3][0]
    rng = np.random.default_rng(0)
    s = MultiKrum(F, 3, center=None)
    for _ in range(3):
        perm = rng.permutation(N)
        got = s.server(upload([clients[i] for i in perm]), 0)["w_glob"]
        picked = sorted(int(perm[j]) for j in s.engine.last_krum["selected"])
        assert picked == sel, perm
        order = [int(perm[j]) for j in s.engine.last_krum["selected"]]  # the mean is taken in upload order
        same(got, AVG().server(upload([clients[i] for i in order], 1), 0)["w_glob"], f"perm {perm}")


def test_more_than_f_bad_uploads_exit_and_the_engine_stays_usable(clients, refs, cuda):
    cl = [dict(c) for c in clients]
    for i in (0, 1):
        cl[i] = {k: np.full_like(v, np.nan) for k, v in cl[i].items()}  # three non-finite uploads, f = 2
    s = MultiKrum(F, center=None)
    with pytest.raises(SystemExit):
        s.server(upload(cl), 0)
    assert s._prev_glob is None
    sel = refs[N - F][0]
    same(s.server(upload(clients), 1)["w_glob"], AVG().server(upload([clients[i] for i in sel], 1), 0)["w_glob"], "after")
    with pytest.raises(SystemExit):  # N < 2 f + 3
        Krum(4).server(upload(clients), 0)
    with pytest.raises(SystemExit):
        Krum(F, devices=[cuda, cuda]).server(upload(clients), 0)


def same_values(got, want, where):
    """As `same`, whatever the two dicts' key orders."""
    assert sorted(got) == sorted(want), f"{where}: keys"
    same({k: got[k] for k in want}, want, where)


def test_a_left_out_upload_cannot_move_columns_by_reordering_its_dict(clients, keys, cuda):
    """Upload 0 sets the round's key order.  Here it is the scaled upload, it lists its keys in reverse,
    and it is left out: the selected uploads' mean must still be read from their own keys' columns."""
    cl = list(clients)
    cl[0], cl[BAD_SCALED] = cl[BAD_SCALED], cl[0]
    cl[0] = {k: cl[0][k] for k in reversed(keys)}
    sel, sc, gram, tol = reference_selection(cl, keys, F, 3)
    assert 0 not in sel and BAD_INF not in sel
    for output in ("reference", "device"):
        s = MultiKrum(F, 3, output=output, center=None)
        for form in ("host", "device"):
            ups = cl if form == "host" else [{k: torch.from_numpy(v.copy()).to(cuda) for k, v in c.items()} for c in cl]
            got = s.server(upload(ups), 0)["w_glob"]
            assert s.engine.last_krum["selected"].tolist() == sel
            assert list(got) == list(reversed(keys))  # the round's key order
            want = AVG(output=output).server(upload([ups[i] for i in sel], 1), 0)["w_glob"]
            same_values(got, want, f"reordered upload 0, {form} uploads, {output}")
            torch.cuda.synchronize()


def test_a_key_missing_from_a_left_out_upload_leaves_the_rounds_keys(clients, keys, cuda):
    """The round aggregates the keys common to ALL uploads, whoever is selected: a key that only a
    left-out upload lacks stays out, and nothing raises."""
    cl = list(clients)
    cl[BAD_INF] = {k: v for k, v in cl[BAD_INF].items() if k != keys[-1]}
    common = keys[:-1]
    sel, sc, gram, tol = reference_selection(cl, common, F, 3)
    assert BAD_INF not in sel
    s = MultiKrum(F, 3, center=None)
    got = s.server(upload(cl), 0)["w_glob"]
    check_audit(s.engine, sel, sc, gram, tol, False)
    assert list(got) == common
    same(got, Aggregator().ensemble([1] * 3, [cl[i] for i in sel], common), "missing key")
