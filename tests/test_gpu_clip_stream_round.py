"""GPU: streamed norm-clipped and DP-FedAvg rounds (StreamedNormClip -> Aggregator.ensemble_clipped_chunked /
begin_clipped_round -> ops.clip_fold_stack).

Where NormClip takes the round (N <= 128) the streamed round must equal it bit for bit, audit
included, whatever the chunk size.  Beyond 128 clients there is no one-launch round to compare with:
the device's norms are held to the float64 reference within the norm kernel's derived bound
(clip_ref.norm_bound, as tests/test_gpu_clip_round.py does), the scales follow from them
(clip.clip_scales), and the result must equal clip_ref's clipped mean of the uploads under those
scales, bit for bit, for every chunk size."""
import types

import numpy as np
import pytest
import torch

import clip_ref as cr
import robust_ref as rr
from flearn_amd import AVG, NormClip, StreamedNormClip, clip, device_state_dicts, layouts, ops
from flearn_amd.aggregator import ServerOptimizer
from flearn_amd.bucketplan import key_runs
from flearn_amd.wire import Encrypt
from test_gpu_clip_round import OUTPUTS, _host, same, upload
from test_gpu_dp_round import noised_reference

pytestmark = pytest.mark.gpu

LENET = layouts.get("lenet5")
BN = [("conv.weight", (8, 3, 3, 3), "f32")] + layouts._bn("bn", 8) + [("fc.weight", (10, 8), "f32"), ("fc.bias", (10,), "f32")]
N, BIG = 23, 300
KS = (1, 5, 16, 23, 64)
AUDIT = ["centered", "chunks", "clipped", "norm2", "replaced", "scale", "tau"]
NOISE = ["noise_multiplier", "seed", "sequence", "sigma"]


def model(layout, rng, scale=1.0, counter=0):
    flat = (scale * rng.standard_normal(layouts.fp32_elems(layout))).astype(np.float32)
    return layouts.synthetic_state_dict(layout, flat, counter)


def round_of(layout, g, n, seed, distinct=None):
    """n uploads around g with update norms that all differ: client i is base[i % distinct] plus a
    per-client offset (distinct None: n independent updates, norms growing with the index)."""
    rng = np.random.default_rng(seed)
    f32 = [k for k, _, t in layout if t == "f32"]
    base = [model(layout, rng) for _ in range(distinct or n)]
    out = []
    for i in range(n):
        b = base[i % len(base)]
        s = np.float32(0.02 * (1 + i % len(base)))
        c = {k: (g[k] + s * b[k] + np.float32(1e-4 * (i // len(base)))).astype(np.float32) for k in f32}
        c.update({k: np.array(10 * i + 1, np.int64).reshape(g[k].shape) for k in g if k not in c})
        out.append({k: c[k] for k in g})
    return out


def norms_of(clients, g):
    keys = [k for k in g if g[k].dtype == np.float32]
    return np.sqrt(sum(cr.norm2(np.stack([c[k].reshape(-1) for c in clients]), g[k].reshape(-1)) for k in keys))


def poisoned(clients, g):
    """NaN, inf and x 1e6 uploads, which chunks of 5 and of 16 put in different chunks."""
    cl = [dict(c) for c in clients]
    f32 = [k for k in g if g[k].dtype == np.float32]
    cl[2].update({k: np.full_like(cl[2][k], np.nan) for k in f32})
    cl[9].update({k: np.full_like(cl[9][k], np.inf) for k in f32})
    cl[19].update({k: (g[k] + np.float32(1e6) * (cl[19][k] - g[k])).astype(np.float32) for k in f32})
    return cl


def audits_equal(a, b, where):
    for k in ("norm2", "scale", "clipped", "replaced"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (where, k)  # (a NaN norm included)
    assert a["tau"] == b["tau"] and a["centered"] is b["centered"], where


@pytest.fixture(scope="module")
def g0():
    return model(LENET, np.random.default_rng(1))


@pytest.fixture(scope="module")
def clients(g0):
    return poisoned(round_of(LENET, g0, N, 2), g0)


@pytest.fixture(scope="module")
def tau(g0):
    norms = norms_of(round_of(LENET, g0, N, 2), g0)
    return float(0.5 * (norms[11] + norms[12]))


def forms_of(clients, cuda):
    cpu = [{k: torch.from_numpy(v.copy()) for k, v in c.items()} for c in clients]
    slab = device_state_dicts(cpu[0], len(cpu), cuda)
    for d, c in zip(slab, cpu):
        for k, v in c.items():
            d[k].copy_(v)
    return {"numpy": clients, "torch cpu": cpu, "slab": slab}


# -- N <= 128: NormClip's round, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("output", OUTPUTS)
def test_equals_normclip_for_every_chunk_size(output, clients, g0, tau, cuda):
    for form, ups in forms_of(clients, cuda).items():
        ref = NormClip(tau=tau, output=output)
        ref.init_global(g0)
        want = ref.server(upload(ups), 0)["w_glob"]
        audit = ref.engine.last_clip
        assert audit["replaced"].tolist() == [2, 9] and 19 in audit["clipped"].tolist()
        for k in KS:
            s = StreamedNormClip(tau, output=output, chunk_clients=k)
            s.init_global(g0)
            got = s.server(upload(ups, 0.5), 0)["w_glob"]  # the weights are not used
            same(got, want, f"{form} K={k} {output}")
            mine = s.engine.last_clip
            assert sorted(mine) == AUDIT and mine["chunks"] == -(-N // min(k, N))
            audits_equal(mine, audit, f"{form} K={k}")
        if form == "slab":
            assert s.engine._chunk_packers[0].last_row_tables["f32"] == "slab"
        torch.cuda.synchronize()


def test_bn_model_equals_normclip(cuda):
    rng = np.random.default_rng(7)
    g = model(BN, rng)
    cl = round_of(BN, g, N, 8)
    tau = float(np.median(norms_of(cl, g)))
    counter = next(k for k in g if k.endswith("num_batches_tracked"))
    for output in OUTPUTS:
        ref = NormClip(tau=tau, output=output)
        ref.init_global(g)
        want = ref.server(upload(cl), 0)["w_glob"]
        for k in (4, 23):
            s = StreamedNormClip(tau, output=output, chunk_clients=k)
            s.init_global(g)
            got = s.server(upload(cl), 0)["w_glob"]
            same(got, want, f"bn K={k} {output}")
            audits_equal(s.engine.last_clip, ref.engine.last_clip, f"bn K={k}")
            assert float(_host(got[counter])) == np.mean([int(c[counter]) for c in cl])


# -- N > 128 -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(cuda):
    """300 BN-model uploads through K = 7 and K = 128: (g, uploads, tau, {K: (w_glob, audit, plan)})."""
    g = model(BN, np.random.default_rng(11))
    cl = round_of(BN, g, BIG, 12, distinct=12)
    f32 = [k for k in g if g[k].dtype == np.float32]
    cl[40].update({k: np.full_like(cl[40][k], np.nan) for k in f32})
    cl[200].update({k: (g[k] + np.float32(1e6) * (cl[200][k] - g[k])).astype(np.float32) for k in f32})
    tau = float(np.median(norms_of(round_of(BN, g, BIG, 12, distinct=12), g)))
    runs = {}
    for k in (7, 128):
        s = StreamedNormClip(tau, chunk_clients=k)
        s.init_global(g)
        runs[k] = (s.server(upload(cl), 0)["w_glob"], s.engine.last_clip, s.engine.last_plan, s.engine.device)
    return g, cl, tau, runs


def test_300_clients_chunk_sizes_agree(big):
    g, cl, tau, runs = big
    (a, audit_a, _, _), (b, audit_b, _, _) = runs[7], runs[128]
    same(a, b, "K = 7 against K = 128")
    audits_equal(audit_a, audit_b, "K = 7 against K = 128")
    assert (audit_a["chunks"], audit_b["chunks"]) == (43, 3)


def test_300_clients_against_the_reference(big):
    g, cl, tau, runs = big
    got, audit, plan, device = runs[7]
    f32 = [k for k in g if g[k].dtype == np.float32]
    x = {k: np.stack([c[k].reshape(-1) for c in cl]) for k in f32}
    ref = sum(cr.norm2(x[k], g[k].reshape(-1)) for k in f32)
    norm2 = audit["norm2"]
    assert norm2.dtype == np.float64 and norm2.shape == (BIG,)
    # one launch per chunk and run of keys on the natural grid, the runs added in float64: the worst
    # launch's relative bound holds for the sum of non-negative terms
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    runs_ = key_runs(plan.groups["f32"])
    bound = max(cr.norm_bound(cr.launch_plan(n, c1 - c0, cus)) for c0, c1 in runs_ for n in (7, BIG % 7)) + len(runs_) * 2.0 ** -52
    finite = np.isfinite(ref)
    assert (np.isfinite(norm2) == finite).all() and not finite[40]
    assert (np.abs(norm2[finite] - ref[finite]) <= bound * ref[finite]).all()
    scale = clip.clip_scales(norm2, tau)
    assert audit["scale"].tobytes() == scale.tobytes() == cr.scales(norm2, tau).tobytes()
    assert audit["replaced"].tolist() == [40] and 200 in audit["clipped"].tolist()
    assert 100 < (scale < 1).sum() < 200  # tau is the median norm: both branches carry real weight
    for k in f32:
        assert rr.same_bits(_host(got[k]), cr.clipped_mean(x[k], g[k].reshape(-1), scale).reshape(g[k].shape)), k
    counter = next(k for k in g if k.endswith("num_batches_tracked"))
    assert float(_host(got[counter])) == np.mean([int(c[counter]) for c in cl])  # over all 300
    assert all(np.isfinite(_host(v)).all() for v in got.values())


# -- uploads as they arrive ----------------------------------------------------------------------------
def test_begin_round_equals_server(clients, g0, tau, cuda):
    for k in (5, 16):
        ref = StreamedNormClip(tau, chunk_clients=k)
        ref.init_global(g0)
        want = ref.server(upload(clients), 0)
        s = StreamedNormClip(tau, chunk_clients=k)
        s.init_global(g0)
        rnd = s.begin_round(0)
        for u in upload(clients):
            rnd.add(u)
        got = rnd.finish()
        assert list(got) == list(want) == ["w_glob"]
        same(got["w_glob"], want["w_glob"], f"begin_round K={k}")
        audits_equal(s.engine.last_clip, ref.engine.last_clip, f"begin_round K={k}")
        same(s._prev_glob, ref._prev_glob, "the next round's centre")


def test_begin_round_takes_encoded_uploads_and_hides_params(clients, g0, tau, cuda):
    enc = Encrypt()
    seen = []

    class Spy(StreamedNormClip):
        def server_post_processing(self, ensemble_params_lst, ensemble_params, **kwargs):
            seen.append(ensemble_params_lst)
            return ensemble_params

    s = Spy(tau, encrypt=enc, chunk_clients=5)
    s.init_global(g0)
    rnd = s.begin_round(0)
    for u in upload(clients, 2.0):
        rnd.add(enc.encode(u))
    got = rnd.finish()["w_glob"]
    ref = StreamedNormClip(tau, chunk_clients=5)
    ref.init_global(g0)
    want = ref.server(upload(clients), 0)["w_glob"]
    for k in want:
        assert rr.same_bits(_host(got[k]), _host(want[k])), k
    (uploads_seen,) = seen  # the uploads without their params
    assert len(uploads_seen) == N and all("params" not in u and u["agg_weight"] == 2.0 for u in uploads_seen)


def test_bad_later_uploads_take_server_exceptions_route(clients, g0, tau, cuda):
    first = next(iter(g0))
    for bad in ({k: v for k, v in clients[7].items() if k != first},
                dict(clients[7], **{first: np.zeros((2, 2), np.float32)})):
        s = StreamedNormClip(tau, chunk_clients=5)
        s.init_global(g0)
        rnd = s.begin_round(0)
        for u in upload(clients[:7]):
            rnd.add(u)
        with pytest.raises(SystemExit):
            rnd.add({"agg_weight": 1, "params": bad})
        if first in bad:  # (a key one upload lacks leaves the whole list's key intersection, as in the reference)
            with pytest.raises(SystemExit):
                t = StreamedNormClip(tau, chunk_clients=5)
                t.init_global(g0)
                t.server(upload(clients[:7] + [bad]), 0)
    ok = StreamedNormClip(tau, chunk_clients=5)  # the device stays usable
    ok.init_global(g0)
    ok.server(upload(clients), 0)


# -- DP-FedAvg -------------------------------------------------------------------------------------------
def test_dp_round_equals_normclip(clients, g0, tau, cuda):
    ref = NormClip(tau=tau, noise_multiplier=1.1, seed=5)
    ref.init_global(g0)
    want = ref.server(upload(clients), 0)["w_glob"]
    for k in (5, 64):
        s = StreamedNormClip(tau, chunk_clients=k, noise_multiplier=1.1, seed=5)
        s.init_global(g0)
        same(s.server(upload(clients), 0)["w_glob"], want, f"DP K={k}")
        mine = s.engine.last_clip
        assert sorted(mine) == sorted(AUDIT + NOISE) and s.sequence == ref.sequence == 1
        assert [mine[n] for n in NOISE] == [ref.engine.last_clip[n] for n in NOISE] == [1.1, 5, 0, float(np.float32(1.1 * tau))]
    # begin_round advances the sequence at finish(); the same (seed, sequence) repeats the bits
    rnd = s.begin_round(1)
    for u in upload(clients):
        rnd.add(u)
    assert s.sequence == 1
    second = rnd.finish()["w_glob"]
    assert s.sequence == 2 and s.engine.last_clip["sequence"] == 1
    t = StreamedNormClip(tau, chunk_clients=7, noise_multiplier=1.1, seed=5, sequence=1)
    t._prev_glob = ref._copy(want)
    same(t.server(upload(clients), 1)["w_glob"], second, "the same (seed, sequence)")
    assert any(not rr.same_bits(_host(second[k]), _host(want[k])) for k in want)


def test_dp_round_of_300_clients(big):
    g, cl, tau, runs = big
    plain, _, _, _ = runs[7]
    s = StreamedNormClip(tau, chunk_clients=7, noise_multiplier=1.1, seed=5, sequence=3)
    s.init_global(g)
    got = s.server(upload(cl), 0)["w_glob"]
    audit = s.engine.last_clip
    shim = types.SimpleNamespace(last_clip={k: v for k, v in audit.items() if k != "chunks"}, last_plan=s.engine.last_plan)
    _, ref = noised_reference(shim, cl, g, tau, 1.1, 5, 3)
    keys = list(ref)
    moved = np.concatenate([(_host(got[k]) - _host(plain[k])).reshape(-1) for k in keys])
    noise = np.concatenate([ref[k][2].reshape(-1) for k in keys])
    worst = float(np.abs(moved - noise).max())
    print(f"300-client DP round: |moved - noise| = {worst:.3g}, sigma / N = {audit['sigma'] / BIG:.3g}")
    assert worst <= 2 * max(b.max() for _, b, _ in ref.values())  # test_gpu_dp_round.py's tolerance for this comparison
    again = StreamedNormClip(tau, chunk_clients=128, noise_multiplier=1.1, seed=5, sequence=3)
    again.init_global(g)
    same(again.server(upload(cl), 0)["w_glob"], got, "the same (seed, sequence), another chunk size")
    counter = next(k for k in g if k.endswith("num_batches_tracked"))
    assert rr.same_bits(_host(got[counter]), _host(plain[counter]))  # counters are not noised


# -- the server step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["avgm", "adagrad"])
def test_server_optimiser_over_three_rounds(op, g0, cuda):
    opt, opt_ref = ServerOptimizer(op), ServerOptimizer(op)
    opt.init_global(g0)
    opt_ref.init_global(g0)
    tau = float(np.median(norms_of(round_of(LENET, g0, N, 30), g0)))
    s, ref = StreamedNormClip(tau, server_opt=opt, chunk_clients=5), NormClip(tau=tau, server_opt=opt_ref)
    s.init_global(g0)
    ref.init_global(g0)
    centre = g0
    for r in range(3):
        cl = round_of(LENET, centre, N, 30 + r)
        got = s.server(upload(cl), r)["w_glob"]
        same(got, ref.server(upload(cl), r)["w_glob"], f"{op} round {r}")
        audits_equal(s.engine.last_clip, ref.engine.last_clip, f"{op} round {r}")
        assert 0 < s.engine.last_clip["clipped"].size < N
        assert all(rr.same_bits(opt.v_t()[k], opt_ref.v_t()[k]) for k in g0), r
        centre = {k: np.asarray(got[k]).astype(np.float32) for k in g0}
    assert any(np.abs(opt.v_t()[k]).max() > 0 for k in g0)


def test_first_round_without_init_global_is_the_streamed_mean(clients, cuda):
    finite = [c for i, c in enumerate(clients) if i not in (2, 9)]
    for k in (5, 16):
        s = StreamedNormClip(1e-3, chunk_clients=k)
        got = s.server(upload(finite, 0.5), 0)["w_glob"]
        audit = s.engine.last_clip
        assert audit["centered"] is False and audit["clipped"].size == 0 and audit["norm2"] is None
        assert sorted(audit) == AUDIT
        same(got, AVG(chunk_clients=k).server(upload(finite, 1), 0)["w_glob"], f"first round K={k}")
        s.server(upload(finite), 1)  # the second round is centred on the first's result
        assert s.engine.last_clip["centered"] is True and s.engine.last_clip["clipped"].size == len(finite)


# -- the order of the launches -----------------------------------------------------------------------------
def test_clip_fold_lags_the_norms_by_one_chunk(clients, g0, tau, cuda, monkeypatch):
    calls = []
    norm, fold = ops.rownorm2_stack, ops.clip_fold_stack
    # (what, the chunk stack's address: the two stack sets alternate, so a chunk's launches share one)
    monkeypatch.setattr(ops, "rownorm2_stack", lambda *a, **kw: (calls.append(("norm", a[0].data_ptr())), norm(*a, **kw))[1])
    monkeypatch.setattr(ops, "clip_fold_stack", lambda *a, **kw: (calls.append(("fold", a[0].data_ptr())), fold(*a, **kw))[1])
    s = StreamedNormClip(tau, chunk_clients=6)
    s.init_global(g0)
    rnd = s.engine.begin_clipped_round(tau, s._prev_glob, chunk_clients=6)
    ups = clients + clients[:1]  # 24 uploads: four full chunks, the fourth folded before finish()
    held = {}
    for i, c in enumerate(ups):
        rnd.add({"agg_weight": 1, "params": c})
        if (i + 1) % 6 == 0:
            held[(i + 1) // 6] = rnd.device_bytes
    got = rnd.finish()
    collapsed = [c for i, c in enumerate(calls) if i == 0 or calls[i - 1] != c]  # one norm launch per run of keys
    assert [what for what, _ in collapsed] == ["norm", "norm", "fold", "norm", "fold", "norm", "fold", "fold"]
    (a, b) = (collapsed[0][1], collapsed[1][1])
    assert a != b and [ptr for _, ptr in collapsed] == [a, b, a, a, b, b, a, b]  # norm(c) and fold(c) read set c % 2
    assert s.engine.last_clip["chunks"] == 4
    assert held[2] == held[3] == held[4] > 0  # from the 2nd chunk to the 4th nothing grows
    monkeypatch.undo()
    same(got, s.server(upload(ups), 0)["w_glob"], "the accumulator against the strategy")
