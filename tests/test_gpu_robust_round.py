"""GPU: robust rounds through the strategies (TrimmedMean, Median -> Aggregator.ensemble_trimmed)
against the numpy restatement of the rules (tests/robust_ref.py), bit for bit: the three output
modes, every upload form, permuted and poisoned rounds, the server-fused AVGM / Adagrad step
(expected values from the one-launch reduce kernel over robust_ref's sums) and the refusals.
The clients are those of existing golden fixtures, read and not modified."""
import numpy as np
import pytest
import torch

import robust_ref as rr
from flearn_amd import AVG, Median, TrimmedMean, device_state_dicts, ops
from flearn_amd import _native as na
from flearn_amd.aggregator import Aggregator, DynState, ServerOptimizer
from golden_io import Golden

pytestmark = pytest.mark.gpu

OUTPUTS = ("reference", "float32", "device")


def upload(clients, weight=1.0):
    return [{"agg_weight": weight, "params": c} for c in clients]


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.fixture(scope="module")
def lenet():
    return Golden("avg_lenet5_n10").clients()


@pytest.fixture(scope="module")
def bnmodel():
    return Golden("avg_bnmodel_pyint_n4").clients()


@pytest.fixture(scope="module")
def lenet_ref(lenet):
    """robust_ref's float64 global models of the ten LeNet5 clients, by trim count (computed once)."""
    return {t: rr.ensemble(lenet, t) for t in (2, 4)}


def check(got, want, output, where, in_dtypes=None):
    """got against robust_ref's reference-typed `want`: "reference" holds it as it is, "float32" /
    "device" hold fl32 of it for fp32 keys."""
    assert list(got) == list(want), f"{where}: key order"
    for k, w in want.items():
        g = got[k]
        if output == "device":
            assert isinstance(g, torch.Tensor) and g.is_cuda, k
        w = np.asarray(w)
        if output != "reference" and (in_dtypes is None or in_dtypes[k] == np.float32):
            with np.errstate(all="ignore"):
                w = w.astype(np.float32)
        assert rr.same_bits(_host(g), w), f"{where}: {k}"


@pytest.mark.parametrize("output", OUTPUTS)
def test_plain_rounds_lenet(output, lenet, lenet_ref, cuda):
    for make, t in ((lambda **k: TrimmedMean(0.2, **k), 2), (lambda **k: TrimmedMean(2, **k), 2),
                    (lambda **k: Median(**k), 4)):
        s = make(output=output)
        got = s.server(upload(lenet), 0)["w_glob"]
        check(got, lenet_ref[t], output, f"{type(s).__name__} t={t} {output}")
        assert s.engine.last_plan.groups["f32"].numerics.denom == 10 - 2 * t
    assert ops.last_launch()[0].startswith("fold_finish_kernel<")
    if output == "reference":  # the robust rounds left make_plan's cached plan for these uploads as it was
        got = AVG().server(upload(lenet, 1), 1)["w_glob"]
        for k in lenet[0]:
            acc = lenet[0][k].copy()
            for c in lenet[1:]:
                acc = acc + c[k]
            assert rr.same_bits(got[k], acc.astype(np.float64) / np.float64(10)), k


@pytest.mark.parametrize("output", OUTPUTS)
def test_median_of_the_bn_model_counts_through_the_elem_kernel(output, bnmodel, cuda, monkeypatch):
    launched = []
    real = ops.trim_sum_stack

    def spy(*a, **k):
        real(*a, **k)
        launched.append(ops.last_launch()[0])

    monkeypatch.setattr(ops, "trim_sum_stack", spy)
    got = Median(output=output).server(upload(bnmodel, 3), 0)["w_glob"]
    want = rr.ensemble(bnmodel, 1)
    check(got, want, output, f"bn median {output}", {k: np.asarray(v).dtype for k, v in bnmodel[0].items()})
    assert sorted(launched) == ["trim_kernel_elem<long>", "trim_kernel_rows<4,4,true>"]
    counts = sorted(int(c["bn1.num_batches_tracked"]) for c in bnmodel)
    assert float(_host(got["bn1.num_batches_tracked"])) == (counts[1] + counts[2]) / 2


def test_reference_dtypes_value_types_and_key_order(bnmodel, lenet, cuda):
    got = TrimmedMean(1).server(upload(bnmodel), 0)["w_glob"]
    assert list(got) == list(bnmodel[0])
    for k, v in got.items():
        if np.asarray(bnmodel[0][k]).ndim == 0:
            assert type(v) is np.float64, k  # a numpy scalar, as the reference returns 0-d buffers
        else:
            assert isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == bnmodel[0][k].shape, k
    check(got, rr.ensemble(bnmodel, 1), "reference", "bn t=1")
    # float64 uploads stay float64 sums; keys some client lacks drop out, extra keys are ignored
    cl = [{"a": c["fc3.weight"].astype(np.float64) * 1.5, "b": c["fc3.bias"], "only%d" % i: np.zeros(3, np.float32)}
          for i, c in enumerate(lenet[:7])]
    got = TrimmedMean(2).server(upload(cl), 0)["w_glob"]
    check(got, rr.ensemble(cl, 2, keys=["a", "b"]), "reference", "f64 keys")
    assert got["a"].dtype == np.float64 and got["b"].dtype == np.float64
    key_lst = ["fc3.bias", "conv1.bias"]
    got = TrimmedMean(2).engine.ensemble_trimmed(lenet, 2, key_lst)
    check(got, rr.ensemble(lenet, 2, keys=key_lst), "reference", "key_lst")


def test_upload_forms_give_the_same_bits(lenet, bnmodel, lenet_ref, cuda):
    for clients, t, want in ((lenet, 2, lenet_ref[2]), (bnmodel, 1, rr.ensemble(bnmodel, 1))):
        for output in ("reference", "device"):
            dts = {k: np.asarray(v).dtype for k, v in clients[0].items()}
            s = TrimmedMean(t, output=output)
            cpu = [{k: torch.from_numpy(np.asarray(v).copy()) for k, v in c.items()} for c in clients]
            got = s.server(upload(cpu), 0)["w_glob"]
            check(got, want, output, f"torch cpu {output}", dts)
            if output == "reference":
                assert all(isinstance(v, torch.Tensor) and not v.is_cuda for v in got.values())
            dev = [{k: v.to(cuda) for k, v in c.items()} for c in cpu]
            got = s.server(upload(dev), 1)["w_glob"]
            check(got, want, output, f"device uploads {output}", dts)
            assert s.engine.packer.last_row_tables["f32"] in ("rows", "gather")
            slab = device_state_dicts(cpu[0], len(cpu), cuda)
            for d, c in zip(slab, cpu):
                for k, v in c.items():
                    d[k].copy_(v)
            got = s.server(upload(slab), 2)["w_glob"]
            check(got, want, output, f"slab uploads {output}", dts)
            assert s.engine.packer.last_row_tables["f32"] == "slab"
            torch.cuda.synchronize()


def test_permuting_the_uploads_changes_no_bit(lenet, lenet_ref, cuda):
    rng = np.random.default_rng(0)
    for s, t in ((TrimmedMean(2), 2), (Median(), 4)):
        for _ in range(3):
            perm = rng.permutation(len(lenet))
            ups = [{"agg_weight": float(i + 1), "params": lenet[i]} for i in perm]  # the weights are not used
            check(s.server(ups, 0)["w_glob"], lenet_ref[t], "reference", f"perm {perm}")


def test_poisoned_round(lenet, cuda):
    """Two of ten clients poisoned — one uploads NaN, one a model scaled by 1e30 — and trim = 2: every
    element of the global model is finite and robust_ref's; FedAVG on the same uploads is not finite."""
    cl = [dict(c) for c in lenet]
    cl[3] = {k: np.full_like(v, np.nan) for k, v in cl[3].items()}
    cl[7] = {k: v * np.float32(1e30) for k, v in cl[7].items()}
    assert all(np.isfinite(v).all() for v in cl[7].values())
    for output in OUTPUTS:
        got = TrimmedMean(trim=2, output=output).server(upload(cl), 0)["w_glob"]
        check(got, rr.ensemble(cl, 2), output, f"poisoned {output}")
        assert all(np.isfinite(_host(v)).all() for v in got.values())
        assert all(np.abs(_host(v)).max() <= 1.0 for v in got.values())  # the clients' values are in (-1, 1)
    avg = AVG().server(upload(cl), 0)["w_glob"]
    assert not any(np.isfinite(_host(v)).any() for v in avg.values())
    one_nan = TrimmedMean(trim=0).server(upload(cl), 0)["w_glob"]  # a NaN among the kept values gives NaN
    assert all(np.isnan(_host(v)).all() for v in one_nan.values())


# ---------------------------------------------------------------------------------------------
# server-fused AVGM / Adagrad: expected values from the one-launch reduce kernel over robust_ref's sums
# ---------------------------------------------------------------------------------------------


def reduce_kernel_step(opt, sums32, denom, prev32, v64, cuda):
    """(w float64, fl32(w), v') of the fused step on fp32 sums: ops.reduce_stack over a one-row stack
    holding the sums with weight fl32(1.0) — the sum is the row itself — the same op and state."""
    n = sums32.size
    m = -(-n // 64) * 64

    def pad(a, dt):
        return torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(m - n, dt)]).astype(dt)).to(cuda)

    stack = pad(sums32, np.float32).view(1, m)
    prev, v = pad(prev32, np.float32), pad(v64, np.float64)
    out32, out64, v_out = torch.empty_like(prev), torch.empty_like(v), torch.empty_like(v)
    one = torch.ones(1, dtype=torch.float32, device=cuda)
    ops.reduce_stack(stack, one, na.MODE_W32_DIV64, float(denom), out32=out32, out64=out64, op=opt.op, prev=prev, v=v,
                     v_out=v_out, beta=opt.beta, eta=opt.eta, tau=opt.tau, beta2=opt.beta2)
    assert ops.last_launch()[0].startswith("reduce_kernel_")
    shape = sums32.shape
    return tuple(t.cpu().numpy()[:n].reshape(shape) for t in (out64, out32, v_out))


@pytest.mark.parametrize("op", ["avgm", "adagrad"])
def test_server_fused_rounds(op, lenet, cuda, monkeypatch):
    opt = ServerOptimizer(op)
    s = TrimmedMean(2, server_opt=opt)
    rng = np.random.default_rng(9)
    prev = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in lenet[0].items()}
    v = {k: np.zeros(a.shape, np.float64) for k, a in prev.items()}
    opt.init_global(prev)
    real = ops.fold_finish
    for r in range(3):
        clients = [{k: (a * np.float32(1 + r) + np.float32(0.01 * i * r)).astype(np.float32) for k, a in c.items()}
                   for i, c in enumerate(lenet)]
        if r == 1:  # a refused finish launch leaves the state on the pair it had
            before = opt.state_dict()

            def refuse(*a, **k):
                raise ValueError("refused launch")

            monkeypatch.setattr(ops, "fold_finish", refuse)
            with pytest.raises(SystemExit):
                s.server(upload(clients), r)
            monkeypatch.setattr(ops, "fold_finish", real)
            after = opt.state_dict()
            for part in ("w_glob", "v_t"):
                assert all(rr.same_bits(after[part][k], before[part][k]) for k in prev), part
        got = s.server(upload(clients), r)["w_glob"]
        for k in prev:
            sums = rr.trimmed_sum(np.stack([c[k] for c in clients]), 2)
            w64, prev[k], v[k] = reduce_kernel_step(opt, sums, 6, prev[k], v[k], cuda)
            assert rr.same_bits(got[k], w64), (op, r, k)
        vt = opt.v_t()
        assert all(rr.same_bits(vt[k], v[k]) for k in prev), (op, r)
        assert all(rr.same_bits(opt.state_dict()["w_glob"][k], prev[k]) for k in prev), (op, r)
    assert any(np.abs(v[k]).max() > 0 for k in v)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------


def test_refusals_exit_through_the_strategy_and_leave_the_engine_usable(lenet, lenet_ref, cuda):
    s = TrimmedMean(2)
    half = upload([{"w": np.ones(8, np.float16) * i} for i in range(5)])
    with pytest.raises(SystemExit):
        s.server(half, 0)
    check(s.server(upload(lenet), 1)["w_glob"], lenet_ref[2], "reference", "after float16")
    s.server_opt = DynState({k: np.zeros_like(v) for k, v in lenet[0].items()})
    with pytest.raises(SystemExit):
        s.server(upload(lenet), 2)
    s.server_opt = None
    check(s.server(upload(lenet), 3)["w_glob"], lenet_ref[2], "reference", "after Dyn state")
    many = upload([{"w": np.full(8, i, np.float32)} for i in range(129)])
    with pytest.raises(SystemExit):
        s.server(many, 4)
    with pytest.raises(SystemExit):  # 2 * trim >= N
        s.server(upload(lenet[:4]), 5)
    with pytest.raises(SystemExit):
        s.server([], 6)
    with pytest.raises(KeyError):  # agg_weight must be present, as in flearn's upload format (not used)
        s.server([{"params": c} for c in lenet], 7)
    check(s.server(upload(lenet), 8)["w_glob"], lenet_ref[2], "reference", "after every refusal")
    check(s.server(many[:128], 9)["w_glob"], rr.ensemble([u["params"] for u in many[:128]], 2), "reference", "N = 128")
    with pytest.raises(SystemExit):
        TrimmedMean(2, devices=[cuda, cuda]).server(upload(lenet), 0)
    with pytest.raises(SystemExit):
        TrimmedMean(2, chunk_clients=4).server(upload(lenet), 0)
    with pytest.raises(SystemExit):
        Median(chunk_clients=4).server(upload(lenet), 0)


def test_engine_refusals_name_their_reason(lenet, cuda, monkeypatch):
    eng = Aggregator()
    with pytest.raises(TypeError, match="float16"):
        eng.ensemble_trimmed([{"w": np.ones(8, np.float16)}] * 3, 1)
    with pytest.raises(TypeError, match="Dyn"):
        eng.ensemble_trimmed(lenet, 2, server_opt=DynState({k: np.zeros_like(v) for k, v in lenet[0].items()}))
    with pytest.raises(ValueError, match="128"):
        eng.ensemble_trimmed([{"w": np.ones(8, np.float32)}] * 129, 1)
    for bad in (-1, 5, 2.0, True):
        with pytest.raises(ValueError, match="trim"):
            eng.ensemble_trimmed(lenet, bad)
    with pytest.raises(ValueError, match="devices"):
        Aggregator(devices=[cuda, cuda]).ensemble_trimmed(lenet, 2)
    with pytest.raises(ValueError, match="chunk_clients"):
        Aggregator(chunk_clients=4).ensemble_trimmed(lenet, 2)
    monkeypatch.setattr(eng, "_dist", True)
    with pytest.raises(ValueError, match="group"):
        eng.ensemble_trimmed(lenet, 2)
