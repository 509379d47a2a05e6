"""GPU: a round aggregated in chunks of clients (Aggregator.begin_round, chunk_clients=, and
Strategy.begin_round) against the reference's golden fixtures.  Chunking must be invisible: every
result is bit-equal to the fixture's output — what the one-launch path returns — with its dtypes,
value types and key order, in all three output modes."""
import numpy as np
import pytest
import torch

from flearn_amd import AVG, AVGM, BN, LG, LG_R, OPT, Dyn
from flearn_amd import aggregator as agg
from flearn_amd import layouts
from flearn_amd.aggregator import Aggregator
from flearn_amd.semantics import KIND_F32
from golden_io import Golden, assert_dict_bitwise, bitwise_equal, cases, decode_weight, regenerate

pytestmark = pytest.mark.gpu

REDUCE_CASES = [c for c in cases() if c.startswith(("avg_", "bn_", "lg_", "trace_"))]
ROUND_CASES = [c for c in cases() if c.endswith("_rounds3") and not c.startswith("dyn_")]
DYN_CASES = [c for c in cases() if c.startswith("dyn_")]


def upload(clients, weights):
    return [{"agg_weight": w, "params": c} for w, c in zip(weights, clients)]


def strategy_for(g: Golden, **kw):
    call = g.meta["call"]
    if call.startswith("BN()"):
        return BN(**kw)
    if call.startswith("LG_R("):
        return LG_R(g.meta["shared_key_layers"], **kw)
    if call.startswith("LG("):
        return LG(g.meta["shared_key_layers"], **kw)
    return AVG(**kw)


def chunk_sizes(n):
    return sorted({max(1, k) for k in (1, 2, 3, n - 1, n, n + 1)})


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _check_output(got, g: Golden, output, where):
    want = g.output()
    first = g.clients()[0]
    assert list(got) == [k for k in first if k in want], f"{where}: first-client key order"
    if output == "reference":
        assert_dict_bitwise(got, want, where)
        kinds = g.output_kinds()
        for k, v in got.items():  # value types as the reference returns them
            if kinds[k].startswith("scalar:"):
                assert type(v).__name__ == kinds[k].split(":")[1], k
            elif kinds[k].startswith("torch:"):
                assert isinstance(v, torch.Tensor) and str(v.dtype) == kinds[k][6:], k
            else:
                assert isinstance(v, np.ndarray), k
        return
    for k, w in want.items():  # "float32" / "device": fl32(w_glob) for fp32 keys, what load_state_dict stores
        w = _host(w)
        if output == "device":
            assert isinstance(got[k], torch.Tensor) and got[k].is_cuda, k
        if w.dtype == np.float64 and g.meta["in_dtypes"][k] == "float32":
            w = w.astype(np.float32)
        assert bitwise_equal(_host(got[k]), w), f"{where}: {k}"


@pytest.mark.parametrize("output", ["reference", "float32", "device"])
@pytest.mark.parametrize("name", REDUCE_CASES)
def test_fixture_through_chunk_clients(name, output, cuda):
    """Every non-half reduce fixture through its strategy, chunk_clients in {1, 2, 3, N-1, N, N+1}:
    Python float / int, np.float32 / np.float64 / np.int64 weights, the BN model's int64 counter,
    torch CPU uploads, unequal key sets (the drop-in form keeps the reference's intersection)."""
    g = Golden(name)
    ups = upload(g.clients(), g.weights())
    for k in chunk_sizes(len(ups)):
        s = strategy_for(g, output=output, chunk_clients=k)
        got = s.server(ups, 0)["w_glob"]
        _check_output(got, g, output, f"{name} K={k} {output}")
        assert agg.last_launch()[0].startswith("fold_finish_kernel<") or output != "reference"


def test_fixtures_cover_every_weight_type():
    kinds = {e["t"] for n in REDUCE_CASES for e in Golden(n).meta["weights"]}
    assert {"pyfloat", "pyint", "np.float32", "np.float64", "np.int64"} <= kinds
    assert any(Golden(n).meta.get("input_kind") == "torch" for n in REDUCE_CASES)
    assert any("int64" in Golden(n).meta["in_dtypes"].values() for n in REDUCE_CASES)


@pytest.mark.parametrize("output", ["reference", "device"])
@pytest.mark.parametrize("name", ["avg_w1_n10", "avg_bnmodel_pyfloat_n4", "avg_np64_n10"])
def test_device_uploads_through_chunk_clients(name, output, cuda):
    """Uploads resident on the GPU: each chunk is gathered into its chunk stack (or read in place
    when it is one slab) and folded."""
    g = Golden(name)
    cl = [{k: torch.from_numpy(np.asarray(v)).to(cuda) for k, v in c.items()} for c in g.clients()]
    for k in (1, 3, len(cl)):
        s = AVG(output=output, chunk_clients=k)
        got = s.server(upload(cl, g.weights()), 0)["w_glob"]
        for key, w in g.output().items():
            w = _host(w)
            if output == "device" and w.dtype == np.float64 and g.meta["in_dtypes"][key] == "float32":
                w = w.astype(np.float32)
            assert bitwise_equal(_host(got[key]), w), (name, k, key)


# ---------------------------------------------------------------------------------------------
# multi-round fixtures: the server-fused optimizers and FedDyn, chunk_clients=2
# ---------------------------------------------------------------------------------------------


def _round_inputs(g, r):
    layout = [(k, tuple(s)) for k, s in g.meta["gen"]["layout"]]
    clients = regenerate(layout, 6, g.meta["gen"]["seeds"][r])
    return clients, [decode_weight(e) for e in g.meta["round_weights"][r]]


def _fused(op, **kw):
    return AVGM(server_side=True, **kw) if op == "avgm" else OPT(server_side=True, method=op, **kw)


def _prev0(g):
    return {k[6:]: v for k, v in g.arrays.items() if k.startswith("prev0:")}


@pytest.mark.parametrize("name", ROUND_CASES)
def test_server_fused_rounds_with_chunk_clients(name, cuda):
    g = Golden(name)
    s = _fused(g.meta["op"], chunk_clients=2)
    s.server_opt.init_global(_prev0(g))
    for r in range(g.meta["rounds"]):
        clients, weights = _round_inputs(g, r)
        got = s.server(upload(clients, weights), r)["w_glob"]
        assert_dict_bitwise(got, g.output(f"w{r}"), f"{name} w{r}")
        assert_dict_bitwise(s.server_opt.v_t(), g.output(f"v{r}"), f"{name} v{r}")


def test_server_fused_first_round_without_a_previous_model(cuda):
    """No init_global: round 0 returns the mean and adopts it (prev = fl32(mean), v_t = 0), as the
    one-launch path does; round 1 is then the same fused step on both paths."""
    g = Golden("avgm_pyfloat_rounds3")
    a, b = _fused("avgm"), _fused("avgm", chunk_clients=4)
    for r in range(2):
        clients, weights = _round_inputs(g, r)
        want = a.server(upload(clients, weights), r)["w_glob"]
        got = b.server(upload(clients, weights), r)["w_glob"]
        assert_dict_bitwise(got, want, f"round {r}")
    assert_dict_bitwise(b.server_opt.v_t(), a.server_opt.v_t(), "v_t")


def test_server_fused_restart_between_chunked_rounds(cuda):
    g = Golden("adagrad_pyfloat_rounds3")
    s = _fused("adagrad", chunk_clients=2)
    s.server_opt.init_global(_prev0(g))
    clients, weights = _round_inputs(g, 0)
    s.server(upload(clients, weights), 0)
    saved = s.server_opt.state_dict()
    del s
    s = _fused("adagrad", chunk_clients=2)
    s.server_opt.load_state(saved)
    for r in range(1, g.meta["rounds"]):
        clients, weights = _round_inputs(g, r)
        got = s.server(upload(clients, weights), r)["w_glob"]
        assert_dict_bitwise(got, g.output(f"w{r}"), f"w{r} after restore")
        assert_dict_bitwise(s.server_opt.v_t(), g.output(f"v{r}"), f"v{r} after restore")


def _dyn_inputs(g, r):
    keys = g.meta["client_keys"]
    clients = [{k: g.arrays[f"r{r}x{i}:{k}"].copy() for k in keys} for i in range(g.meta["n_clients"])]
    return clients, [decode_weight(e) for e in g.meta["round_weights"][r]]


def _dyn_h0(g):
    return {k[6:]: v.copy() for k, v in g.arrays.items() if k.startswith("hinit:")}


@pytest.mark.parametrize("streamed", ["chunk_clients", "begin_round"])
@pytest.mark.parametrize("name", DYN_CASES)
def test_dyn_rounds_streamed(name, streamed, cuda):
    g = Golden(name)
    h = _dyn_h0(g)
    s = Dyn(h, chunk_clients=2)
    for r in range(g.meta["rounds"]):
        clients, weights = _dyn_inputs(g, r)
        if streamed == "chunk_clients":
            got = s.server(upload(clients, weights), r)["w_glob"]
        else:
            rnd = s.begin_round(r)
            for u in upload(clients, weights):
                rnd.add(u)
            got = rnd.finish()["w_glob"]
        assert_dict_bitwise(got, g.output(f"w{r}"), f"{name} w{r}")
        assert s.theta is got  # dyn.py:34
        assert s.h is h
        assert_dict_bitwise(s.h, g.output(f"h{r}"), f"{name} h{r}")
        dev = s._dyn.dev_keys
        assert_dict_bitwise({k: v for k, v in s._dyn.theta_host().items() if k in dev},
                            {k: np.asarray(v) for k, v in g.output(f"theta{r}").items() if k in dev}, f"{name} theta{r}")


def test_dyn_partial_h_streamed_equals_one_launch(cuda):
    g = Golden("dyn_pyfloat_rounds3")
    h0 = _dyn_h0(g)
    for drop in ("bn1.weight", "fc.bias"):
        h0.pop(drop)
    a = Dyn({k: v.copy() for k, v in h0.items()})
    b = Dyn({k: v.copy() for k, v in h0.items()}, chunk_clients=2)
    for r in range(2):
        clients, weights = _dyn_inputs(g, r)
        want = a.server(upload(clients, weights), r)["w_glob"]
        got = b.server(upload(clients, weights), r)["w_glob"]
        assert_dict_bitwise(got, want, f"w{r}")
        assert_dict_bitwise(b.h, a.h, f"h{r}")


# ---------------------------------------------------------------------------------------------
# begin_round + add one by one + finish == server() on the same list
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["avg_lenet5_n10", "avg_bnmodel_pyint_n4", "bn_strategy_n4", "lg_strategy_n4",
                                  "lg_r_strategy_n4", "avg_torch_n3"])
def test_begin_round_equals_server(name, cuda):
    g = Golden(name)
    ups = upload(g.clients(), g.weights())
    want = strategy_for(g).server(ups, 0)
    for k in (None, 1, 3):
        s = strategy_for(g, chunk_clients=k)
        rnd = s.begin_round(0)
        for u in ups:
            rnd.add(u)
        got = rnd.finish()
        assert list(got) == list(want) == ["w_glob"]
        assert list(got["w_glob"]) == list(want["w_glob"])
        assert_dict_bitwise(got["w_glob"], want["w_glob"], f"{name} K={k}")
        assert_dict_bitwise(got["w_glob"], g.output(), f"{name} K={k} fixture")
        for key in want["w_glob"]:
            assert type(got["w_glob"][key]) is type(want["w_glob"][key]), key


def test_distill_begin_round_equals_server(cuda):
    """FedDistill's logits ride next to the params: begin_round keeps them and averages them at finish()."""
    from flearn_amd import Distill

    g = Golden("distill_server_n4")
    ups = upload(g.clients(), g.weights())
    for i, u in enumerate(ups):
        u["logits"] = torch.from_numpy(g.arrays[f"logits{i}"].copy())
    want = Distill().server(ups, 0)
    rnd = Distill(chunk_clients=3).begin_round(0)
    for u in ups:
        rnd.add(u)
    got = rnd.finish()
    assert list(got) == list(want) == ["w_glob", "glob_logits"]
    assert_dict_bitwise(got["w_glob"], g.output(), "distill w_glob")
    assert_dict_bitwise({"glob_logits": got["glob_logits"].numpy()}, g.output("glob"), "distill glob_logits")


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name,strategy", [("avg_lenet5_n10", AVG), ("avg_bnmodel_pyint_n4", AVG), ("bn_strategy_n4", BN)])
def test_begin_round_takes_encoded_uploads(name, strategy, fast, cuda):
    """HTTP mode: add(encoded string) goes through receive_processing; the codec's pinned rows are
    packed chunk by chunk like any upload."""
    from flearn_amd.wire import Encrypt

    g = Golden(name)
    enc = Encrypt(fast_min_chars=0 if fast else None)
    s = strategy(encrypt=enc, chunk_clients=3)
    rnd = s.begin_round(0)
    for w, c in zip(g.weights(), g.clients()):
        rnd.add(enc.encode({"agg_weight": w, "params": c}))
    assert_dict_bitwise(rnd.finish()["w_glob"], g.output(), name)


# ---------------------------------------------------------------------------------------------
# the memory bound
# ---------------------------------------------------------------------------------------------


def _lenet_round(engine, n, k, rng):
    shapes = [(key, tuple(s)) for key, s, kind in layouts.get("lenet5") if kind == "f32"]
    assert len(shapes) == 10
    rnd = engine.begin_round(chunk_clients=k)
    ups = []
    for _ in range(n):
        p = {key: rng.standard_normal(s).astype(np.float32) for key, s in shapes}
        ups.append(p)
        rnd.add({"agg_weight": 1.0, "params": p})
    return rnd, ups, rnd.finish()


def test_device_bytes_do_not_grow_with_the_client_count(cuda):
    rng = np.random.default_rng(5)
    k = 4
    sizes, rows = [], []
    for n in (4, 40):
        engine = Aggregator()
        rnd, ups, got = _lenet_round(engine, n, k, rng)
        want = Aggregator().ensemble([1.0] * n, ups)
        assert_dict_bitwise(got, want, f"n={n}")
        sizes.append(rnd.device_bytes)
        rows.append(rnd.max_stack_rows)
        stride = engine.last_plan.groups[KIND_F32].stride
        assert set(engine.last_plan.groups) == {KIND_F32}
        # two chunk stacks, the accumulator (at most 8 B per column, possibly double-buffered) and the outputs
        assert 0 < rnd.device_bytes <= 2 * k * stride * 4 + 2 * stride * 8 + stride * (4 + 8)
        for p in engine._chunk_packers:  # the packers' device stacks never have more than K rows
            for (tag, _), t in p._dev.items():
                if tag[0] == "in":
                    assert t.numel() <= k * stride, (tag, t.numel())
    assert sizes[0] == sizes[1] and rows == [k, k]


# ---------------------------------------------------------------------------------------------
# refusals and errors
# ---------------------------------------------------------------------------------------------


def _two():
    g = Golden("avg_w1_n3")
    return g, upload(g.clients(), g.weights())


def test_refusals(cuda):
    g, ups = _two()
    half = {"agg_weight": 1.0, "params": {"w": np.ones(8, np.float16)}}
    with pytest.raises(TypeError, match="float16"):
        Aggregator().begin_round().add(half)
    with pytest.raises(SystemExit):
        AVG(chunk_clients=2).server([half, half], 0)
    with pytest.raises(ValueError, match="devices"):
        Aggregator(devices=[cuda, cuda]).begin_round()
    with pytest.raises(SystemExit):  # through a strategy: server_exception, like every refused round
        AVG(devices=[cuda, cuda], chunk_clients=2).server(ups, 0)
    rnd = Aggregator().begin_round(chunk_clients=2)
    for u in ups:
        rnd.add(u)
    assert_dict_bitwise(rnd.finish(), g.output(), "finish")
    with pytest.raises(RuntimeError, match="after finish"):
        rnd.add(ups[0])
    with pytest.raises(IndexError):  # what ensemble([], []) raises
        Aggregator().begin_round().finish()
    with pytest.raises(SystemExit):
        AVG().begin_round(0).finish()
    with pytest.raises(SystemExit):
        AVG(chunk_clients=2).server([], 0)


def test_group_is_refused(cuda, monkeypatch):
    """group=True: a streamed round is not sharded over a process group (checked on an engine whose
    group flag is set: no process group is needed to see the refusal)."""
    engine = Aggregator()
    monkeypatch.setattr(engine, "_dist", True)
    with pytest.raises(ValueError, match="group"):
        engine.begin_round()


@pytest.mark.parametrize("k", [1, 2, 5])
def test_later_uploads_off_the_layout_exit_through_the_strategy(k, cuda):
    g, ups = _two()
    p1 = ups[1]["params"]
    first = next(iter(p1))
    missing = {"agg_weight": 1.0, "params": {key: v for key, v in p1.items() if key != first}}
    reshaped = {"agg_weight": 1.0, "params": {**p1, first: np.asarray(p1[first]).reshape(-1)[:-1].copy()}}
    promoted = {"agg_weight": np.float64(1.0), "params": p1}
    for bad in (missing, reshaped, promoted):
        if bad is not missing:  # server() sees the whole list: a missing key narrows the intersection, as ever
            with pytest.raises(SystemExit):
                AVG(chunk_clients=k).server([ups[0], bad, ups[2]], 0)
        rnd = AVG(chunk_clients=k).begin_round(0)
        rnd.add(ups[0])
        with pytest.raises(SystemExit):
            rnd.add(bad)
    engine_rnd = Aggregator().begin_round(chunk_clients=k)
    engine_rnd.add(ups[0])
    with pytest.raises(KeyError):
        engine_rnd.add(missing)
    with pytest.raises(ValueError):
        engine_rnd.add(reshaped)
    with pytest.raises(TypeError, match="promote differently"):
        engine_rnd.add(promoted)


def test_refused_fused_round_leaves_the_state(cuda, monkeypatch):
    """A streamed fused round whose finish launch is refused leaves v_t and the previous global model
    bit-equal to before it; the rounds after it still match the reference."""
    from flearn_amd import ops

    g = Golden("avgm_pyfloat_rounds3")
    s = _fused("avgm", chunk_clients=2)
    s.server_opt.init_global(_prev0(g))
    real = ops.fold_finish
    for r in range(g.meta["rounds"]):
        clients, weights = _round_inputs(g, r)
        if r == 1:
            before = s.server_opt.state_dict()

            def refuse(*a, **k):
                if k.get("epi") is not None:
                    raise ValueError("refused launch")
                return real(*a, **k)

            monkeypatch.setattr(ops, "fold_finish", refuse)
            with pytest.raises(SystemExit):
                s.server(upload(clients, weights), r)
            monkeypatch.setattr(ops, "fold_finish", real)
            after = s.server_opt.state_dict()
            assert_dict_bitwise(after["v_t"], before["v_t"], "v_t after a refused round")
            assert_dict_bitwise(after["w_glob"], before["w_glob"], "previous global model after a refused round")
        got = s.server(upload(clients, weights), r)["w_glob"]
        assert_dict_bitwise(got, g.output(f"w{r}"), f"w{r}")
        assert_dict_bitwise(s.server_opt.v_t(), g.output(f"v{r}"), f"v{r}")
