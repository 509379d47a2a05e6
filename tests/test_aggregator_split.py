"""flearn_amd.aggregator after its split into ops (device entry points), serverstate (resident
optimizer state) and smallround (the small-host-round records), and the one server step that
one-launch and streamed rounds share: every name the two modules defined is still importable from
them and is the object of its new home; the modules import each other in one direction, at module
level; the shared step asks a stack-like and a folded-like sum for the same thing and advances
the state only after the sum's launch returned; and ops.FoldedSum hands fa_fold_finish the
epilogue reduce_stack would build.  The robust rounds live in robustround and are bound on the
class; what they share with the other rounds (Packer.dense_stack, Packer.hold_slab,
bucketplan.key_runs) is checked here on CPU stand-ins.  No GPU."""
import ast
import contextlib
import importlib
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from flearn_amd import _native as na
from flearn_amd.semantics import KIND_F32

#: the names flearn_amd.aggregator defined before the split, by new home ...
MOVED = {
    "flearn_amd.ops": ["_ptr", "_check_cuda", "_check_window", "_check_stack", "_check_weights", "_check_arrays",
                       "_epilogue", "_byte_range", "_check_v_out", "reduce_stack", "_reduce_stack8", "reduce_stack_f64",
                       "reduce_stack_i64", "reduce_stack_f16", "apply_update", "apply_dyn", "set_reduce_grid",
                       "last_launch", "fill_uniform", "mean_tables"],
    "flearn_amd.serverstate": ["_layout_signature", "_flatten", "_to_shards", "_bucket_host", "ServerOptimizer",
                               "_host_array", "_as_host", "DynState"],
    "flearn_amd.smallround": ["chain_table", "_SmallChain", "_SmallBucket", "_SmallRecord"],
}
KEPT = ["_F64", "_ONE_W32", "OUTPUTS", "Aggregator", "assemble_on_device"]
#: ... and flearn_amd.streaming's (its own _ptr was a copy of the aggregator's)
STREAMING_MOVED = ["_ACC_TORCH", "acc_kind_of", "fold_stack", "fold_finish"]
STREAMING_KEPT = ["_F16", "_F64", "RoundAccumulator"]

ENGINE = ("ops", "serverstate", "smallround", "robustround", "aggregator", "streaming", "dist")
ROOT = Path(__file__).resolve().parent.parent / "flearn_amd"


@pytest.mark.parametrize("home", sorted(MOVED))
def test_aggregator_still_exports_every_name(home):
    from flearn_amd import aggregator

    mod = importlib.import_module(home)
    for name in MOVED[home]:
        assert getattr(aggregator, name) is getattr(mod, name), name
    for name in KEPT:
        assert hasattr(aggregator, name), name


def test_streaming_still_exports_every_name():
    from flearn_amd import ops, streaming

    for name in STREAMING_MOVED:
        assert getattr(streaming, name) is getattr(ops, name), name
    for name in STREAMING_KEPT:
        assert hasattr(streaming, name), name


def test_small_round_switches_stay_on_the_class():
    from flearn_amd import smallround
    from flearn_amd.aggregator import Aggregator

    assert Aggregator.small_zero_copy is True and Aggregator.small_parts == 1
    assert Aggregator._small_round is smallround._small_round  # bound as a method: no call layer in between


def test_robust_rounds_are_bound_on_the_class():
    from flearn_amd import aggregator, bucketplan, robustround
    from flearn_amd.aggregator import Aggregator

    assert aggregator.key_runs is bucketplan.key_runs
    assert Aggregator.ensemble_trimmed is robustround.ensemble_trimmed  # bound as _small_round is
    assert Aggregator.ensemble_krum is robustround.ensemble_krum
    assert Aggregator._check_center is robustround._check_center  # a staticmethod: no engine needed
    assert Aggregator._center_row is robustround._center_row
    assert Aggregator._check_center(None, None) is None
    assert Aggregator.last_krum is None  # before the first Krum round
    for name in ("ensemble_trimmed", "ensemble_krum", "_check_center", "_center_row"):
        assert getattr(Aggregator, name).__doc__, name


def _package_imports(mod: str):
    """(names of the package a module's imports mention, those of them below module level)."""
    tree = ast.parse((ROOT / f"{mod}.py").read_text())
    top = {id(n) for n in tree.body}
    every, nested = set(), set()
    for node in ast.walk(tree):
        names = []
        if isinstance(node, ast.ImportFrom) and (node.level or (node.module or "").startswith("flearn_amd")):
            names = (node.module or "").split(".") + [a.name for a in node.names]
        elif isinstance(node, ast.Import):
            names = [p for a in node.names if a.name.startswith("flearn_amd") for p in a.name.split(".")]
        names = {n for n in names if (ROOT / f"{n}.py").exists()}
        every |= names
        if id(node) not in top:
            nested |= names
    return every, nested


def test_import_graph_has_one_direction():
    assert _package_imports("ops")[0] <= {"_native", "rowtable", "semantics"}
    for mod in ("serverstate", "smallround"):
        assert not _package_imports(mod)[0] & {"aggregator", "streaming"}, mod
    assert "aggregator" not in _package_imports("streaming")[0]
    assert not _package_imports("robustround")[0] & {"aggregator", "streaming"}
    for mod in ENGINE:  # no import of one another inside a function
        assert not _package_imports(mod)[1] & set(ENGINE), mod


# -- what the rounds share of the packer and the plan ---------------------------------------------


def _pool_packer(last_row_tables=()):
    """A Packer with no device: its buffers come from the CPU and `hold` only records."""
    from flearn_amd.packer import Packer

    class PoolPacker(Packer):
        def __init__(self):
            self.made, self.held, self.last_row_tables = {}, [], dict(last_row_tables)

        def device_bucket(self, tag, shape, dtype, device=None):
            assert tag not in self.made, tag
            self.made[tag] = torch.zeros(shape, dtype=dtype)
            return self.made[tag]

        def hold(self, objs, device):
            self.held.append((objs, device))

    return PoolPacker()


def _fake_row_table(log):
    from flearn_amd.rowtable import RowTable

    class FakeRows(RowTable):
        def gather_into(self, stack):
            log.append(stack)

    return object.__new__(FakeRows)


def test_dense_stack_gathers_a_row_table_once_and_passes_a_stack_through(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())  # CPU shards
    _, plan, (sh, other) = _two_cpu_shards()
    stride = plan.f32.stride
    packer = _pool_packer()
    stack = torch.zeros(2, stride)
    got = packer.dense_stack(plan, KIND_F32, [(sh, stack)], 2)
    assert got[0] is sh and got[1] is stack and not packer.made  # as packed: no buffer, no copy
    log = []
    got = packer.dense_stack(plan, KIND_F32, [(other, _fake_row_table(log))], 5)
    ((tag, buf),) = packer.made.items()
    assert tag == ("in", KIND_F32, other.index) and buf.shape == (5, stride) and buf.dtype == torch.float32
    assert got[0] is other and got[1] is buf
    assert len(log) == 1 and log[0] is buf  # one gather, into that bucket
    with pytest.raises(ValueError):  # a column-sharded bucket has no dense stack
        packer.dense_stack(plan, KIND_F32, [(sh, stack), (other, stack)], 2)
    with pytest.raises(ValueError):
        packer.dense_stack(plan, KIND_F32, [], 2)


def test_hold_slab_holds_only_what_was_read_in_place():
    a, b = torch.zeros(3), torch.zeros(3)
    packer = _pool_packer({KIND_F32: "slab"})
    packer.hold_slab(KIND_F32, (t for t in (a, b)), "dev")  # any iterable of stacks
    ((objs, device),) = packer.held
    assert len(objs) == 2 and objs[0] is a and objs[1] is b and device == "dev"
    for how in ("rows", "gather", "copy"):
        packer = _pool_packer({KIND_F32: how})
        packer.hold_slab(KIND_F32, [a], "dev")
        assert packer.held == [], how
    packer = _pool_packer({KIND_F32: "slab"})
    packer.hold_slab("f64", [a], "dev")  # a kind the last pack did not see as device uploads
    assert packer.held == []


def test_key_runs_merge_adjacent_keys_and_split_at_padding():
    from flearn_amd.bucketplan import Group, Segment, key_runs

    f32 = np.dtype(np.float32)

    def group(*segs):  # (numel, offset) per key
        return Group(KIND_F32, None, [Segment(f"k{i}", (n,), n, off, f32) for i, (n, off) in enumerate(segs)], 512)

    assert key_runs(group((64, 0), (128, 64), (5, 192))) == [(0, 197)]  # whole ALIGN spans: no gap
    assert key_runs(group((10, 0), (64, 64), (3, 128), (7, 192))) == [(0, 10), (64, 131), (192, 199)]
    # a zero-element key takes a padded span of its own and is no run; nor does it join its neighbours
    assert key_runs(group((64, 0), (0, 64), (64, 128))) == [(0, 64), (128, 192)]
    assert key_runs(group((0, 0), (64, 64), (0, 128))) == [(64, 128)]
    assert key_runs(group((0, 0))) == [] and key_runs(group()) == []


# -- the shared f32 step ------------------------------------------------------------------------


def _two_cpu_shards():
    from flearn_amd.bucket import Shard, make_plan

    rng = np.random.default_rng(11)
    model = {"a": rng.standard_normal((10, 10)).astype(np.float32), "b": rng.standard_normal(7).astype(np.float32)}
    plan = make_plan([1.0, 1.0], [model, model])
    cpu = torch.device("cpu")
    return model, plan, [Shard(0, cpu, 0, 64), Shard(1, cpu, 64, plan.f32.stride)]  # the cut splits key "a"


class _Pool:
    """Stands in for the engine's buffer pool (Packer.device_bucket) on the CPU."""

    def __init__(self):
        self.made = {}

    def device_bucket(self, tag, shape, dtype, device):
        return self.made.setdefault(tag, torch.zeros(shape, dtype=dtype))


class _FakeSum:
    """Records what the step asks of it; like: "stack" / "folded", the fields of ops.StackSum /
    ops.FoldedSum.  A launch that returns writes mean = 3, the fused model = prev + 1, v_out = v + 1."""

    def __init__(self, like, log, refuse):
        self.n_clients, self.log, self.refuse = 2, log, refuse
        if like == "stack":
            self.stack, self.weights, self.reorder = None, None, False
        else:
            self.acc, self.acc_kind, self.n_cols = None, na.ACC_F32, 0

    def mean(self, nm, denom, **kw):
        self.log.append((nm, denom, kw))
        if self.refuse:
            raise ValueError("refused launch")
        v, v_out, prev = kw.get("v"), kw.get("v_out"), kw.get("prev")
        if v_out is not None:
            v_out.copy_(v + 1)
        if kw["out32"] is not None:
            kw["out32"].copy_(prev + 1) if prev is not None else kw["out32"].fill_(3.0)
        if kw["out64"] is not None and kw["out64"] is not v_out:
            kw["out64"].fill_(3.0)


#: case -> (output mode, what mean() is asked for (buffers by role), the role of the returned tensor)
CASES = {
    "mean64": ("reference", {"out32": None, "out64": "out64"}, "out64"),
    "mean32": ("float32", {"out32": "out32", "out64": None}, "out32"),
    "first_round": ("reference", {"out32": "out32", "out64": "out64"}, "out64"),
    "fused": ("reference", {"out32": "prev_o", "out64": "out64", "op": na.OP_BY_NAME["adagrad"], "prev": "prev", "v": "v",
                            "v_out": "v_o", "beta": 0.9, "eta": 0.5, "tau": 1e-3, "beta2": 0.99}, "out64"),
    "dyn": ("reference", {"out32": None, "out64": "theta_o", "op": na.OP_DYN, "v": "theta", "v_out": "theta_o", "h": "h",
                          "alpha": 0.25}, "theta_o"),
}


def _snapshot(opt):
    from flearn_amd.serverstate import DynState

    if opt is None or not opt.state:
        return None
    return opt.theta_host() if isinstance(opt, DynState) else opt.state_dict()


def _same(got, want):
    if got is None or want is None:
        return got is want
    if "w_glob" in want and isinstance(want["w_glob"], dict):
        return all(_same(got[k], want[k]) for k in want)
    return set(got) == set(want) and all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want)


def _drive(case, like, refuse, monkeypatch):
    """One round of `case` through Aggregator._server_step with fake sums.  Returns per shard
    (nm, denom, the request with buffers named by role, the returned tensor's role), the optimizer
    and its state before the step."""
    from flearn_amd.aggregator import Aggregator
    from flearn_amd.serverstate import DynState, ServerOptimizer

    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())  # CPU shards
    model, plan, shards = _two_cpu_shards()
    agg = object.__new__(Aggregator)  # no HIP library, no device: the step itself needs neither
    agg.output, agg._dist, agg.reorder, agg.packer = CASES[case][0], False, False, _Pool()
    opt, roles = None, [{} for _ in shards]
    if case in ("first_round", "fused"):
        opt = ServerOptimizer("adagrad", eta=0.5, tau=1e-3)
        if case == "fused":
            opt.load_state({"w_glob": model, "v_t": {k: np.abs(x).astype(np.float64) for k, x in model.items()}})
            assert opt.prepare(plan, shards)
            for sh in shards:
                roles[sh.index] = dict(zip(map(id, opt.step_buffers(sh)), ("prev", "v", "prev_o", "v_o")))
    elif case == "dyn":
        opt = DynState({k: x.copy() for k, x in model.items()}, alpha=0.25)
        assert opt.prepare(plan, shards)
        for sh in shards:
            hs, theta = opt.state[sh.index]
            roles[sh.index] = {id(hs): "h", id(theta.cur): "theta", id(theta.other): "theta_o"}
    before = _snapshot(opt)
    log = []
    sums = {KIND_F32: [(sh, _FakeSum(like, log, refuse)) for sh in shards]}
    if refuse:
        with pytest.raises(ValueError, match="refused launch"):
            agg._server_step(plan, sums, opt)
        return log, opt, before, plan
    results = agg._server_step(plan, sums, opt)
    assert list(results) == [KIND_F32] and [sh for sh, _ in results[KIND_F32]] == shards
    seen = []
    for (sh, out), (nm, denom, kw) in zip(results[KIND_F32], log):
        role = roles[sh.index]
        role.update({id(t): tag[0] for tag, t in agg.packer.made.items() if tag[2] == sh.index})
        assert out.numel() == sh.width
        seen.append((nm, denom, {k: role.get(id(v), v) for k, v in kw.items()}, role[id(out)]))
    return seen, opt, before, plan


@pytest.mark.parametrize("case", sorted(CASES))
def test_shared_step_asks_both_kinds_of_sum_for_the_same_thing(case, monkeypatch):
    _, want, returned = CASES[case]
    by_like = {}
    for like in ("stack", "folded"):
        seen, opt, before, plan = _drive(case, like, False, monkeypatch)
        nm = plan.f32.numerics
        assert len(seen) == 2  # one launch per shard
        for nm_, denom, request, out_role in seen:
            assert nm_ is nm and denom == nm.denom
            assert request == want  # the keyword names, and which buffer or value each one got
            assert out_role == returned
        by_like[like] = [s[1:] for s in seen]
        # the launch returned: the state shows what it wrote
        model = _two_cpu_shards()[0]
        after = _snapshot(opt)
        if case == "first_round":  # adopt: prev = the fp32 mean, v_t = 0
            assert _same(after, {"w_glob": {k: np.full_like(x, 3.0) for k, x in model.items()},
                                 "v_t": {k: np.zeros(x.shape) for k, x in model.items()}})
        elif case == "fused":
            assert _same(after, {"w_glob": {k: x + np.float32(1) for k, x in before["w_glob"].items()},
                                 "v_t": {k: x + 1 for k, x in before["v_t"].items()}})
        elif case == "dyn":
            assert _same(after, {k: x + 1 for k, x in before.items()})
    assert by_like["stack"] == by_like["folded"]


@pytest.mark.parametrize("like", ["stack", "folded"])
@pytest.mark.parametrize("case", ["first_round", "fused", "dyn"])
def test_shared_step_leaves_the_state_when_the_launch_is_refused(case, like, monkeypatch):
    log, opt, before, _ = _drive(case, like, True, monkeypatch)
    assert len(log) == 1  # the first shard's launch raised: nothing after it ran
    assert (case == "first_round") == (before is None)
    assert _same(_snapshot(opt), before)


# -- FoldedSum.mean -----------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["avgm", "adagrad", "yogi", "adam", "dyn", "mean"])
def test_folded_sum_builds_the_epilogue_reduce_stack_would(name, monkeypatch):
    from flearn_amd import ops

    n_cols, n_clients = 96, 7
    acc, prev, h, out32 = (torch.zeros(n_cols) for _ in range(4))
    v, v_out, out64 = (torch.zeros(n_cols, dtype=torch.float64) for _ in range(3))
    nm = SimpleNamespace(kind=KIND_F32, mode=na.MODE_W32_DIV64)
    got = []
    monkeypatch.setattr(ops, "fold_finish", lambda *a, **k: got.append((a, k)))
    total = ops.FoldedSum(acc, na.ACC_F32, n_clients, n_cols)
    if name == "mean":
        total.mean(nm, 2.5, out32=out32, out64=out64)
        want = None
    elif name == "dyn":  # as reduce_stack: no prev, FedDyn's N = the clients summed
        total.mean(nm, 2.5, out32=out32, out64=out64, op=na.OP_DYN, v=v, v_out=v_out, h=h, alpha=0.03)
        want = ops._epilogue(na.OP_DYN, None, v, h=h, alpha=0.03, n_dyn=n_clients, v_out=v_out)
    else:
        op, hyper = na.OP_BY_NAME[name], dict(beta=0.8, eta=0.2, tau=1e-4, beta2=0.95)
        total.mean(nm, 2.5, out32=out32, out64=out64, op=op, prev=prev, v=v, v_out=v_out, **hyper)
        want = ops._epilogue(op, prev, v, hyper["beta"], hyper["eta"], hyper["tau"], hyper["beta2"], v_out=v_out)
    ((args, kw),) = got
    assert args == (na.ACC_F32, nm.mode, acc, 2.5, n_cols) and args[2] is acc
    assert set(kw) == {"out32", "out64", "epi"} and kw["out32"] is out32 and kw["out64"] is out64
    if want is None:
        assert kw["epi"] is None
        return
    fields = [f for f, _ in na.Epilogue._fields_]
    assert [getattr(kw["epi"], f) for f in fields] == [getattr(want, f) for f in fields]
    assert kw["epi"].op == (na.OP_DYN if name == "dyn" else na.OP_BY_NAME[name])
    assert kw["epi"].v == v.data_ptr() and kw["epi"].v_out == v_out.data_ptr()
    assert kw["epi"].n_clients == (n_clients if name == "dyn" else 0)
