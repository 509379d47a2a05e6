"""flearn_amd.dist after its split into shardplan (the planner), push (the one-shot push
transport) and dist (collectives, double-buffered state, the reducer): every name the single
module had is still importable from it and is the object of its new home; `ShardedReducer.step`
still finds `all_gather_into` as a global of flearn_amd.dist (what bench.py's fault injections
assign); and the planner returns the plans it returned before the split, tuple for tuple."""
import json
import os
import tempfile
from pathlib import Path

import pytest
import torch
import torch.distributed as dist

#: the names of flearn_amd.dist before the split (standard-library imports left out), by new home
MOVED = {
    "flearn_amd.shardplan": ["ALIGN", "CONTENTION_PRIOR", "REP_FRACTIONS", "ShardPlan", "StripeModel", "plan_shards",
                             "plan_stripes", "shard_candidates"],
    "flearn_amd.push": ["DeviceBuffer", "HipIpc", "MAX_PUSH_RANKS", "PARK_CAP", "PushGather", "_IPC", "_LARGEST",
                        "_PARKED", "_PUSH_ORDER", "_RecvPool", "_TRIMMED", "_all_ok", "_group_alive", "_map_peers",
                        "_resolve_group", "_unmap_all", "peer_stream", "push_order", "shutdown_push", "size_class"],
    "flearn_amd.streams": ["side_stream"],
    "flearn_amd.dist": ["DoubleBuffer", "PingPong", "ShardedReducer", "_host_staged", "all_gather_into",
                        "gather_columns", "hip_reduce_fn"],
}


@pytest.mark.parametrize("home", sorted(MOVED))
def test_dist_still_exports_every_name(home):
    import importlib

    from flearn_amd import dist as fa_dist

    mod = importlib.import_module(home)
    for name in MOVED[home]:
        assert getattr(fa_dist, name) is getattr(mod, name), name
        if home == "flearn_amd.dist":
            assert getattr(fa_dist, name).__module__ == home, name


def test_shardplan_imports_no_torch():
    src = (Path(__file__).resolve().parent.parent / "flearn_amd" / "shardplan.py").read_text()
    assert "torch" not in src.split('"""', 2)[2]


def test_step_resolves_all_gather_into_in_dist(monkeypatch):
    from flearn_amd import dist as fa_dist

    init = "file://" + os.path.join(tempfile.mkdtemp(prefix="fa_inject_"), "pg")
    dist.init_process_group("gloo", init_method=init, rank=0, world_size=1)
    try:
        plan = fa_dist.ShardPlan.make(256, 1, 0, stripes=2)
        data = torch.arange(plan.local_cols, dtype=torch.float32)

        def reduce_fn(col_begin, n_cols, out_slice):
            out_slice.copy_(data[col_begin : col_begin + n_cols])

        real, calls = fa_dist.all_gather_into, []

        def counting(dst, src, group=None, async_op=False):
            calls.append(src.numel())
            return real(dst, src, group=group, async_op=async_op)

        monkeypatch.setattr(fa_dist, "all_gather_into", counting)  # assigned, as bench.py's injections do
        red = fa_dist.ShardedReducer(plan, reduce_fn, "cpu", gather=True)
        full = red.step()
        assert calls == [plan.shard_of(c) for c in range(plan.stripes)] and len(calls) == 2
        assert torch.equal(full, data[:256])
    finally:
        dist.destroy_process_group()


def _cases():
    doc = json.loads((Path(__file__).resolve().parent / "golden" / "shardplan_cases.json").read_text())
    return doc["n_clients"], doc["cases"]


def test_planner_returns_the_recorded_plans():
    from flearn_amd.shardplan import CONTENTION_PRIOR, StripeModel, plan_shards, plan_stripes, shard_candidates

    n_clients, cases = _cases()
    assert {(c["n_cols"], c["world"], c["contended"]) for c in cases} == {
        (n, w, k) for n in (64, 4097, 365_000, 25_600_000) for w in (1, 2, 3, 8) for k in (False, True)}
    for c in cases:
        n_cols, world = c["n_cols"], c["world"]
        model = StripeModel.assumed(n_clients, world)
        if c["contended"]:
            model = model.with_contention(*CONTENTION_PRIOR)
        assert plan_stripes(c["local_cols"], model) == tuple(c["plan_stripes"]), c
        assert plan_shards(n_cols, world, model) == (tuple(c["plan_shards"][0]), c["plan_shards"][1]), c
        assert shard_candidates(n_cols, world, model) == [(tuple(w), rep) for w, rep in c["shard_candidates"]], c
