"""flearn_amd.bucket after its split into bucketplan (the plan), packer (the native pack calls and
the Packer) and rowtable (device-resident uploads): every name the single module defined is still
importable from it and is the object of its new home; the fp32 row layout has one producer that
the wire decoder, the packer and a hand-built tuple agree with; and each native table format has
one builder, held here to literal tables and to what the native packs then copy.  No GPU."""
import ast
import base64
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

from flearn_amd import layouts, wire
from flearn_amd.semantics import KIND_F32

#: the names flearn_amd.bucket defined before the split, by new home
MOVED = {
    "flearn_amd.bucketplan": ["ALIGN", "ALIGN_F16", "STRIDE_ALIGN_F16", "SMALL_BYTES", "_STORE", "TORCH_DTYPE", "_NP",
                              "FMT", "Segment", "Group", "BucketPlan", "_as_array_meta", "_raw_signature",
                              "_plain_dicts", "_same_signature_native", "select_keys", "_PLANS", "_PLANS_MAX",
                              "_PLANS_LOCK", "make_plan", "_build_plan", "_same_numerics", "Shard", "rank_width",
                              "split_columns"],
    "flearn_amd.packer": ["AsyncPack", "NativeRows", "Packer"],
    "flearn_amd.rowtable": ["RowTable", "_ROW_SOURCES"],
}


@pytest.mark.parametrize("home", sorted(MOVED))
def test_bucket_still_exports_every_name(home):
    import importlib

    from flearn_amd import bucket

    mod = importlib.import_module(home)
    for name in MOVED[home]:
        assert getattr(bucket, name) is getattr(mod, name), name


def test_underscore_names_tests_and_tools_import():
    from flearn_amd import bucket, packer, rowtable

    assert bucket._NativeRows is packer.NativeRows
    assert bucket.Packer._pieces is packer.Packer._pieces and callable(bucket.Packer._async_rows)
    assert bucket.Packer._slab_stack is rowtable.slab_stack
    assert callable(bucket.Packer.row_table)


def test_plan_module_imports_no_wire():
    """bucketplan (and what it imports of the package) names neither wire nor the modules built on
    it, so wire can import the plan module at module level without a cycle."""
    root = Path(__file__).resolve().parent.parent / "flearn_amd"
    for mod in ("bucketplan", "_native", "semantics"):
        for node in ast.walk(ast.parse((root / f"{mod}.py").read_text())):
            names = []
            if isinstance(node, ast.ImportFrom):
                names = [node.module or ""] + [a.name for a in node.names]
            elif isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            for n in names:
                assert not {"wire", "packer", "rowtable", "bucket", "aggregator", "ops", "serverstate", "smallround",
                            "streaming"} & set(n.split(".")), (mod, n)


def _mixed():
    rng = np.random.default_rng(4)
    return {"w0": rng.random((3, 5), dtype=np.float32), "scalar": np.array(1.5, dtype=np.float32),
            "f64": rng.random(7), "empty": np.zeros((0,), dtype=np.float32),
            "steps": np.array(3, dtype=np.int64), "w1": rng.random(130, dtype=np.float32)}


def _lenet():
    lay = layouts.get("lenet5")
    flat = np.random.default_rng(0).standard_normal(layouts.fp32_elems(lay)).astype(np.float32)
    return layouts.synthetic_state_dict(lay, flat)


@pytest.mark.parametrize("make", [_lenet, _mixed])
def test_row_layout_has_one_source(make):
    """The layout the decoder registers for an upload is the bucket side's producer for the plan
    of that upload, and both are the tuple tests/test_wire.py builds by hand."""
    from flearn_amd.bucket import make_plan

    text = base64.b64encode(pickle.dumps({"agg_weight": 1.0, "params": make()})).decode()
    params = wire.Encrypt(fast_min_chars=0).decode(text)["params"]
    ent = wire._live_entry(params)
    if ent is None:
        pytest.skip("decode did not register a pinned row here (no pinned memory)")
    g = make_plan([1.0], [params]).groups[KIND_F32]
    by_hand = tuple((s.key, s.shape, s.offset) for s in g.segments) + (g.stride,)
    assert ent[1] == g.row_layout == by_hand
    assert ent.layout is ent[1] and wire.wire_row(params, by_hand) is not None


def _cut_case():
    """3 fp32 keys of 5, 64 and 130 elements (offsets 0, 64, 128; stride 320) on 2 shards [0, 192)
    and [192, 320): the third key is cut after 64 elements.  4 clients, client 2 skipped."""
    from flearn_amd.bucket import Packer, Shard, make_plan

    rng = np.random.default_rng(1)
    ups = [{"a": rng.random(5, dtype=np.float32), "b": rng.random(64, dtype=np.float32),
            "c": rng.random(130, dtype=np.float32)} for _ in range(4)]
    plan = make_plan([1.0] * 4, ups)
    g = plan.groups[KIND_F32]
    assert g.stride == 320
    cpu = torch.device("cpu")
    shards = [Shard(0, cpu, 0, 192), Shard(1, cpu, 192, 320)]
    return ups, plan, Packer._pieces(g, shards), shards


def _cut_table(b0, b1):
    """The job table of _cut_case, written out: per packed client its four pieces as (source
    dict, value bytes, format, destination, chunk, first byte, bytes); staging rows are 768 and
    512 bytes."""
    f = ord("f")
    return np.array([row for r in (0, 1, 3) for row in (
        (r, 20, f, b0 + r * 768, 0, 0, 20),
        (r, 256, f, b0 + r * 768 + 256, 0, 0, 256),
        (r, 520, f, b0 + r * 768 + 512, 0, 0, 256),
        (r, 520, f, b1 + r * 512, 0, 256, 264))], dtype=np.int64)


def test_async_job_table_builder_matches_the_literal():
    from flearn_amd.bucket import AsyncPack, Packer

    b0, b1 = 1 << 40, 3 << 40  # fake staging addresses
    r = np.array([0, 1, 3])[:, None]
    table = AsyncPack.table(src=r, value_bytes=[20, 256, 520, 520], fmt=ord("f"),
                            dst=np.array([b0, b0 + 256, b0 + 512, b1]) + r * np.array([768, 768, 768, 512]),
                            chunk=0, first_byte=[0, 0, 0, 256], nbytes=[20, 256, 256, 264])
    assert table.dtype == np.int64 and table.shape == (12, 7)
    assert np.array_equal(table, _cut_table(b0, b1))
    ups, plan, pieces, shards = _cut_case()
    assert [(p.segment.key, p.src_lo, p.src_hi, p.shard.index, p.dst_lo) for p in pieces] == [
        ("a", 0, 5, 0, 0), ("b", 0, 64, 0, 64), ("c", 0, 64, 0, 128), ("c", 64, 130, 1, 0)]
    hosts = [torch.full((4, sh.width), -7.0) for sh in shards]
    aps, bounds = Packer([torch.device("cpu")] * 2)._async_rows(plan, pieces, hosts, [None, None, object(), None])
    assert bounds == [(0, 1), (1, 2), (2, 3), (3, 4)]
    got = np.concatenate([ap.desc.reshape(7, -1).T for ap in aps])
    assert np.array_equal(got, _cut_table(hosts[0].data_ptr(), hosts[1].data_ptr()))
    assert [ap.keys for ap in aps] == [("a", "b", "c", "c"), ("a", "b", "c", "c"), (), ("a", "b", "c", "c")]


def test_small_chain_table_packs_part_k_as_chunk_k():
    """aggregator.chain_table on CPU staging: n = 7 clients in 3 parts (2, 2, 3), two keys; client
    i of part k lands in staging row i + k, the two partial-sum rows stay untouched, and chunk k
    is exactly part k."""
    from flearn_amd.aggregator import chain_table
    from flearn_amd.bucket import AsyncPack, Packer, Shard, make_plan

    n, parts, bounds = 7, 3, [0, 2, 4, 7]
    rng = np.random.default_rng(2)
    ups = [{"w": rng.random((9, 11), dtype=np.float32), "b": rng.random(3, dtype=np.float32)} for _ in range(n)]
    g = make_plan([1.0] * n, ups).groups[KIND_F32]
    pieces = Packer._pieces(g, [Shard(0, torch.device("cpu"), 0, g.stride)])
    stage = np.full((n + parts - 1, g.stride), -7.0, dtype=np.float32)
    table = chain_table(pieces, stage.ctypes.data, g.stride * 4, bounds)
    part_of = np.repeat(np.arange(parts), np.diff(bounds))
    assert table.shape == (n * len(pieces), 7) and np.array_equal(table[:, 4], part_of[table[:, 0]])
    ap = AsyncPack(tuple(p.segment.key for p in pieces) * n, table, parts)
    h = ap.start(ups)
    assert h is not None
    for k in range(parts):
        ap.wait(h, k)
    ap.end(h)
    for i in range(n):
        row = stage[i + part_of[i]]
        for s in g.segments:
            assert np.array_equal(row[s.offset : s.offset + s.numel], ups[i][s.key].reshape(-1)), (i, s.key)
    for r in (2, 5):  # row b_(k+1) + k: where launch k writes its partial sum
        assert (stage[r] == -7.0).all()


def test_pack_rows_descriptor_has_one_builder():
    """_DictPack (the client update) and NativeRows (the server pack), built for the same one-row,
    one-shard layout, hand fa_py_pack_rows the same descriptor up to the trailing skip flags."""
    from flearn_amd.bucket import NativeRows, Packer, Shard, make_plan
    from flearn_amd.strategy._update import DeviceUpdater, _DictPack

    d = {"w": np.arange(70, dtype=np.float32).reshape(7, 10), "s": np.array(2.0, dtype=np.float32),
         "b": np.arange(3, dtype=np.float32)}
    lay, total = DeviceUpdater("avgm")._layout(d)
    g = make_plan([1.0], [d]).groups[KIND_F32]
    assert total == g.stride and [(e.key, e.offset) for e in lay] == [(s.key, s.offset) for s in g.segments]
    # one row has no pitch: _DictPack writes 0 there, and so does a [1, stride] view of row pitch 0
    host = torch.zeros(g.stride).as_strided((1, g.stride), (0, 1))
    pieces = Packer._pieces(g, [Shard(0, torch.device("cpu"), 0, g.stride)])
    nat = NativeRows(pieces, [host], [d], [None])
    (keys, desc), = _DictPack(lay, np.float32, host.data_ptr()).parts
    m = len(keys)
    assert keys == nat.keys and len(desc) == len(nat.desc) == 7 * m + 1
    assert np.array_equal(desc[: 7 * m], nat.desc[: 7 * m])
    assert nat(0, 1) and np.array_equal(host[0, :70].numpy(), d["w"].reshape(-1))
