"""Host-only: the streamed round's geometry (plan_fold_window, flearn_amd/csrc/fa_geometry.hpp), its
numerics rule (the sum type per chunk, the divide from the whole weight list) and its chunk plans
(flearn_amd/streaming.py).  No GPU: tests/fold_geometry_probe.cpp is compiled against the geometry
header alone, and a RoundAccumulator that never reaches a full chunk touches no device."""
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from flearn_amd import _native as na
from flearn_amd.bucketplan import make_plan
from flearn_amd.semantics import resolve
from flearn_amd.streaming import RoundAccumulator, acc_kind_of
from test_host import WEIGHT_SETS

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
CUS = (256, 304, 64)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fold_geometry") / "fold_geometry_probe"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "fold_geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(queries)
        names = ("family", "V", "W", "D", "grid", "chunks", "rounds", "piece_chunks", "pieces")
        return [dict(zip(names, [f.split()[0]] + [int(x) for x in f.split()[1:]])) for f in out]

    return ask


def widths(cus):
    grid = int(cus * 0.75 + 0.5)
    return [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, grid * 256 + 1, 208 * 16384 + 5,
            grid * 16384 + 1, (cus * 13 // 16) * 16384, (cus * 13 // 16) * 16384 + 1, 25_610_152, 86_567_656]


@pytest.mark.parametrize("kind", [na.ACC_F32, na.ACC_F32_W64])
@pytest.mark.parametrize("cus", CUS)
def test_fold_rows_geometry(cus, kind, probe):
    ws = widths(cus)
    for ncols, p in zip(ws, probe([f"{kind} {n} {cus} 0" for n in ws])):
        assert p["family"] == "fold_rows"
        chunks = (-(-ncols // 4) + 63) // 64
        assert p["chunks"] == chunks
        # the register budget of the fp32 families: 64 KiB of client rows in flight per block
        assert p["V"] * p["W"] * p["D"] == 64 and p["W"] == 4 and p["V"] in (1, 2, 4, 8, 16)
        # no piece wider than the lanes' slots, i.e. than 64 KiB of a row
        assert 1 <= p["piece_chunks"] <= p["V"] * p["W"] <= 64
        # the pieces cover every 1-KiB chunk exactly once: piece i is chunks [i * pc, (i + 1) * pc)
        # cut at the window's end, the last piece not empty, and block b takes pieces b, b + grid, ...
        pc, pieces, grid = p["piece_chunks"], p["pieces"], p["grid"]
        assert (pieces - 1) * pc < chunks <= pieces * pc
        owned = [len(range(b, pieces, grid)) for b in range(min(grid, 4))] + [len(range(grid - 1, pieces, grid))]
        assert sum(len(range(b, pieces, grid)) for b in range(grid)) == pieces
        assert max(owned) <= p["rounds"] and pieces > (p["rounds"] - 1) * grid
        # the grid: at most one block per chunk, ~0.75 blocks per CU, up to 13/16 of the CUs for a
        # window just past one round of full pieces
        assert 1 <= grid <= min(chunks, cus * 13 // 16)
        if chunks >= int(cus * 0.75 + 0.5):
            assert grid >= int(cus * 0.75 + 0.5)
        # the narrowest piece that covers the share
        share = -(-chunks // grid)
        assert p["V"] == 16 or (p["V"] * 4 >= share and (p["V"] == 1 or p["V"] * 2 < share))


def test_fold_rows_geometry_pins(probe):
    """Literals at 256 CUs: narrow windows are 16 rows deep; the flagship width runs 9 rounds of
    58-chunk pieces on 192 blocks; one round + 1 chunk takes 193 blocks instead of a second round."""
    got = probe([f"0 {n} 256 0" for n in (5, 192 * 1024, 192 * 16384 + 1, 208 * 16384 + 5, 25_610_152)] + ["1 5 256 7",
                                                                                                        "0 1000000 256 7"])
    assert [(p["V"], p["D"], p["grid"], p["rounds"], p["piece_chunks"]) for p in got] == [
        (1, 16, 1, 1, 1), (1, 16, 192, 1, 4), (16, 1, 193, 1, 64), (16, 1, 192, 2, 35), (16, 1, 192, 9, 58),
        (1, 16, 1, 1, 1), (16, 1, 7, 9, 63)]  # 3907 chunks: ceil(3907 / 448) rounds, ceil(3907 / 63) chunks


@pytest.mark.parametrize("cus", CUS)
def test_fold_elem_geometry(cus, probe):
    ws = [1, 255, 256, 257, 100_003, 10_000_000]
    for kind in (na.ACC_F64, na.ACC_I64):
        for ncols, p in zip(ws, probe([f"{kind} {n} {cus} 0" for n in ws])):
            assert p["family"] == "fold_elem"
            assert p["grid"] == min(-(-ncols // 256), 4 * cus)  # grid-stride: every column is some lane's
    assert probe([f"{na.ACC_F64} 10000000 {cus} 5"])[0]["grid"] == 5  # fa_set_reduce_grid applies


# ---------------------------------------------------------------------------------------------
# the streaming numerics rule
# ---------------------------------------------------------------------------------------------


def host_round(chunk_clients=1000, key_lst=None):
    """A RoundAccumulator over a stand-in engine: nothing here reaches a device as long as no chunk fills."""
    agg = SimpleNamespace(_dist=False, devices=[torch.device("cpu")])
    return RoundAccumulator(agg, key_lst, None, chunk_clients)


def uploads(ws, xdtype):
    return [{"agg_weight": w, "params": {"a": np.full((3, 5), i + 1, xdtype), "b": np.arange(70, dtype=xdtype)}}
            for i, w in enumerate(ws)]


@pytest.mark.parametrize("wname", sorted(WEIGHT_SETS))
@pytest.mark.parametrize("xdtype", [np.float32, np.float64, np.int64])
def test_chunk_sum_type_and_finish_numerics_are_the_whole_lists(wname, xdtype):
    ws = WEIGHT_SETS[wname]
    ups = uploads(ws, xdtype)
    acc = host_round()
    if len({np.result_type(w, xdtype) for w in ws}) > 1:  # mixed promotion: at the first offending add
        first_bad = next(i for i, w in enumerate(ws) if np.result_type(w, xdtype) != np.result_type(ws[0], xdtype))
        for u in ups[:first_bad]:
            acc.add(u)
        with pytest.raises(TypeError, match="promote differently"):
            acc.add(ups[first_bad])
        return
    if np.result_type(ws[0], xdtype) == np.float16:
        pytest.fail("no weight set promotes these dtypes to float16")
    for u in ups:
        acc.add(u)
    whole = resolve(ws, xdtype)
    assert acc._acc_dtype == {np.dtype(xdtype): whole.acc_dtype}
    fin = acc.numerics(xdtype)
    assert (fin.kind, fin.mode, fin.denom, fin.out_dtype, fin.acc_dtype) == (whole.kind, whole.mode, whole.denom,
                                                                              whole.out_dtype, whole.acc_dtype)
    assert fin.denom == float(np.sum(ws))
    # every chunking: the chunk's plan sums in the whole list's type, with the weights numpy's cast gives
    for k in (1, 2, 3):
        acc = host_round()
        for lo in range(0, len(ws), k):
            plan = acc.chunk_plan(ws[lo : lo + k], [u["params"] for u in ups[lo : lo + k]])
            (g,) = plan.groups.values()
            assert g.kind == whole.kind and g.numerics.acc_dtype == whole.acc_dtype
            assert acc_kind_of(g.kind, g.numerics.mode) == acc_kind_of(whole.kind, whole.mode)
            assert g.numerics.weights.tobytes() == whole.weights[lo : lo + k].tobytes()


def test_np16_weights_follow_resolve():
    """np.float16 weights promote like any strong float16: fp32 tensors stay fp32 (a float32 result)."""
    ws = WEIGHT_SETS["np16"]
    assert resolve(ws, np.float32).mode == na.MODE_W32_DIV32


def test_chunk_plans_have_the_whole_lists_layout():
    """Chunk bounds, and the layout taken from the first upload: every chunk's plan has the keys,
    offsets and strides of make_plan on the whole list; extra keys of later uploads are ignored."""
    rng = np.random.default_rng(0)
    shapes = {"conv.weight": (6, 1, 5, 5), "conv.bias": (6,), "bn.running_mean": (6,), "bn.num_batches_tracked": (),
              "fc.weight": (10, 84)}
    dts = {"bn.num_batches_tracked": np.int64}

    def client(extra=False):
        d = {k: rng.standard_normal(s).astype(dts.get(k, np.float32)) if k not in dts else np.int64(7) * np.ones(s, np.int64)
             for k, s in shapes.items()}
        if extra:
            d["extra"] = np.zeros(3, np.float32)
        return d

    n, k = 7, 3
    ws = [float(i + 1) for i in range(n)]
    ps = [client(extra=i in (2, 5)) for i in range(n)]
    whole = make_plan(ws, [{key: p[key] for key in shapes} for p in ps])
    acc = host_round(chunk_clients=1000)
    bounds = []
    for lo in range(0, n, k):
        plan = acc.chunk_plan(ws[lo : lo + k], ps[lo : lo + k]) if lo else None
        if lo == 0:
            for w, p in zip(ws[:k], ps[:k]):
                acc.add({"agg_weight": w, "params": p})
            plan = acc.chunk_plan(ws[:k], ps[:k])
        bounds.append((lo, lo + plan.n_clients))
        assert plan.keys == whole.keys == list(shapes)
        assert set(plan.groups) == set(whole.groups)
        for kind, g in plan.groups.items():
            assert g.stride == whole.groups[kind].stride
            assert [(s.key, s.shape, s.offset) for s in g.segments] == [(s.key, s.shape, s.offset)
                                                                        for s in whole.groups[kind].segments]
    assert bounds == [(0, 3), (3, 6), (6, 7)]


def test_later_uploads_must_match_the_first():
    base = uploads([1.0, 1.0, 1.0], np.float32)
    acc = host_round()
    acc.add(base[0])
    with pytest.raises(KeyError):
        acc.add({"agg_weight": 1.0, "params": {"a": base[1]["params"]["a"]}})
    with pytest.raises(ValueError, match="does not match client 0"):
        acc.add({"agg_weight": 1.0, "params": {"a": np.zeros((5, 3), np.float32), "b": base[1]["params"]["b"]}})
    with pytest.raises(ValueError, match="does not match client 0"):
        acc.add({"agg_weight": 1.0, "params": {"a": base[1]["params"]["a"].astype(np.float64), "b": base[1]["params"]["b"]}})
    with pytest.raises(TypeError, match="promote differently"):
        acc.add({"agg_weight": np.float64(1.0), "params": base[1]["params"]})
    with pytest.raises(TypeError):
        acc.add({"agg_weight": "1", "params": base[1]["params"]})
    acc.add(base[1])  # a refused upload left the round as it was
    assert acc._weights == [1.0, 1.0]


def test_refusals_before_anything_is_queued():
    with pytest.raises(TypeError, match="float16"):
        host_round().add({"agg_weight": 1.0, "params": {"a": np.zeros(4, np.float16)}})
    two = SimpleNamespace(_dist=False, devices=[torch.device("cpu"), torch.device("cpu")])
    with pytest.raises(ValueError, match="devices"):
        RoundAccumulator(two, None, None, 4)
    with pytest.raises(ValueError, match="group"):
        RoundAccumulator(SimpleNamespace(_dist=True, devices=[torch.device("cpu")]), None, None, 4)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="chunk_clients"):
            host_round(chunk_clients=bad)
    with pytest.raises(IndexError):  # what ensemble([], []) raises
        host_round().finish()
    acc = host_round()
    with pytest.raises(IndexError):
        acc.finish()
    with pytest.raises(RuntimeError, match="after finish"):
        acc.add({"agg_weight": 1.0, "params": {"a": np.zeros(4, np.float32)}})


def test_strategies_take_chunk_clients_and_default_to_none():
    import flearn_amd as fa

    for make in (fa.AVG, fa.BN, fa.Prox, fa.SGD, lambda **k: fa.LG(["a"], **k), lambda **k: fa.LG_R(["a"], **k),
                 lambda **k: fa.AVGM(server_side=True, **k), lambda **k: fa.OPT(server_side=True, **k),
                 lambda **k: fa.Dyn({"a": np.zeros(3, np.float32)}, **k)):
        assert make().chunk_clients is None
        assert make(chunk_clients=5).chunk_clients == 5
    assert fa.setup_strategy("avg", None, chunk_clients=5).chunk_clients == 5
    assert fa.setup_strategy("lg", None, shared_key_layers=["a"]).chunk_clients is None
