"""Host-only: the ABI 29 surface and every refusal of fa_sparse_fold_f32 / fa_sparse_workspace (decided before
any HIP call), the top-k rule, sparse.check_round's refusals, the wire round trip and the strategy names."""
import numpy as np
import pytest

import flearn_amd
from flearn_amd import _build
from flearn_amd import _native as na
from flearn_amd import bf16, quant, sparse
from test_cabi import FAKE, header_define

WC = na.SPARSE_WINDOW


def test_abi_surface():
    L = na.load()
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 29
    assert header_define("FA_SPARSE_MAX_CLIENTS") == na.SPARSE_MAX_CLIENTS == 1024 and header_define("FA_SPARSE_WINDOW") == WC
    assert all(f in na.EXPORTS and hasattr(L, f) for f in ("fa_sparse_workspace", "fa_sparse_fold_f32"))
    assert _build.HERE / "csrc" / "fa_sparse.hip" in _build.SOURCES
    assert L.fa_sparse_workspace(3, 2 * WC + 1) == 3 * 4 * 4 and L.fa_sparse_workspace(1, 0) == 16  # int32 [n][windows + 1], up to 16
    for n, cols in ((0, 10), (1025, 10), (1, -1), (1, 2 ** 32)):
        assert L.fa_sparse_workspace(n, cols) == header_define("FA_ERR_ARG") and L.fa_last_error()


OUT, WS = FAKE + 0x100000, FAKE + 0x200000
GOOD = dict(pairs=FAKE, stride=64, n=5, weights=FAKE, center=None, wsum=0.0, acc_in=None, acc_out=OUT, col=0, ncols=3 * WC,
            ws=WS, wsb=5 * 4 * 4)
ARG = [dict(pairs=None), dict(weights=None), dict(acc_out=None), dict(ws=None), dict(n=0), dict(n=1025, wsb=1 << 20), dict(ncols=-1),
       dict(col=-4), dict(stride=-2), dict(acc_in=OUT + 16), dict(acc_in=OUT - 12 * WC + 16), dict(n=0, pairs=FAKE + 4)]
SIZE = [dict(col=2 ** 32), dict(col=2 ** 32 - 4, ncols=4), dict(ncols=2 ** 32, wsb=1 << 40), dict(stride=2 ** 27 + 2), dict(wsb=5 * 4 * 4 - 1),
        dict(wsb=0), dict(ncols=3 * WC + 1)]  # the last: one more window than the workspace holds
ALIGN = [dict(pairs=FAKE + 8), dict(stride=63), dict(col=2), dict(center=FAKE + 4), dict(acc_in=FAKE + 8), dict(acc_out=OUT + 4),
         dict(ws=WS + 8), dict(weights=FAKE + 2)]
OK = [dict(ncols=0), dict(ncols=0, col=2 ** 32 - 1 - 3), dict(ncols=0, stride=0)]


@pytest.mark.parametrize("want,cases", [("FA_ERR_ARG", ARG), ("FA_ERR_SIZE", SIZE), ("FA_ERR_ALIGN", ALIGN), (None, OK)])
def test_sparse_fold_refusals_need_no_gpu(want, cases):
    L, code = na.load(), header_define(want) if want else 0
    for over in cases:
        a = dict(GOOD, **over)
        rc = L.fa_sparse_fold_f32(a["pairs"], a["stride"], a["n"], a["weights"], a["center"], a["wsum"], a["acc_in"], a["acc_out"],
                                  a["col"], a["ncols"], a["ws"], a["wsb"], None)
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0, over
        assert rc == code and (code == 0 or L.fa_last_error()), over


def test_top_k_rule_ties_clamps_and_centre():
    x = np.array([1, -3, 3, 0.5, -3, 2, 3], np.float32)
    e = sparse.sparsify_array(x, k=3)
    assert e["idx"].dtype == np.uint32 and e["idx"].tolist() == [1, 2, 4] and e["val"].tolist() == [-3, 3, -3]  # ties: the lower index
    assert e["val"].dtype == np.float32 and e["shape"] == (7,) and e["delta"] is False
    assert sparse.sparsify_array(x, k=4)["idx"].tolist() == [1, 2, 4, 6] and sparse.sparsify_array(x, k=5)["idx"].tolist() == [1, 2, 4, 5, 6]
    assert [sparse.top_k_count(n, r) for n, r in ((7, 0.01), (1000, 0.01), (1001, 0.01), (5, 1.0), (0, 0.5))] == [1, 10, 11, 5, 0]
    assert sparse.top_k_count(7, k=0) == 0 and sparse.top_k_count(7, k=9) == 7 and sparse.sparsify_array(x, k=0)["idx"].size == 0
    assert sparse.sparsify_array(x.reshape(7, 1), k=99)["idx"].tolist() == list(range(7))
    g = np.array([1, -3, 0, 0, 0, 0, 3], np.float32)
    d = sparse.sparsify_array(x, g, k=2)
    assert d["delta"] is True and d["idx"].tolist() == [2, 4] and d["val"].tolist() == [3, -3]
    assert (sparse.densify_entry(d, g) == np.array([1, -3, 3, 0, -3, 0, 3], np.float32)).all()
    for bad in (dict(ratio=0), dict(ratio=1.5), dict(k=-1), dict(k=1.5), dict(k=True)):
        with pytest.raises(ValueError, match="ratio|k must"):
            sparse.sparsify_array(x, **bad)
    with pytest.raises(ValueError, match="finite"):
        sparse.sparsify_state_dict({"w": np.array([1, np.nan], np.float32)})
    sd = {"w": np.arange(300, dtype=np.float32).reshape(3, 100), "n": np.array(3), "d": np.ones(2)}
    up = sparse.sparsify_state_dict(sd)
    assert sparse.is_sparse(up) and not sparse.is_sparse(sd) and up["w"]["idx"].tolist() == [297, 298, 299] and up["n"] == 3
    assert up["d"].dtype == np.float64 and sparse.entry_shape(up["w"]) == (3, 100)
    assert (sparse.densify_state_dict(up)["w"][2, 97:] == [297, 298, 299]).all()


def entry(**fields):
    return dict(sparse.sparsify_array(np.arange(1, 301, dtype=np.float32), k=4), **fields)


@pytest.mark.parametrize("exc,match,fields", [
    (TypeError, "idx must be uint32", {"idx": np.array([1, 2, 3, 4], np.int64)}), (TypeError, "val must be float32", {"val": np.ones(4)}),
    (ValueError, "one length", {"val": np.ones(3, np.float32)}), (ValueError, ">= the tensor's 300", {"idx": np.array([1, 2, 3, 300], np.uint32)}),
    (ValueError, "strictly ascending", {"idx": np.array([1, 2, 2, 4], np.uint32)}),
    (ValueError, "strictly ascending", {"idx": np.array([1, 3, 2, 4], np.uint32)}), (ValueError, "delta must be a bool", {"delta": 1}),
    (ValueError, "does not match client 0", {"shape": (300, 1)}), (ValueError, "delta=True in a round of delta=False", {"delta": True}),
])
def test_check_round_refusals(exc, match, fields):
    with pytest.raises(exc, match=match):
        sparse.check_round([{"w": entry()}, {"w": entry(**fields)}], ["w"])


def test_check_round_formats_and_the_wire():
    w = np.arange(1, 301, dtype=np.float32)
    good = {"w": entry(), "n": np.array(1)}
    skeys, delta, entries = sparse.check_round([good, good], ["w", "n"])
    assert skeys == ["w"] and delta is False and entries[1]["w"][0].tolist() == [296, 297, 298, 299]
    for other, match in (({"w": w}, "sparse in some uploads"), ({"w": quant.quantize_array(w)}, "one format"),
                         ({"w": bf16.encode_tensor(w)}, "one format")):
        with pytest.raises(ValueError, match=match):
            sparse.check_round([good, dict(good, **other)], ["w", "n"])
    with pytest.raises(ValueError, match="plain fp32"):
        sparse.check_round([dict(good, x=w)] * 2, ["w", "x"])
    enc = flearn_amd.Encrypt()
    back = enc.decode(enc.encode({"agg_weight": 2.0, "params": good}))["params"]
    assert back["w"]["idx"].dtype == np.uint32 and back["w"]["shape"] == (300,) and back["w"]["delta"] is False
    assert (back["w"]["idx"] == good["w"]["idx"]).all() and back["w"]["val"].tobytes() == good["w"]["val"].tobytes()
    assert sparse.check_round([back], ["w", "n"])[0] == ["w"]


def test_strategy_names_and_constructor():
    assert "TopKAVG" in flearn_amd.__all__ and "TopKAVG" in flearn_amd.strategy.__all__
    for bad in (dict(ratio=0), dict(ratio=2), dict(k=-1), dict(error_feedback=None), dict(error_feedback="yes")):
        with pytest.raises(ValueError, match="ratio|k must|error_feedback"):
            flearn_amd.TopKAVG(**bad)
    s = flearn_amd.setup_strategy("avg_topk", None, ratio=0.1, delta=False, error_feedback=False, output="float32", chunk_clients=4)
    assert type(s) is flearn_amd.TopKAVG and (s.ratio, s.k, s.delta, s.error_feedback, s.output, s.chunk_clients) == (0.1, None, False, False, "float32", 4)
    up = s.client(type("Trainer", (), {"weight": {"w": np.arange(40, dtype=np.float32), "n": np.array(2)}})())["params"]
    assert up["w"]["idx"].tolist() == [36, 37, 38, 39] and up["n"] == 2 and not s._residual
