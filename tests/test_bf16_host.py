"""Host-only: the ABI 26 surface and every refusal of fa_fold_bf16 (decided before any HIP call),
flearn_amd/bf16.py's encoder against CPU torch's own rounding, and the refusals of bf16.check_round,
Aggregator.ensemble_bf16 and the BF16AVG strategy, raised before the engine touches a device.  No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import flearn_amd
from flearn_amd import _build
from flearn_amd import _native as na
from flearn_amd import bf16, bf16round
from test_quant_host import bare_engine, header_define  # an engine without a device; a #define of the C header

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "flearn_amd.h"
FAKE = 0x100000  # never dereferenced: validation rejects the call first


def test_abi_surface():
    L = na.load()
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 26
    out = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    assert "fa_fold_bf16" in na.EXPORTS and hasattr(L, "fa_fold_bf16") and re.search(r"\bT\s+fa_fold_bf16$", out, flags=re.M)
    assert re.search(r"\bint\s+fa_fold_bf16\s*\(\s*const\s+uint16_t\s*\*", HEADER.read_text())
    assert REPO / "flearn_amd" / "csrc" / "fa_bf16.hip" in _build.SOURCES


def test_fold_bf16_refusals_need_no_gpu():
    L = na.load()
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")
    out = FAKE + 0x10000

    def call(stack=FAKE, stride=4096, n=5, weights=FAKE, acc_in=None, acc_out=out, col=0, ncols=4096):
        rc = L.fa_fold_bf16(stack, stride, n, weights, acc_in, acc_out, col, ncols, None)
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0
        return rc

    for null in ("stack", "weights", "acc_out"):
        assert call(**{null: None}) == arg and b"null" in L.fa_last_error()
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error() and call(n=-(2**31)) == arg
    assert call(ncols=-1) == arg and b"window" in L.fa_last_error()
    assert call(col=-8) == arg and call(col=8, ncols=4096) == arg and call(col=8192, ncols=0) == arg
    big = 2**63 - 1  # sums of these would overflow: the window check must not form them
    assert call(col=big - 7, ncols=16) == arg and call(ncols=big) == arg
    assert call(acc_in=out + 16) == arg and b"overlap" in L.fa_last_error()
    assert call(n=0, stack=FAKE + 4) == arg  # an argument error wins over an alignment error
    for bad in (dict(stack=FAKE + 2), dict(stack=FAKE + 8), dict(stride=4100), dict(col=4, ncols=8), dict(col=513, ncols=1),
                dict(acc_out=out + 8), dict(acc_in=FAKE + 4), dict(weights=FAKE + 2)):
        assert call(**bad) == align and L.fa_last_error(), bad
    assert call(ncols=0) == 0 and call(col=4096, ncols=0) == 0 and call(ncols=0, weights=FAKE + 4) == 0


def edge_values():
    """fp32 around every rounding case: random, ties both ways, subnormals, values that round up to inf, +-inf, +-0"""
    rng = np.random.default_rng(3)
    bits = np.concatenate([rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32),
                           np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x00000001, 0x00008000, 0x00018000,
                                     0x807FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                                     0x00000000, 0x80000000], dtype=np.uint32)])
    x = bits.view(np.float32)
    return x[~np.isnan(x)]


def test_encode_is_torch_s_rounding_and_decode_is_exact():
    x = edge_values()
    want = torch.from_numpy(x).to(torch.bfloat16)
    e = bf16.encode_state_dict({"w": x.reshape(-1, 2), "n": np.array(3), "d": np.ones(2)})
    assert bf16.is_entry(e["w"]) and bf16.is_bf16(e["w"]) and not bf16.is_bf16(e["n"]) and e["d"].dtype == np.float64
    assert e["w"]["shape"] == (x.size // 2, 2) and e["w"]["bf16"].dtype == np.uint16
    assert (e["w"]["bf16"].reshape(-1).view(np.int16) == want.view(torch.int16).numpy()).all()
    assert np.isinf(bf16.decode(e["w"])).sum() > np.isinf(x).sum()  # values that round up to inf are among them
    assert bf16.decode(e["w"]).tobytes() == want.to(torch.float32).numpy().reshape(-1, 2).tobytes()
    nan = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    assert np.isnan(bf16.decode(bf16.encode_tensor(nan))).all() and np.isnan(bf16.widen(bf16.round_f32(nan, True, np.random.default_rng(0)))).all()
    t = want.reshape(-1, 2)  # a bfloat16 tensor: lossless both ways
    back = bf16.encode_state_dict({"w": t})["w"]
    assert (back["bf16"].view(np.int16) == t.view(torch.int16).numpy()).all() and back["shape"] == tuple(t.shape)
    assert bf16.decode(t).tobytes() == t.to(torch.float32).numpy().tobytes()


def test_stochastic_rounding_picks_a_neighbour_and_repeats_from_its_seed():
    x = edge_values()
    x = x[np.isfinite(x)]
    a = bf16.round_f32(x, True, np.random.default_rng(7))
    assert (a == bf16.round_f32(x, True, np.random.default_rng(7))).all()
    down = (x.view(np.uint32) >> 16).astype(np.uint16)  # truncation: the neighbour towards zero
    exact = (x.view(np.uint32) & 0xFFFF) == 0
    assert ((a == down) | (a == down + 1)).all() and (a[exact] == down[exact]).all() and (a != down).any()


def uploads(n=4):
    rng = np.random.default_rng(2)
    return [bf16.encode_state_dict({"w": rng.standard_normal((30, 5)).astype(np.float32), "b": torch.randn(5).bfloat16(),
                                    "n": np.array(i, dtype=np.int64)}) for i in range(n)]


def test_check_round_and_engine_refusals_touch_no_device():
    from flearn_amd.aggregator import Aggregator
    from flearn_amd.serverstate import DynState

    assert Aggregator.ensemble_bf16 is bf16round.ensemble_bf16 and Aggregator.last_bf16 is None
    ups, w = uploads(), [1.0] * 4
    bkeys, rows = bf16.check_round(ups, ["w", "b", "n"])
    assert bkeys == ["w", "b"] and rows[2]["w"].shape == (150,) and rows[2]["w"].dtype == np.uint16

    def refused(exc, match, ups=ups, w=w, agg=None, **kw):
        with pytest.raises(exc, match=match):
            (agg or bare_engine()).ensemble_bf16(w, ups, **kw)

    def with_key(i, key, v):
        return [dict(u, **{key: v}) if j == i else u for j, u in enumerate(ups)]

    refused(ValueError, "group", agg=bare_engine(_dist=True))
    refused(ValueError, "one device", agg=bare_engine(devices=[torch.device("cpu")] * 2))
    refused(TypeError, "Dyn", server_opt=object.__new__(DynState))
    refused(ValueError, "chunk_clients", agg=bare_engine(chunk_clients=0))
    refused(ValueError, "some uploads", with_key(2, "w", np.zeros((30, 5), np.float32)))
    refused(ValueError, "does not match client 0", with_key(3, "w", {"bf16": np.zeros(150, np.uint16), "shape": (150,)}))
    refused(ValueError, "plain fp32", [dict(u, extra=np.zeros(3, np.float32)) for u in ups])
    refused(TypeError, "float16", [dict(u, extra=np.zeros(3, np.float16)) for u in ups])
    refused(TypeError, "uint16", with_key(1, "w", {"bf16": np.zeros((30, 5), np.int16), "shape": (30, 5)}))
    refused(ValueError, "shape", with_key(1, "w", {"bf16": np.zeros(150, np.uint16), "shape": (30, 4)}))
    for w64 in ([np.float64(1.0)] * 4, [np.int64(2)] * 4):
        refused(TypeError, "float64", w=w64)
    with pytest.raises(AssertionError, match="touched its packer"):  # a good round gets as far as the pack
        bare_engine(chunk_clients=3).ensemble_bf16(w, ups)
    with pytest.raises(TypeError):  # unchanged: the plain round refuses bfloat16 tensors
        bare_engine().ensemble(w, [{"b": u["b"]} for u in ups])


def test_strategy_surface_and_server_exception_route():
    from flearn_amd.strategy import AVG, BF16AVG

    s = flearn_amd.setup_strategy("AVG_BF16", None, stochastic=True, seed=3, output="float32", chunk_clients=4)
    assert type(s) is flearn_amd.BF16AVG and issubclass(BF16AVG, AVG) and (s.stochastic, s.seed, s.chunk_clients) == (True, 3, 4)
    trainer = type("T", (), {"weight": {"w": torch.tensor([1.0, 1.00390625, -3.0]), "n": torch.tensor(3)}})
    up = BF16AVG().client(trainer, 2.0)
    assert up["agg_weight"] == 2.0 and up["params"]["w"]["bf16"].tolist() == [0x3F80, 0x3F80, 0xC040] and up["params"]["n"] == 3
    s._engine = bare_engine()
    with pytest.raises(SystemExit):  # a client-data error takes server_exception's route
        s.server([{"agg_weight": 1.0, "params": dict(u, w=np.zeros((30, 5), np.float32)) if i == 1 else u}
                  for i, u in enumerate(uploads())], 0)
