"""Host-only: the ABI 27 surface and every refusal of fa_deq_fold_q1 (decided before any HIP call), the
1-bit quantizer against tests/quant1_ref.py bit for bit, check_entry's and check_round's 1-bit refusals,
the wire round trip, the "avg_q1" strategy name and the client's error-feedback residual."""
import numpy as np
import pytest

import flearn_amd
import quant1_ref as q1r
from flearn_amd import _build
from flearn_amd import _native as na
from flearn_amd import quant
from test_cabi import FAKE, header_define


def test_abi_surface():
    L = na.load()
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 27
    assert header_define("FA_Q1_BLOCK") == na.Q1_BLOCK == quant.Q1_BLOCK == q1r.BLOCK == 128
    assert header_define("FA_Q1_CHUNK") == na.Q1_CHUNK == q1r.CHUNK == 2048
    assert "fa_deq_fold_q1" in na.EXPORTS and hasattr(L, "fa_deq_fold_q1")
    assert _build.HERE / "csrc" / "fa_quant1.hip" in _build.SOURCES


OUT = FAKE + 0x10000
GOOD = dict(stack=FAKE, stride=512, n=5, scales=FAKE, sstride=32, weights=FAKE, center=None, acc_in=None, acc_out=OUT,
            col=0, ncols=4096)  # a row of 512 bytes holds 4096 columns: 32 scale blocks
ARG = [dict(stack=None), dict(scales=None), dict(weights=None), dict(acc_out=None), dict(n=0), dict(n=-1), dict(ncols=-1),
       dict(col=-2048), dict(col=2048, ncols=4096), dict(col=6144, ncols=0), dict(ncols=4097), dict(stride=-16),
       dict(col=2**63 - 2047, ncols=4096), dict(ncols=2**63 - 1), dict(sstride=31), dict(sstride=0),
       dict(col=2048, ncols=129, sstride=17), dict(acc_in=OUT + 16), dict(acc_in=OUT + 4 * 4096 - 16),
       dict(acc_in=OUT - 4 * 4096 + 16), dict(n=0, stack=FAKE + 4)]  # the last: an argument error wins over alignment
ALIGN = [dict(stack=FAKE + 4), dict(stack=FAKE + 1), dict(stride=512 + 8), dict(col=128, ncols=1), dict(center=FAKE + 4),
         dict(acc_out=OUT + 8), dict(acc_in=FAKE + 4), dict(scales=FAKE + 2), dict(weights=FAKE + 1), dict(col=1024, ncols=16)]
OK = [dict(ncols=0), dict(col=4096, ncols=0), dict(ncols=0, sstride=0), dict(ncols=0, scales=FAKE + 4, weights=FAKE + 4)]


@pytest.mark.parametrize("want,cases", [("FA_ERR_ARG", ARG), ("FA_ERR_ALIGN", ALIGN), (None, OK)])
def test_deq_fold_q1_refusals_need_no_gpu(want, cases):
    L, code = na.load(), header_define(want) if want else 0
    for over in cases:
        a = dict(GOOD, **over)
        rc = L.fa_deq_fold_q1(a["stack"], a["stride"], a["n"], a["scales"], a["sstride"], a["weights"], a["center"],
                              a["acc_in"], a["acc_out"], a["col"], a["ncols"], None)
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0, over
        assert rc == code and (code == 0 or L.fa_last_error()), over
    assert want != "FA_ERR_ALIGN" or b"2048" in L.fa_last_error()  # the last case: col_begin's unit is named


@pytest.mark.parametrize("n", [1, 7, 8, 127, 128, 129, 300])
def test_quantizer_round_trip(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    x[:: 5] = (0.0, -0.0)[n % 2]  # zeros of both signs take the non-negative code
    g = rng.standard_normal(n).astype(np.float32)
    for center in (None, g):
        e = quant.quantize_array(x.reshape(-1, 1), center, bits=1)
        q1, scales = q1r.quantize(x, center)
        assert set(e) == {"q1", "shape", "scale", "block", "delta"} and e["block"] == 128 and e["delta"] is (center is not None)
        assert e["shape"] == (n, 1) and e["q1"].dtype == np.uint8 and e["q1"].shape == ((n + 7) // 8,) and (e["q1"] == q1).all()
        assert e["scale"].dtype == np.float32 and q1r.same_bits(e["scale"], scales)
        u = x if center is None else x - g
        assert (q1r.unpack(e["q1"], 8 * len(q1)) == np.concatenate([u < 0, np.zeros(8 * len(q1) - n, bool)])).all()
        back = quant.dequantize_entry(e, center).reshape(-1)
        assert q1r.same_bits(back, q1r.dequantize(e["q1"], n, e["scale"], center))
        assert center is not None or (np.signbit(back) == (x < 0)).all()
    z = quant.quantize_array(np.concatenate([np.zeros(128, np.float32), x]), bits=1)
    assert z["scale"][0] == 0 and not z["q1"][:16].any()  # an all-zero block


def entry(**fields):
    e = quant.quantize_array(np.random.default_rng(2).standard_normal(300).astype(np.float32), bits=1)
    if "scale1" in fields:
        e["scale"][1] = fields.pop("scale1")
    return dict(e, **fields)


@pytest.mark.parametrize("exc,match,fields", [
    *[(ValueError, "finite and >= 0", {"scale1": v}) for v in (-1.0, np.nan, np.inf)],
    (ValueError, "need 38 code bytes", {"q1": np.zeros(37, np.uint8)}), (ValueError, "need 3 scales", {"scale": np.ones(2, np.float32)}),
    (TypeError, "q1 must be uint8", {"q1": np.zeros(38, np.int8)}), (ValueError, "block must be 128", {"block": 1024}),
    (ValueError, "shape", {"shape": 300}), (ValueError, "one width", {"q4": np.zeros(150, np.uint8)}),
])
def test_check_entry_and_check_round_refusals(exc, match, fields):
    bad = entry(**fields)
    with pytest.raises(exc, match=match):
        quant.check_entry("w", bad)
    with pytest.raises(exc, match=match):
        quant.check_round([{"w": entry()}, {"w": bad}], ["w"])


def test_legal_scales_stochastic_and_the_round_s_width():
    assert all(quant.check_entry("w", entry(scale1=ok)) for ok in (0.0, -0.0, 1e-45, 1.0, 2.0 ** 127))
    sd = {"w": np.ones((3, 50), np.float32), "b": np.ones(7, np.float32), "n": np.array(3)}
    for f in (quant.quantize_array, quant.quantize_state_dict):
        with pytest.raises(ValueError, match="stochastic"):
            f(sd["w"] if f is quant.quantize_array else sd, stochastic=True, rng=np.random.default_rng(0), bits=1)
    with pytest.raises(ValueError, match="finite"):
        quant.quantize_array(np.array([1.0, np.nan], np.float32), bits=1)
    u1, u4, u8 = (quant.quantize_state_dict(sd, bits=b) for b in (1, 4, 8))
    assert quant.is_quantized(u1) and quant.bits_of(u1["w"]) == 1 and quant.entry_shape(u1["w"]) == (3, 50)
    assert quant.check_round([u1, u1], list(sd))[::4] == (["w", "b"], 1)
    for mixed in ([u1, u8], [u4, u1], [dict(u1, b=u4["b"])] * 2):  # across clients, across keys
        with pytest.raises(ValueError, match="one width"):
            quant.check_round(mixed, list(sd))


def test_wire_round_trip():
    rng = np.random.default_rng(9)
    sd = {"w": rng.standard_normal((41, 7)).astype(np.float32), "n": np.array(3)}
    up = {"agg_weight": 0.25, "params": quant.quantize_state_dict(sd, bits=1)}
    enc = flearn_amd.Encrypt()
    r, v = enc.decode(enc.encode(up))["params"]["w"], up["params"]["w"]
    assert type(r) is dict and set(r) == set(v) and r["block"] == 128 and r["delta"] is False and r["shape"] == (41, 7)
    assert r["q1"].dtype == np.uint8 and (r["q1"] == v["q1"]).all() and q1r.same_bits(np.asarray(r["scale"]), v["scale"])
    assert q1r.same_bits(quant.dequantize_entry(r), quant.dequantize_entry(v))


def test_strategy_name_and_error_feedback_residual():
    s = flearn_amd.setup_strategy("avg_q1", None, delta=False, output="float32", chunk_clients=4)
    assert type(s) is flearn_amd.QuantizedAVG and (s.bits, s.delta, s.error_feedback, s.output, s.chunk_clients) == (1, False, True, "float32", 4)
    assert flearn_amd.QuantizedAVG(bits=1, error_feedback=False).error_feedback is False and not flearn_amd.QuantizedAVG().error_feedback
    for kw in (dict(bits=4, error_feedback=True), dict(bits=8, error_feedback=True), dict(bits=1, stochastic=True),
               dict(bits=1, error_feedback="yes")):
        with pytest.raises(ValueError, match="error_feedback|stochastic"):
            flearn_amd.QuantizedAVG(**kw)
    rng = np.random.default_rng(5)
    e = np.zeros(300, np.float32)
    for _ in range(2):  # the second upload quantizes x + e
        x = rng.standard_normal(300).astype(np.float32)
        up = s.client(type("Trainer", (), {"weight": {"w": x, "n": np.array(2)}})())["params"]
        u = x + e
        q1, scales = q1r.quantize(u)
        assert (up["w"]["q1"] == q1).all() and q1r.same_bits(up["w"]["scale"], scales) and up["n"] == 2
        e = u - q1r.dequantize(q1, 300, scales)
        assert e.any() and q1r.same_bits(s._residual["w"], e)
