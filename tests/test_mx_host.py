"""Host-only: the ABI 28 surface and every refusal of fa_deq_fold_mx (decided before any HIP call), the
Microscaling quantizer against tests/mx_ref.py's float64 restatement, check_entry's and check_round's
refusals, the strategy names and the format keyword."""
import numpy as np
import pytest

import flearn_amd
import mx_ref as mxr
from flearn_amd import _build
from flearn_amd import _native as na
from flearn_amd import quant
from test_cabi import FAKE, header_define


def test_abi_surface():
    L = na.load()
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 28
    assert header_define("FA_MX_BLOCK") == na.MX_BLOCK == quant.MX_BLOCK == mxr.BLOCK == 32
    assert header_define("FA_MX_CHUNK") == na.MX_CHUNK == mxr.CHUNK == 2048
    assert (header_define("FA_MX_MIN_EXP"), header_define("FA_MX_MAX_EXP")) == (quant.MX_MIN_EXP, quant.MX_MAX_EXP) == (27, 227)
    assert (header_define("FA_MX_FP4"), header_define("FA_MX_FP8")) == (na.MX_FP4, na.MX_FP8) == (4, 8)
    assert "fa_deq_fold_mx" in na.EXPORTS and hasattr(L, "fa_deq_fold_mx")
    assert _build.HERE / "csrc" / "fa_mx.hip" in _build.SOURCES


OUT = FAKE + 0x10000
GOOD = dict(stack=FAKE, stride=2048, n=5, scales=FAKE, sstride=128, weights=FAKE, center=None, acc_in=None, acc_out=OUT,
            col=0, ncols=4096, elem=4)  # a row of 2048 bytes holds 4096 FP4 columns: 128 scale blocks
ARG = [dict(stack=None), dict(scales=None), dict(weights=None), dict(acc_out=None), dict(n=0), dict(ncols=-1), dict(col=-2048),
       dict(col=2048, ncols=4096), dict(ncols=4097), dict(elem=8, ncols=2049), dict(stride=-16), dict(ncols=2**63 - 1),
       dict(col=2**63 - 2047), dict(elem=0), dict(elem=6), dict(elem=16), dict(sstride=124), dict(sstride=0),
       dict(acc_in=OUT + 16), dict(acc_in=OUT - 4 * 4096 + 16), dict(n=0, stack=FAKE + 4)]  # the last: an argument error wins
ALIGN = [dict(stack=FAKE + 4), dict(stride=2048 + 8), dict(center=FAKE + 4), dict(acc_out=OUT + 8), dict(acc_in=FAKE + 4),
         dict(scales=FAKE + 2), dict(weights=FAKE + 1), dict(sstride=130), dict(col=32, ncols=1), dict(col=1024, ncols=16)]
OK = [dict(ncols=0), dict(col=4096, ncols=0), dict(ncols=0, sstride=0), dict(elem=8, ncols=0, col=2048)]


@pytest.mark.parametrize("want,cases", [("FA_ERR_ARG", ARG), ("FA_ERR_ALIGN", ALIGN), (None, OK)])
def test_deq_fold_mx_refusals_need_no_gpu(want, cases):
    L, code = na.load(), header_define(want) if want else 0
    for over in cases:
        a = dict(GOOD, **over)
        rc = L.fa_deq_fold_mx(a["stack"], a["stride"], a["n"], a["scales"], a["sstride"], a["weights"], a["center"],
                              a["acc_in"], a["acc_out"], a["col"], a["ncols"], a["elem"], None)
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0, over
        assert rc == code and (code == 0 or L.fa_last_error()), over
    assert want != "FA_ERR_ALIGN" or b"2048" in L.fa_last_error()  # the last case: col_begin's unit is named


def unpacked(e, bits, n):
    return mxr.codes_of(e[f"mx{bits}"][None], bits)[0, :n]


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("n", [1, 31, 33, 300])
def test_quantizer_is_the_rule_in_float64(n, bits):
    """Random magnitudes over 60 binades, exact ties (odd multiples of half a step: to the even code), values
    past the block's largest binade (saturation), zeros of both signs, an all-zero block and blocks whose
    exponent is clamped at both ends."""
    rng = np.random.default_rng(n + bits)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    ties = (np.arange(n) % 16 + 0.5) * (0.5 if bits == 4 else 0.125) * np.where(np.arange(n) % 3, 1, -1)
    top = np.full(n, 7.9, np.float32) * np.where(np.arange(n) % 2, 1, -1)  # 7.9 / 2 = 3.95 ... all beyond 6: saturates FP4
    tiny, huge = np.full(n, 2.0 ** -120, np.float32), np.full(n, -(2.0 ** 120), np.float32)
    x[::5] = (0.0, -0.0)[n % 2]
    g = rng.standard_normal(n).astype(np.float32)
    for vals, center in ((x, None), (x, g), (ties.astype(np.float32), None), (top, None), (tiny, None), (huge, None)):
        vals = vals.astype(np.float32)
        e = quant.quantize_array(vals.reshape(-1, 1), center, bits=bits, format="mx")
        codes, scales = mxr.quantize(vals if center is None else vals - center, bits)
        assert set(e) == {f"mx{bits}", "shape", "scale", "block", "delta"} and e["block"] == 32 and e["delta"] is (center is not None)
        assert e["shape"] == (n, 1) and e[f"mx{bits}"].dtype == np.uint8 and e[f"mx{bits}"].shape == (-(-n * bits // 8),)
        assert e["scale"].dtype == np.uint8 and (e["scale"] == scales).all() and (unpacked(e, bits, n) == codes).all()
        back = quant.dequantize_entry(e, center).reshape(-1)
        want = mxr.deq_fold(None, e[f"mx{bits}"][None], e["scale"][None], [1.0], n, bits, center)
        assert mxr.same_bits(back, want) and np.isfinite(back).all()
    assert (scales == 227).all() and (mxr.quantize(tiny, bits)[1] == 27).all()  # clamped: 2^120 saturates, 2^-120 is 0 or tiny
    z = quant.quantize_array(np.concatenate([np.zeros(32, np.float32), x]), bits=bits, format="mx")
    assert z["scale"][0] == 27 and not unpacked(z, bits, 32).any()  # an all-zero block


def entry(bits=4, **fields):
    e = quant.quantize_array(np.random.default_rng(2).standard_normal(300).astype(np.float32), bits=bits, format="mx")
    if "scale1" in fields:
        e["scale"][1] = fields.pop("scale1")
    return dict(e, **fields)


@pytest.mark.parametrize("exc,match,fields", [
    *[(ValueError, "27 ... 227", {"scale1": v}) for v in (0, 26, 228, 255)],
    (ValueError, "need 150 code bytes", {"mx4": np.zeros(149, np.uint8)}), (ValueError, "need 10 scales", {"scale": np.full(9, 127, np.uint8)}),
    (TypeError, "mx4 must be uint8", {"mx4": np.zeros(150, np.int8)}), (TypeError, "scales must be uint8", {"scale": np.ones(10, np.float32)}),
    (ValueError, "block must be 32", {"block": 128}), (ValueError, "shape", {"shape": 300}),
    (ValueError, "one format", {"q4": np.zeros(150, np.uint8)}), (ValueError, "one format", {"mx8": np.zeros(300, np.uint8)}),
])
def test_check_entry_and_check_round_refusals(exc, match, fields):
    bad = entry(**fields)
    with pytest.raises(exc, match=match):
        quant.check_entry("w", bad)
    with pytest.raises(exc, match=match):
        quant.check_round([{"w": entry()}, {"w": bad}], ["w"])


def test_legal_scales_keywords_and_the_round_s_format():
    assert all(quant.check_entry("w", entry(b, scale1=ok)) for ok in (27, 127, 227) for b in (4, 8))
    nan = entry(8, mx8=np.full(300, 0xFF, np.uint8))  # E4M3's NaN codes are legal input
    assert quant.check_entry("w", nan) and np.isnan(quant.dequantize_entry(nan)).all()
    sd = {"w": np.ones((3, 50), np.float32), "b": np.ones(7, np.float32), "n": np.array(3)}
    for f in (quant.quantize_array, quant.quantize_state_dict):
        arg = sd["w"] if f is quant.quantize_array else sd
        with pytest.raises(ValueError, match="stochastic"):
            f(arg, stochastic=True, rng=np.random.default_rng(0), bits=4, format="mx")
        for kw in (dict(bits=1, format="mx"), dict(bits=4, format="fp"), dict(bits=2, format="mx")):
            with pytest.raises(ValueError, match="format|bits"):
                f(arg, **kw)
    with pytest.raises(ValueError, match="finite"):
        quant.quantize_array(np.array([1.0, np.inf], np.float32), bits=8, format="mx")
    m4, m8, u4, u8, u1 = (quant.quantize_state_dict(sd, bits=b, format=f) for b, f in ((4, "mx"), (8, "mx"), (4, "int"), (8, "int"), (1, "int")))
    assert quant.is_quantized(m4) and quant.bits_of(m4["w"]) == 4 and quant.bits_of(m8["w"]) == 8 and quant.entry_shape(m8["w"]) == (3, 50)
    assert quant.check_round([m4, m4], list(sd))[::4] == (["w", "b"], "mx4") and quant.check_round([m8], list(sd))[4] == "mx8"
    for mixed in ([m4, u4], [u8, m8], [m4, m8], [u1, m4], [dict(m4, b=m8["b"])] * 2):  # across clients, across keys
        with pytest.raises(ValueError, match="one format"):
            quant.check_round(mixed, list(sd))
    for mixed, match in (([u8, u4], "all q8 or all q4"), ([u4, u1], "one width")):  # the existing messages stay
        with pytest.raises(ValueError, match=match):
            quant.check_round(mixed, list(sd))


def test_strategy_names_and_constructor():
    d = flearn_amd.QuantizedAVG()
    assert (d.bits, d.format) == (8, "int")
    for b in (4, 8):
        s = flearn_amd.setup_strategy(f"avg_mx{b}", None, delta=False, output="float32", chunk_clients=4)
        assert type(s) is flearn_amd.QuantizedAVG and (s.bits, s.format, s.delta, s.output, s.chunk_clients) == (b, "mx", False, "float32", 4)
        up = s.client(type("Trainer", (), {"weight": {"w": np.arange(40, dtype=np.float32), "n": np.array(2)}})())["params"]
        assert f"mx{b}" in up["w"] and up["n"] == 2
    for kw in (dict(bits=1, format="mx"), dict(bits=4, format="MX"), dict(bits=4, format=None), dict(bits=4, format="mx", stochastic=True),
               dict(bits=8, format="mx", error_feedback=True)):
        with pytest.raises(ValueError, match="format|stochastic"):
            flearn_amd.QuantizedAVG(**kw)
