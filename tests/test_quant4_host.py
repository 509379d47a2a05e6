"""Host-only: the ABI 24 surface and every refusal of fa_deq_fold_q4 (decided before any HIP call), the
4-bit quantizer against tests/quant4_ref.py bit for bit and against its derived error bound,
check_entry's and check_round's 4-bit refusals, the wire round trip, and the "avg_q4" strategy name."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flearn_amd
import quant4_ref as q4r
from flearn_amd import _build
from flearn_amd import _native as na
from flearn_amd import quant
from test_cabi import FAKE, header_define

REPO = Path(__file__).resolve().parent.parent
MIN = float(2.0 ** -100)


@pytest.fixture(scope="module")
def L():
    return na.load()


def test_abi_surface(L):
    text = (REPO / "include" / "flearn_amd.h").read_text()
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 24
    assert header_define("FA_Q4_BLOCK") == na.Q4_BLOCK == quant.Q4_BLOCK == q4r.BLOCK == 128
    assert header_define("FA_Q4_CHUNK") == na.Q4_CHUNK == q4r.CHUNK == 2048
    floor = float.fromhex(re.search(r"#define\s+FA_Q4_MIN_SCALE\s+(\S+?)f?\s", text).group(1))
    assert floor == float(quant.Q4_MIN_SCALE) == float(q4r.MIN_SCALE) == MIN and quant.Q4_MIN_SCALE.dtype == np.float32
    assert re.search(r"\bint\s+fa_deq_fold_q4\s*\(\s*const\s+uint8_t\s*\*", text)
    out = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    assert "fa_deq_fold_q4" in na.EXPORTS and hasattr(L, "fa_deq_fold_q4") and re.search(r"\bT\s+fa_deq_fold_q4$", out, flags=re.M)
    assert REPO / "flearn_amd" / "csrc" / "fa_quant4.hip" in _build.SOURCES
    assert "fa_deq_fold_q4" in re.search(r"/\* HOST function: what the calling thread's last.*?call launched", text, flags=re.S).group(0)


OUT = FAKE + 0x10000
GOOD = dict(stack=FAKE, stride=2048, n=5, scales=FAKE, sstride=32, weights=FAKE, center=None, acc_in=None, acc_out=OUT,
            col=0, ncols=4096)  # a row of 2048 bytes holds 4096 columns: 32 scale blocks
ARG = [dict(stack=None), dict(scales=None), dict(weights=None), dict(acc_out=None), dict(n=0), dict(n=-1), dict(ncols=-1),
       dict(col=-2048), dict(col=2048, ncols=4096), dict(col=6144, ncols=0), dict(ncols=4097), dict(stride=-16),
       dict(col=2**63 - 2047, ncols=4096), dict(ncols=2**63 - 1), dict(sstride=31), dict(sstride=0),
       dict(col=2048, ncols=129, sstride=17), dict(acc_in=OUT + 16), dict(acc_in=OUT + 4 * 4096 - 16),
       dict(acc_in=OUT - 4 * 4096 + 16), dict(n=0, stack=FAKE + 4)]  # the last: an argument error wins over alignment
ALIGN = [dict(stack=FAKE + 4), dict(stack=FAKE + 1), dict(stride=2048 + 8), dict(col=128, ncols=1), dict(center=FAKE + 4),
         dict(acc_out=OUT + 8), dict(acc_in=FAKE + 4), dict(scales=FAKE + 2), dict(weights=FAKE + 1), dict(col=1024, ncols=16)]
OK = [dict(ncols=0), dict(col=4096, ncols=0), dict(ncols=0, sstride=0), dict(ncols=0, scales=FAKE + 4, weights=FAKE + 4)]


@pytest.mark.parametrize("want,cases", [("FA_ERR_ARG", ARG), ("FA_ERR_ALIGN", ALIGN), (None, OK)])
def test_deq_fold_q4_refusals_need_no_gpu(want, cases, L):
    code = header_define(want) if want else 0
    for over in cases:
        a = dict(GOOD, **over)
        rc = L.fa_deq_fold_q4(a["stack"], a["stride"], a["n"], a["scales"], a["sstride"], a["weights"], a["center"],
                              a["acc_in"], a["acc_out"], a["col"], a["ncols"], None)
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0, over
        assert rc == code and (code == 0 or L.fa_last_error()), over
    assert want != "FA_ERR_ALIGN" or b"2048" in L.fa_last_error()  # the last case: col_begin's unit is named


def arrays():
    rng = np.random.default_rng(11)
    out = [np.clip(rng.standard_normal(n) * 10.0 ** e, -3.4e38, 3.4e38).astype(np.float32)
           for n in (1, 3, 127, 128, 129, 1001) for e in (-38, -30, -10, 0, 10, 38)]
    out.append((np.arange(-14, 15) * 0.5).astype(np.float32))  # s = 1: ties, round half to even
    x = rng.standard_normal(384).astype(np.float32)
    x[128:256] *= np.float32(2.0 ** -105)  # a block under the floor between two live ones
    return out + [x, np.zeros(257, np.float32), np.full(5, 7 * 2.0 ** -100, np.float32)]  # the last: s is the floor, kept


def test_quantizer_is_its_restatement_and_within_its_bound():
    under = 0
    for x in arrays():
        e = quant.quantize_array(x.reshape(-1, 1) if x.size % 2 else x, bits=4)
        q4, scales = q4r.quantize(x)
        assert set(e) == {"q4", "shape", "scale", "block", "delta"} and e["block"] == 128 and e["delta"] is False
        assert e["shape"] == ((x.size, 1) if x.size % 2 else (x.size,)) and type(e["shape"]) is tuple
        assert e["q4"].dtype == np.uint8 and e["q4"].shape == ((x.size + 1) // 2,) and (e["q4"] == q4).all()
        assert e["scale"].dtype == np.float32 and q4r.same_bits(e["scale"], scales)
        codes = q4r.unpack(e["q4"], x.size)
        assert np.abs(codes).max() <= 7 and (x.size % 2 == 0 or e["q4"][-1] >> 4 == 0)  # the spare nibble
        per = q4r.col_scales(e["scale"], x.size)
        live = per >= MIN
        assert ((per == 0) | live).all() and (codes[~live] == 0).all()
        back = quant.dequantize_entry(e).reshape(-1)
        assert q4r.same_bits(back, q4r.dequantize(e["q4"], x.size, e["scale"]))
        # one rounding of x / s with |x / s| <= 7 (1 + 2^-23) and one of s * q with |q| <= 7: 14 * 2^-24 < 2^-20
        err = np.abs(back.astype(np.float64) - x.astype(np.float64))
        assert (err[live] <= per[live].astype(np.float64) * (0.5 + 2.0 ** -20)).all()
        assert (np.abs(x[~live]).astype(np.float64) < 7.5 * MIN).all()  # what the floor drops
        under += int((~live & (x != 0)).sum())
    assert under  # the data does reach under the floor
    assert quant.quantize_array(np.ones(3, np.float32))["block"] == 1024  # the default is q8, as it was
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            quant.quantize_array(np.array([1.0, bad], np.float32), bits=4)


def test_stochastic_rounding_is_unbiased():
    x = np.array([0.3, -0.7, 0.5, 2.25, -6.9, 7.0, 0.0, 1e-3], dtype=np.float32)  # s = 1
    draws, rng, acc = 10_000, np.random.default_rng(42), np.zeros(8)
    for _ in range(draws):
        e = quant.quantize_array(x, stochastic=True, rng=rng, bits=4)
        q = q4r.unpack(e["q4"], 8).astype(np.float64)
        assert e["scale"][0] == 1.0 and ((q == np.floor(x)) | (q == np.ceil(x))).all()
        acc += q
    frac = x.astype(np.float64) - np.floor(x)
    assert (np.abs(acc / draws - x) <= 4 * np.sqrt(frac * (1 - frac) / draws)).all()


def entry(**fields):
    e = quant.quantize_array(np.random.default_rng(2).standard_normal(300).astype(np.float32), bits=4)
    if "scale1" in fields:
        e["scale"][1] = fields.pop("scale1")
    return dict(e, **fields)


@pytest.mark.parametrize("exc,match,fields", [
    *[(ValueError, "2\\^-100", {"scale1": v}) for v in (2.0 ** -101, 1e-45, -1.0, np.nan, np.inf)],
    (ValueError, "need 150 code bytes", {"q4": np.zeros(151, np.uint8)}), (ValueError, "need 3 scales", {"scale": np.ones(2, np.float32)}),
    (TypeError, "q4 must be uint8", {"q4": np.zeros(150, np.int8)}), (ValueError, "block must be 128", {"block": 1024}),
    (ValueError, "shape", {"shape": 300}), (ValueError, "not both", {"q8": np.zeros(300, np.int8)}),
])
def test_check_entry_and_check_round_refusals(exc, match, fields):
    with pytest.raises(exc, match=match):
        quant.check_entry("w", entry(**fields))
    with pytest.raises(exc, match=match):
        quant.check_round([{"w": entry()}, {"w": entry(**fields)}], ["w"])


def test_legal_scales_and_the_round_s_width():
    for ok in (0.0, -0.0, 2.0 ** -100, 1.0, 2.0 ** 125):
        quant.check_entry("w", entry(scale1=ok))
    sd = {"w": np.ones((3, 50), np.float32), "b": np.ones(7, np.float32), "n": np.array(3)}
    u4, u8 = quant.quantize_state_dict(sd, bits=4), quant.quantize_state_dict(sd)
    assert quant.is_quantized(u4) and quant.is_entry(u4["w"]) and not quant.is_entry(u4["n"])
    assert quant.check_round([u4, u4], list(sd))[::4] == (["w", "b"], 4) and quant.check_round([u8, u8], list(sd))[4] == 8
    for mixed in ([u4, u8], [u8, u4], [dict(u4, b=u8["b"])] * 2):  # across clients, across keys
        with pytest.raises(ValueError, match="all q8 or all q4"):
            quant.check_round(mixed, list(sd))


def test_wire_round_trip():
    rng = np.random.default_rng(9)
    sd = {"w": rng.standard_normal((41, 7)).astype(np.float32), "b": rng.standard_normal(3).astype(np.float32), "n": np.array(3)}
    for center in (None, {k: np.zeros_like(v) for k, v in sd.items()}):
        up = {"agg_weight": 0.25, "params": quant.quantize_state_dict(sd, center, bits=4)}
        enc = flearn_amd.Encrypt()
        back = enc.decode(enc.encode(up))
        assert back["agg_weight"] == 0.25 and list(back["params"]) == list(up["params"])
        for k in ("w", "b"):
            r, v = back["params"][k], up["params"][k]
            assert type(r) is dict and set(r) == set(v) and r["block"] == 128 and r["delta"] is (center is not None)
            assert type(r["shape"]) is tuple and r["shape"] == v["shape"] and r["q4"].dtype == np.uint8
            assert (r["q4"] == v["q4"]).all() and q4r.same_bits(np.asarray(r["scale"]), v["scale"])
            assert q4r.same_bits(quant.dequantize_entry(r, center and center[k], k), quant.dequantize_entry(v, center and center[k], k))


def test_strategy_name_and_bits():
    s = flearn_amd.setup_strategy("avg_q4", None, delta=False, seed=3, output="float32", chunk_clients=4)
    assert type(s) is flearn_amd.QuantizedAVG and (s.bits, s.delta, s.seed, s.output, s.chunk_clients) == (4, False, 3, "float32", 4)
    assert flearn_amd.QuantizedAVG().bits == 8 and flearn_amd.setup_strategy("avg_q8", None).bits == 8
    for bad in (2, 16, "4", True, None):
        with pytest.raises(ValueError, match="bits"):
            flearn_amd.QuantizedAVG(bits=bad)
    up = s.client(type("Trainer", (), {"weight": {"w": np.linspace(-1, 1, 300, dtype=np.float32), "n": np.array(2)}})())
    assert set(up["params"]["w"]) == {"q4", "shape", "scale", "block", "delta"} and up["params"]["w"]["delta"] is False
