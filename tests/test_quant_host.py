"""Host-only: the ABI 23 surface and every refusal of fa_deq_fold_q8 (decided before any HIP call),
plan_q8_window (tests/quant_geometry_probe.cpp against flearn_amd/csrc/fa_quant_geometry.hpp, and its
Python restatement tests/quant_ref.py), flearn_amd/quant.py's quantizer against its restatement and
its derived error bound, the wire round trip of a quantized upload, and the refusals of
Aggregator.ensemble_quantized and the QuantizedAVG strategy, raised before the engine touches a
device.  No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import flearn_amd
import quant_ref as qr
from flearn_amd import _build
from flearn_amd import _native as na
from flearn_amd import quant, quantround

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
HEADER = REPO / "include" / "flearn_amd.h"
CUS = (256, 304, 64)


def header_define(name):
    return int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", HEADER.read_text()).group(1))


@pytest.fixture(scope="module")
def L():
    return na.load()


# ---------------------------------------------------------------------------------------------
# ABI 23
# ---------------------------------------------------------------------------------------------


def test_abi_surface(L):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_[a-z0-9_]+)\s*\(", text))) == sorted(na.EXPORTS)
    assert re.search(r"\bint\s+fa_deq_fold_q8\s*\(\s*const\s+int8_t\s*\*", text)
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 23
    assert header_define("FA_Q8_BLOCK") == na.Q8_BLOCK == quant.BLOCK == qr.BLOCK == 1024
    out = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    assert "fa_deq_fold_q8" in na.EXPORTS and hasattr(L, "fa_deq_fold_q8")
    assert re.search(r"\bT\s+fa_deq_fold_q8$", out, flags=re.M)
    assert CSRC / "fa_quant.hip" in _build.SOURCES
    assert "fa_deq_fold_q8" in re.search(r"/\* HOST function: what the calling thread's last.*?call launched", HEADER.read_text(),
                                         flags=re.S).group(0)


FAKE = 0x100000  # never dereferenced: validation rejects the call first


def nothing_launched(L):
    rec = na.LaunchRecord()
    assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0


def test_deq_fold_refusals_need_no_gpu(L):
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")

    def call(stack=FAKE, stride=4096, n=5, scales=FAKE, sstride=4, weights=FAKE, center=None, acc_in=None,
             acc_out=FAKE + 0x10000, col=0, ncols=4096):
        rc = L.fa_deq_fold_q8(stack, stride, n, scales, sstride, weights, center, acc_in, acc_out, col, ncols, None)
        nothing_launched(L)
        return rc

    for null in ("stack", "scales", "weights", "acc_out"):
        assert call(**{null: None}) == arg and b"null" in L.fa_last_error()
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error()
    assert call(n=-1) == arg and call(n=-(2**31)) == arg
    assert call(ncols=-1) == arg and b"window" in L.fa_last_error()
    assert call(col=-1024) == arg and call(col=1024, ncols=4096) == arg and call(col=8192, ncols=0) == arg
    big = 2**63 - 1  # sums of these would overflow: the window check must not form them
    assert call(col=big - 1023, ncols=2048) == arg and call(ncols=big) == arg
    assert call(sstride=3) == arg and b"scale_stride" in L.fa_last_error()  # the window's last block has no scale
    assert call(sstride=0) == arg and call(col=3072, ncols=1024, sstride=3) == arg
    # acc_in: the same array, or one that shares no byte of the window
    out = FAKE + 0x10000
    assert call(acc_in=out + 16) == arg and b"overlap" in L.fa_last_error()
    assert call(acc_in=out + 4 * 4096 - 16) == arg and call(acc_in=out - 4 * 4096 + 16) == arg
    assert call(n=0, stack=FAKE + 4) == arg  # an argument error wins over an alignment error, as for fa_fold
    # alignment
    assert call(stack=FAKE + 4) == align and call(stack=FAKE + 8) == align and call(stack=FAKE + 1) == align
    assert call(stride=4096 + 8) == align and call(stride=1032, ncols=1024, sstride=2) == align
    assert b"16" in L.fa_last_error()
    assert call(col=512, ncols=1024) == align and b"1024" in L.fa_last_error()
    assert call(col=16, ncols=16) == align and call(col=1023, ncols=1) == align
    assert call(center=FAKE + 4) == align and call(acc_out=out + 8) == align and call(acc_in=FAKE + 4) == align
    assert call(scales=FAKE + 2) == align and call(weights=FAKE + 1) == align and call(weights=FAKE + 2) == align
    assert b"aligned" in L.fa_last_error()
    # an empty window is a no-op, and scales / weights need 4-byte alignment only
    assert call(ncols=0) == 0 and call(col=4096, ncols=0) == 0 and call(ncols=0, sstride=0) == 0
    assert call(ncols=0, scales=FAKE + 4, weights=FAKE + 4) == 0


# ---------------------------------------------------------------------------------------------
# plan_q8_window
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("quant_geometry") / "quant_geometry_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "quant_geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(x) for x in f.split()] for f in out]

    return ask


BOUNDARIES = [b * 1024 + d for b in (1, 4, 8, 192, 4 * 192, 8 * 192, 8 * 208, 8 * 256, 8 * 247) for d in (-1, 0, 1)]
WIDTHS = sorted({1, 15, 16, 17, 4099, 70001, 1 << 20, 25_610_152, (1 << 25) + 1, *BOUNDARIES})
FORCED = (0, 1, 2, 7, 512)


@pytest.mark.parametrize("cus", CUS)
def test_plan_q8_window(cus, probe):
    qs = [(w, f) for w in WIDTHS for f in FORCED]
    plans = probe([f"plan {w} {cus} {f}" for w, f in qs])
    small = [(w, f) for w, f in qs if w <= 1 << 21]
    covers = dict(zip(small, probe([f"cover {w} {cus} {f}" for w, f in small])))
    for (w, f), got in zip(qs, plans):
        v, ww, d, grid = got
        assert tuple(got) == tuple(qr.plan(w, cus, f)), (w, f)  # the restatement the GPU tests use
        chunks = -(-w // 1024)
        assert ww == 4 and v in qr.VS and v * ww * d == 64 and 1 <= grid <= chunks
        assert qr.instance(v) in qr.TARGETS
        if f:
            assert grid == min(f, chunks)
        else:
            assert grid <= max(qr.natural_grid(cus), cus * 13 // 16)
        if (w, f) in covers:  # the blocks' pieces cover the window exactly once, in pieces the lanes can hold
            pc, pieces, bad, widest = covers[(w, f)]
            assert bad == 0 and 1 <= pc <= v * ww and pieces == -(-chunks // pc) and widest == -(-pieces // grid)
    for v, (w, f) in qr.COVER.items():
        for c in CUS:
            assert qr.plan(w, c, f).V == v
    assert set(qr.COVER) == set(qr.VS)


# ---------------------------------------------------------------------------------------------
# the client's quantizer
# ---------------------------------------------------------------------------------------------


def magnitudes(seed=0):
    """fp32 arrays over the whole range of magnitudes, odd sizes, with exact zeros and ties"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (1, 3, 1023, 1024, 1025, 5000):
        for e in (-38, -30, -10, -3, 0, 3, 10, 30, 38):
            out.append(np.clip(rng.standard_normal(n) * 10.0 ** e, -3.4e38, 3.4e38).astype(np.float32))
    out.append(np.array([3e38, -3.4e38, 1.0, 0.0], dtype=np.float32))
    out.append((np.arange(-127, 128) * 0.5).astype(np.float32))  # ties: round half to even
    out.append(np.zeros(2049, dtype=np.float32))
    out.append(np.zeros(0, dtype=np.float32))
    x = rng.standard_normal(3000).astype(np.float32)
    x[1024:2048] = 0  # an all-zero block between two live ones
    out.append(x)
    out.append(np.full(7, 1e-44, dtype=np.float32))  # amax / 127 underflows to 0
    out.append(np.array([1e-40, -3e-41, 0.0], dtype=np.float32))  # a subnormal scale
    return out


def test_quantizer_is_its_restatement_and_within_its_bound():
    for x in magnitudes():
        e = quant.quantize_array(x.reshape(-1, 1) if x.size % 2 else x)
        codes, scales = qr.quantize(x)
        q8, s = e["q8"].reshape(-1), e["scale"]
        assert e["block"] == 1024 and e["delta"] is False and e["q8"].dtype == np.int8 and s.dtype == np.float32
        assert e["q8"].size == x.size and s.shape == (qr.n_blocks(x.size),)
        assert (q8 == codes.reshape(-1)).all() and qr.same_bits(s, scales)
        assert np.abs(q8.astype(np.int32)).max(initial=0) <= 127
        assert np.isfinite(s).all() and (s >= 0).all()
        per = qr.col_scales(s, x.size)
        assert (q8[per == 0] == 0).all()  # the scale-0 rule
        back = quant.dequantize_entry(e).reshape(-1)
        assert qr.same_bits(back, qr.dequantize(q8, s))
        # one rounding of x / s and one of s * d with |d| <= 127: 254 * 2^-24 < 2^-16
        normal = per >= np.float32(2.0 ** -126)
        err = np.abs(back.astype(np.float64) - x.astype(np.float64))
        assert (err[normal] <= per[normal].astype(np.float64) * (0.5 + 2.0 ** -16)).all()
        zero = per == 0  # what a zero scale drops is below 127 * the smallest subnormal
        assert (np.abs(x[zero]) < 127 * 2.0 ** -149).all()


def test_quantizer_refuses_non_finite_and_other_dtypes():
    for bad in (np.nan, np.inf, -np.inf):
        x = np.ones(2000, dtype=np.float32)
        x[1500] = bad
        with pytest.raises(ValueError, match="finite"):
            quant.quantize_array(x)
        with pytest.raises(ValueError, match="finite"):
            quant.quantize_state_dict({"w": x})
    with pytest.raises(ValueError, match="finite"):  # the difference overflows
        quant.quantize_array(np.full(3, 3e38, np.float32), center=np.full(3, -3e38, np.float32))
    with pytest.raises(TypeError, match="float16"):
        quant.quantize_state_dict({"w": np.ones(3, np.float16)})
    with pytest.raises(TypeError):
        quant.quantize_array(np.ones(3))
    with pytest.raises(ValueError, match="rng"):
        quant.quantize_state_dict({"w": np.ones(3, np.float32)}, stochastic=True)
    with pytest.raises(ValueError, match="center has no key"):
        quant.quantize_state_dict({"w": np.ones(3, np.float32)}, center={})


def test_state_dict_round_trip_and_delta():
    rng = np.random.default_rng(5)
    sd = {"w": rng.standard_normal((3, 700)).astype(np.float32), "b": torch.from_numpy(rng.standard_normal(5).astype(np.float32)),
          "n": np.array(7, dtype=np.int64), "d": rng.standard_normal(4), "e": np.zeros((0, 3), np.float32)}
    q = quant.quantize_state_dict(sd)
    assert quant.is_quantized(q) and not quant.is_quantized(sd) and not quant.is_quantized({})
    assert [k for k, v in q.items() if quant.is_entry(v)] == ["w", "b", "e"]
    assert q["n"] is sd["n"] and q["d"] is sd["d"] and q["w"]["q8"].shape == (3, 700) and q["e"]["scale"].shape == (0,)
    back = quant.dequantize_state_dict(q)
    assert back["w"].dtype == np.float32 and back["w"].shape == (3, 700) and back["n"] is sd["n"]
    assert np.abs(back["w"] - sd["w"]).max() <= q["w"]["scale"].max() * (0.5 + 2.0 ** -16)
    g = {k: (np.asarray(v) + 0.01 * rng.standard_normal(np.shape(v))) for k, v in sd.items() if k != "n"}  # float64
    g["n"] = np.array(6, dtype=np.int64)
    qd = quant.quantize_state_dict(sd, center=g)
    assert all(v["delta"] is True for v in qd.values() if quant.is_entry(v))
    g32 = g["w"].astype(np.float32)
    codes, scales = qr.quantize(sd["w"], center=g32)
    assert (qd["w"]["q8"] == codes).all() and qr.same_bits(qd["w"]["scale"], scales)
    assert qd["w"]["scale"].max() < q["w"]["scale"].max() / 10  # the update is small: finer steps
    back = quant.dequantize_state_dict(qd, center=g)
    assert qr.same_bits(back["w"], qr.dequantize(codes, scales, g32))
    with pytest.raises(ValueError, match="centre"):
        quant.dequantize_state_dict(qd)


def test_stochastic_rounding_is_unbiased_and_reproducible():
    x = np.array([0.3, -0.7, 0.5, 12.25, -126.9, 127.0, 0.0, 1e-3] + [0.0] * 1016, dtype=np.float32)  # s = 1
    draws = 10_000
    rng = np.random.default_rng(42)
    acc = np.zeros(8)
    sq = np.zeros(8)
    for _ in range(draws):
        e = quant.quantize_array(x, stochastic=True, rng=rng)
        assert e["scale"][0] == 1.0
        q = e["q8"][:8].astype(np.float64)
        assert ((q == np.floor(x[:8])) | (q == np.ceil(x[:8]))).all()
        acc += q
        sq += q * q
    mean = acc / draws
    frac = x[:8].astype(np.float64) - np.floor(x[:8])
    se = np.sqrt(frac * (1 - frac) / draws)  # a Bernoulli(frac) above the floor
    assert (np.abs(mean - x[:8]) <= 4 * se).all(), (mean, se)
    assert (mean[[5, 6]] == x[[5, 6]]).all()  # integers are never moved
    a = quant.quantize_array(x, stochastic=True, rng=np.random.default_rng(7))
    b = quant.quantize_array(x, stochastic=True, rng=np.random.default_rng(7))
    c = qr.quantize(x, stochastic=True, rng=np.random.default_rng(7))
    assert (a["q8"] == b["q8"]).all() and (a["q8"] == c[0]).all()


def test_wire_round_trip():
    rng = np.random.default_rng(9)
    sd = {"w": rng.standard_normal((40, 70)).astype(np.float32), "b": rng.standard_normal(3).astype(np.float32),
          "n": np.array(3, dtype=np.int64)}
    for center in (None, {k: np.zeros_like(v) for k, v in sd.items()}):
        up = {"agg_weight": 0.25, "params": quant.quantize_state_dict(sd, center)}
        enc = flearn_amd.Encrypt()
        back = enc.decode(enc.encode(up))
        assert back["agg_weight"] == 0.25 and list(back["params"]) == list(up["params"])
        for k, v in up["params"].items():
            r = back["params"][k]
            if not quant.is_entry(v):
                assert np.asarray(r).dtype == v.dtype and (np.asarray(r) == v).all()
                continue
            assert type(r) is dict and set(r) == {"q8", "scale", "block", "delta"}
            assert r["block"] == 1024 and r["delta"] is (center is not None)
            assert r["q8"].dtype == np.int8 and r["q8"].shape == v["q8"].shape and (r["q8"] == v["q8"]).all()
            assert r["scale"].dtype == np.float32 and qr.same_bits(np.asarray(r["scale"]), v["scale"])
            quant.check_entry(k, r)


# ---------------------------------------------------------------------------------------------
# the engine's and the strategy's refusals: before a device is touched
# ---------------------------------------------------------------------------------------------


class Untouchable:
    """Stands for the packer: any use is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine touched its packer ({name}) before refusing")


def bare_engine(**over):
    from flearn_amd.aggregator import Aggregator

    agg = object.__new__(Aggregator)  # no HIP library, no device
    agg.chunk_clients, agg._dist, agg.devices, agg.output = None, False, [torch.device("cpu")], "reference"
    agg.device, agg.packer, agg.last_plan = agg.devices[0], Untouchable(), None
    for k, v in over.items():
        setattr(agg, k, v)
    return agg


def model(seed):
    rng = np.random.default_rng(seed)
    return {"a.weight": rng.standard_normal((30, 50)).astype(np.float32), "a.bias": rng.standard_normal(5).astype(np.float32),
            "n": np.array(seed, dtype=np.int64)}


def uploads(n, center=None):
    return [quant.quantize_state_dict(model(i), center) for i in range(n)]


def with_entry(ups, i, key, **fields):
    ups = [dict(u) for u in ups]
    ups[i][key] = dict(ups[i][key], **fields)
    return ups


def test_binding_and_import_rule():
    from flearn_amd.aggregator import Aggregator

    assert Aggregator.ensemble_quantized is quantround.ensemble_quantized
    assert Aggregator.last_quant is None
    src = Path(quantround.__file__).read_text()
    assert not re.search(r"^\s*(from|import)\s+[.\w]*\b(aggregator|streaming)\b", src, flags=re.M)
    assert not re.search(r"^\s*from\s+\.\s+import\s+.*\b(aggregator|streaming)\b", src, flags=re.M)
    qsrc = Path(quant.__file__).read_text()  # format, quantizer, checks: no device code
    assert not re.search(r"_native|\bops\b|cuda", qsrc)


def test_engine_refusals_touch_no_device():
    from flearn_amd.serverstate import DynState

    n = 4
    ups, w = uploads(n), [1.0] * n
    g = {k: np.zeros_like(v) for k, v in model(0).items()}
    dups = uploads(n, center=g)

    def refused(exc, match, ups=ups, w=w, agg=None, **kw):
        with pytest.raises(exc, match=match):
            (agg or bare_engine()).ensemble_quantized(w, ups, **kw)

    refused(ValueError, "group", agg=bare_engine(_dist=True))
    refused(ValueError, "one device", agg=bare_engine(devices=[torch.device("cpu")] * 2))
    refused(TypeError, "Dyn", server_opt=object.__new__(DynState))
    for k in (0, -1, True, 2.0):
        refused(ValueError, "chunk_clients", agg=bare_engine(chunk_clients=k))
    # the scales
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        s = ups[2]["a.weight"]["scale"].copy()
        s[1] = bad
        refused(ValueError, "finite and >= 0", with_entry(ups, 2, "a.weight", scale=s))
    refused(ValueError, "need 2 scales", with_entry(ups, 1, "a.weight", scale=np.ones(3, np.float32)))
    refused(ValueError, "need 1 scales", with_entry(ups, 3, "a.bias", scale=np.ones((1, 1), np.float32)))
    refused(TypeError, "scale must be float32", with_entry(ups, 1, "a.bias", scale=np.ones(1)))
    # the codes
    refused(TypeError, "q8 must be int8", with_entry(ups, 1, "a.bias", q8=np.zeros(5, np.uint8)))
    refused(TypeError, "q8 must be int8", with_entry(ups, 0, "a.bias", q8=np.zeros(5, np.float32)))
    refused(TypeError, "unsupported value type", with_entry(ups, 0, "a.bias", q8=[0] * 5))
    refused(ValueError, "do not match client 0", with_entry(ups, 2, "a.bias", q8=np.zeros((5, 1), np.int8)))
    refused(ValueError, "do not match client 0",
            with_entry(ups, 2, "a.bias", q8=np.zeros(1025, np.int8), scale=np.ones(2, np.float32)))
    # block and delta
    for block in (512, 2048, 0, 1024.0, True):
        refused(ValueError, "block must be 1024", with_entry(ups, 1, "a.weight", block=block))
    refused(ValueError, "delta=True in a round of delta=False", with_entry(ups, 3, "a.bias", delta=True))
    refused(ValueError, "delta must be a bool", with_entry(ups, 3, "a.bias", delta=1))
    refused(ValueError, "no centre", dups)
    refused(ValueError, "lacks 'scale'", [dict(u, **{"a.bias": {"q8": u["a.bias"]["q8"]}}) for u in ups])
    refused(ValueError, "center has no key", dups, center={"a.weight": g["a.weight"]})
    refused(ValueError, "elements", dups, center=dict(g, **{"a.bias": np.zeros(4, np.float32)}))
    refused(ValueError, "center", dups, center=[1, 2])
    # plain and quantized for one key, either way round; a plain fp32 tensor beside quantized ones
    plain = [dict(u, **{"a.bias": model(i)["a.bias"]}) if i == 2 else u for i, u in enumerate(ups)]
    refused(ValueError, "quantized in some uploads", plain)
    refused(ValueError, "plain fp32", plain[2:] + plain[:2])  # upload 0 is the one with the plain tensor
    refused(ValueError, "plain fp32", [dict(u, extra=np.zeros(3, np.float32)) for u in ups])
    # float16, float64 weights
    refused(TypeError, "float16", [dict(u, h=np.zeros(3, np.float16)) for u in ups])
    refused(TypeError, "float16", [dict(u, h=torch.zeros(3, dtype=torch.float16)) for u in ups])
    for w64 in ([np.float64(1.0)] * n, [np.int64(2)] * n, [np.int32(2)] * n):
        refused(TypeError, "float64", w=w64)
    refused(TypeError, "promote differently", w=[1.0, np.float64(1.0), 1.0, 1.0])
    refused(ValueError, "differ in length", w=[1.0] * 3)
    with pytest.raises(IndexError):
        bare_engine().ensemble_quantized([], [])
    with pytest.raises(KeyError):
        bare_engine().ensemble_quantized(w, ups, key_lst=["a.bias", "missing"])
    for agg, u, kw in ((bare_engine(), ups, {}), (bare_engine(chunk_clients=3), dups, {"center": g}),
                       (bare_engine(), ups, {"key_lst": ["a.bias", "n"]})):  # good rounds get as far as the pack
        with pytest.raises(AssertionError, match="touched its packer"):
            agg.ensemble_quantized(w, u, **kw)


def test_strategy_surface_and_refusals():
    from flearn_amd.strategy import AVG, QuantizedAVG

    assert flearn_amd.QuantizedAVG is QuantizedAVG
    assert "QuantizedAVG" in flearn_amd.__all__ and "QuantizedAVG" in flearn_amd.strategy.__all__
    assert issubclass(QuantizedAVG, AVG)
    s = QuantizedAVG()
    assert (s.server_opt, s.delta, s.stochastic, s.output, s.chunk_clients, s._prev_glob) == (None, True, False, "reference", None, None)
    s = flearn_amd.setup_strategy("avg_q8", None, delta=False, stochastic=True, seed=3, output="float32", chunk_clients=4)
    assert type(s) is QuantizedAVG and (s.delta, s.stochastic, s.seed, s.output, s.chunk_clients) == (False, True, 3, "float32", 4)
    assert type(flearn_amd.setup_strategy("AVG_Q8", None)) is QuantizedAVG
    with pytest.raises(ValueError, match="dict"):
        QuantizedAVG().init_global([1, 2])
    g = {"a": np.ones(3), "b": torch.ones(2, dtype=torch.float64), "n": np.array(3, dtype=np.int64)}
    s = QuantizedAVG()
    s.init_global(g)
    g["a"][0] = 5.0
    assert s._prev_glob["a"][0] == 1.0 and s._prev_glob["a"].dtype == np.float32  # an fp32 copy of its own
    assert s._prev_glob["b"].dtype == torch.float32 and s._prev_glob["n"].dtype == np.int64


class Trainer:
    def __init__(self, sd):
        self.weight = sd
        self.model = self

    def load_state_dict(self, sd):
        self.loaded = sd


def test_client_uploads_quantized_and_takes_its_centre_from_what_it_received():
    from flearn_amd.strategy import QuantizedAVG

    sd = model(1)
    s = QuantizedAVG()
    up = s.client(Trainer(dict(sd)), 3.0)
    assert up["agg_weight"] == 3.0 and up["params"]["a.weight"]["delta"] is False  # nothing received yet
    assert (up["params"]["a.weight"]["q8"] == qr.quantize(sd["a.weight"])[0]).all()
    glob = {k: np.asarray(v, dtype=np.float64) * 0.999 if v.dtype == np.float32 else v for k, v in model(1).items()}
    s.client_receive(Trainer(dict(sd)), {"w_glob": dict(glob)})
    assert s._received["a.weight"].dtype == np.float32 and s._received["n"].dtype == np.int64
    up = s.client(Trainer(dict(sd)), 1.0)
    e = up["params"]["a.weight"]
    codes, scales = qr.quantize(sd["a.weight"], center=glob["a.weight"].astype(np.float32))
    assert e["delta"] is True and (e["q8"] == codes).all() and qr.same_bits(e["scale"], scales)
    assert up["params"]["n"] == 1
    off = QuantizedAVG(delta=False)
    off.client_receive(Trainer(dict(sd)), {"w_glob": dict(glob)})
    assert off.client(Trainer(dict(sd)), 1.0)["params"]["a.weight"]["delta"] is False
    a = QuantizedAVG(stochastic=True, seed=11).client(Trainer(dict(sd)), 1.0)["params"]["a.weight"]["q8"]
    b = QuantizedAVG(stochastic=True, seed=11).client(Trainer(dict(sd)), 1.0)["params"]["a.weight"]["q8"]
    assert (a == b).all() and (a != up["params"]["a.weight"]["q8"]).any()


def test_strategy_errors_take_server_exceptions_route():
    from flearn_amd.strategy import QuantizedAVG

    def rounds(ups):
        return [{"agg_weight": 1.0, "params": u} for u in ups]

    ups = uploads(4)
    g = {k: np.zeros_like(v) for k, v in model(0).items()}
    bad_scale = ups[1]["a.bias"]["scale"].copy()
    bad_scale[0] = np.nan
    for strat, r in ((QuantizedAVG(), rounds(with_entry(ups, 1, "a.bias", scale=bad_scale))),
                     (QuantizedAVG(), rounds(with_entry(ups, 1, "a.bias", block=256))),
                     (QuantizedAVG(), rounds(uploads(3) + [model(3)])),  # quantized and plain uploads in one round
                     (QuantizedAVG(), rounds([model(3)] + uploads(3))),
                     (QuantizedAVG(), rounds(with_entry(ups, 2, "a.weight", q8=torch.zeros((30, 50), dtype=torch.int8, device="meta"))))):
        strat.init_global(g)
        strat._engine = bare_engine()
        with pytest.raises(SystemExit):
            strat.server(r, 0)
        assert set(strat._prev_glob) == set(g) and (strat._prev_glob["a.weight"] == 0).all()  # the centre is kept
    s = QuantizedAVG()  # delta uploads before the server has a centre
    s._engine = bare_engine()
    with pytest.raises(SystemExit):
        s.server(rounds(uploads(3, center=g)), 0)
