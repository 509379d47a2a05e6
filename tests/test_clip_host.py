"""Host-only: flearn_amd/clip.py against its restatement (tests/clip_ref.py), plan_rownorm_window
(tests/clip_geometry_probe.cpp against flearn_amd/csrc/fa_geometry.hpp alone, and its Python
restatement), the ABI 20 surface and every refusal of fa_rownorm2_f32 / fa_clip_sum_f32 (decided
before any HIP call), and the refusals of Aggregator.ensemble_clipped and the NormClip strategy,
raised before the engine touches a device.  No GPU."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import clip_ref as cr
import flearn_amd
from flearn_amd import _native as na
from flearn_amd import clip, robustround

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
HEADER = REPO / "include" / "flearn_amd.h"
CUS = (256, 304, 64)


def header_define(name):
    return int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", HEADER.read_text()).group(1))


# ---------------------------------------------------------------------------------------------
# radius and scales
# ---------------------------------------------------------------------------------------------


def test_radius_by_quantile():
    d2 = np.array([9.0, 1.0, 4.0, 4.0, np.inf, 16.0, np.nan, 4.0])  # finite norms 1 2 2 2 3 4
    for q, want in ((1 / 6, 1.0), (0.17, 2.0), (0.5, 2.0), (0.51, 2.0), (2 / 3, 2.0), (0.7, 3.0), (0.9, 4.0), (1.0, 4.0),
                    (1e-9, 1.0)):
        assert clip.clip_radius(d2, None, q) == cr.radius(d2, quantile=q) == want, q
    assert clip.clip_radius([np.nan, 25.0, -np.inf], None, 0.3) == 5.0  # one finite norm: every q picks it
    assert clip.clip_radius([np.nan, 25.0], None, 1.0) == 5.0
    assert clip.clip_radius(d2, 2.5, None) == 2.5 and clip.clip_radius(d2, math.inf, None) == math.inf
    assert isinstance(clip.clip_radius(d2, None, 0.5), float)
    rng = np.random.default_rng(0)
    for _ in range(50):
        v = rng.standard_normal(rng.integers(1, 40)) ** 2
        q = float(rng.uniform(1e-3, 1.0))
        assert clip.clip_radius(v, None, q) == cr.radius(v, quantile=q)
    for bad in ([], [np.nan], [np.inf, np.nan, -np.inf]):
        with pytest.raises(ValueError, match="finite"):
            clip.clip_radius(bad, None, 0.5)
    with pytest.raises(ValueError, match="per client"):
        clip.clip_radius(np.zeros((2, 2)), None, 0.5)


def test_scales_at_the_rules_edges():
    tau = 3.0
    up = np.nextafter(9.0, 10.0)
    huge, tiny_tau = 1e300, 1e-30
    d2 = np.array([9.0, 0.0, np.inf, np.nan, up, 36.0, -np.inf, 4.0])
    s = clip.clip_scales(d2, tau)
    assert s.dtype == np.float32 and s.tobytes() == cr.scales(d2, tau).tobytes()
    # sqrt(d2) == tau and d2 = 0 pass; non-finite norms are replaced; sqrt(up) > 3 but 3 / sqrt(up) rounds to 1
    assert math.sqrt(up) > tau and np.float32(tau / math.sqrt(up)) == 1.0
    assert s.tolist() == [1.0, 1.0, 0.0, 0.0, 1.0, 0.5, 0.0, 1.0]
    under = clip.clip_scales([huge], tiny_tau)  # 1e-30 / 1e150 underflows fp32: a scale of 0
    assert under.tolist() == [0.0] and cr.scales([huge], tiny_tau).tolist() == [0.0]
    assert clip.clip_scales(d2, math.inf).tolist() == [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0]
    rng = np.random.default_rng(1)
    for _ in range(50):
        v = rng.standard_normal(17) ** 2 * 10.0 ** rng.integers(-3, 4)
        t = float(rng.uniform(0.01, 30.0))
        got = clip.clip_scales(v, t)
        assert got.tobytes() == cr.scales(v, t).tobytes() and ((got > 0) & (got <= 1)).all()
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="tau"):
            clip.clip_scales(d2, bad)


@pytest.mark.parametrize("tau,quantile", [(None, None), (1.0, 0.5), (0.0, None), (-1.0, None), (math.nan, None), (True, None),
                                          ("1", None), (None, 0.0), (None, 1.5), (None, -0.1), (None, math.nan),
                                          (None, True), (None, "0.5"), ([1.0], None)])
def test_bad_radius_arguments(tau, quantile):
    with pytest.raises(ValueError):
        clip.check_radius(tau, quantile)
    with pytest.raises(ValueError):
        clip.clip_radius([1.0, 2.0], tau, quantile)


def test_good_radius_arguments_and_no_torch():
    assert clip.check_radius(2, None) == (2.0, None) and clip.check_radius(np.float32(0.5), None) == (0.5, None)
    assert clip.check_radius(math.inf, None) == (math.inf, None)
    assert clip.check_radius(None, 1) == (None, 1.0) and clip.check_radius(None, np.float64(0.25)) == (None, 0.25)
    assert "torch" not in clip.__dict__ and "torch" not in Path(clip.__file__).read_text().split('"""', 2)[2]


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("clip_geometry") / "clip_geometry_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "clip_geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(x) for x in f.split()] for f in out]

    return ask


NS = (1, 2, 64, 65, 128)
BOUNDARIES = [b + d for b in (256, 1024, 4096, 16384, 49152, 192 * 16384, 512 * 16384) for d in (-1, 0, 1)]
WIDTHS = sorted({1, 3, 4, 255, 4099, 70001, 1 << 20, 25_610_152, (1 << 25) - 1, 1 << 25, *BOUNDARIES})
FORCED = (0, 1, 2, 512)


@pytest.mark.parametrize("cus", CUS)
def test_plan_rownorm_window(cus, probe, L):
    qs = [(n, w, f) for n in NS for w in WIDTHS for f in FORCED]
    plans = probe([f"plan {n} {w} {cus} {f}" for n, w, f in qs])
    small = [(n, w, f) for n, w, f in qs if w <= 1 << 20 and n in (1, 128)]
    covers = dict(zip(small, probe([f"cover {n} {w} {cus} {f}" for n, w, f in small])))
    for (n, w, f), got in zip(qs, plans):
        v, ww, d, chunks, pc, pieces, grid, per_block, chain, work, cap = got
        assert tuple(got[:10]) == tuple(cr.plan(n, w, cus, f)), (n, w, f)  # the restatement the GPU tests use
        assert ww == 4 and v in (1, 2, 4, 8, 16) and v * ww * d == 64
        assert chunks == -(-(-(-w // 4)) // 64) and 1 <= pc <= v * ww
        assert pieces == -(-chunks // pc) and 1 <= grid <= min(pieces, 512)
        if f:
            assert grid <= f
        assert per_block == -(-pieces // grid)
        assert chain == v + 2 + 7 + per_block + ww - 1
        assert work == grid * n * 4 <= cap == cr.workspace_bytes(n, w) == L.fa_rownorm_workspace(n, w)
        if f == 512 and pieces >= 512:
            assert work == cap  # the cap is reached: what fa_rownorm_workspace returns is what a launch may need
        if (n, w, f) in covers:  # the blocks' pieces cover the window exactly once and no block is idle
            empty, bad, widest = covers[(n, w, f)]
            assert empty == 0 and bad == 0 and widest == per_block
    # the natural grid keeps the chain short: 2^25 columns are 2,048 full pieces, swept in rounds of the grid
    assert max(p[8] for (n, w, f), p in zip(qs, plans) if f == 0) == 16 + 2 + 7 + 3 + -(-2048 // cr.natural_grid(cus))
    assert [r[0] for r in probe(["plan 0 300 64 0", "plan 129 300 64 0", "plan -1 300 64 0"])] == [0, 0, 0]


# ---------------------------------------------------------------------------------------------
# ABI 20
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def L():
    return na.load()


NEW = ("fa_rownorm_workspace", "fa_rownorm2_f32", "fa_clip_sum_f32")


def test_abi_surface(L):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_[a-z0-9_]+)\s*\(", text))) == sorted(na.EXPORTS)
    assert re.search(r"\bint64_t\s+fa_rownorm_workspace\s*\(", text)
    assert re.search(r"\bint\s+fa_rownorm2_f32\s*\(", text) and re.search(r"\bint\s+fa_clip_sum_f32\s*\(", text)
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 20
    assert header_define("FA_CLIP_MAX_CLIENTS") == na.CLIP_MAX_CLIENTS == cr.MAX_CLIENTS == 128
    out = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in na.EXPORTS and hasattr(L, name)
        assert re.search(rf"\bT\s+{name}$", out, flags=re.M)


def test_workspace_is_the_capped_size(L):
    for n in (1, 2, 64, 65, 100, 128):
        for w in (1, 257, 70001, 512 * 256, 512 * 256 + 1, 25_610_152):
            assert L.fa_rownorm_workspace(n, w) == cr.workspace_bytes(n, w)
            for cus in CUS + (1024,):  # whatever the device and the forced grid, a launch's partials fit
                for forced in (0, 1, 7, 100000):
                    assert cr.launch_plan(n, w, cus, forced).workspace_bytes <= cr.workspace_bytes(n, w)
    arg = header_define("FA_ERR_ARG")
    assert [L.fa_rownorm_workspace(n, 64) for n in (0, -1, 129)] == [arg] * 3
    assert L.fa_rownorm_workspace(5, 0) == arg and L.fa_rownorm_workspace(5, -7) == arg
    assert L.fa_rownorm_workspace(100, 2**63 - 1) == L.fa_rownorm_workspace(100, 2**40) == 512 * 100 * 4


FAKE = 0x100000  # never dereferenced: validation rejects the call first


def nothing_launched(L):
    rec = na.LaunchRecord()
    assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0


def test_rownorm_refusals_need_no_gpu(L):
    arg, align, size = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN"), header_define("FA_ERR_SIZE")

    def call(stack=FAKE, stride=64, n=5, center=None, col=0, ncols=64, work=FAKE, wbytes=1 << 20, out=FAKE):
        rc = L.fa_rownorm2_f32(stack, stride, n, center, col, ncols, work, wbytes, out, None)
        nothing_launched(L)
        return rc

    assert call(stack=None) == arg and call(work=None) == arg and call(out=None) == arg
    assert b"null" in L.fa_last_error()
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error()
    assert call(n=-3) == arg
    assert call(n=129) == arg and b"128" in L.fa_last_error()
    assert call(n=2**31 - 1) == arg
    assert call(ncols=0) == arg and b"n_cols" in L.fa_last_error()
    assert call(ncols=-1) == arg
    assert call(col=-4) == arg and b"window" in L.fa_last_error()
    assert call(col=8, ncols=60) == arg  # window > stride
    big = 2**63 - 1  # sums of these would overflow: the window check must not form them
    assert call(col=big - 3, ncols=8) == arg and call(ncols=big) == arg and call(stride=big - 3, col=64, ncols=big) == arg
    need = L.fa_rownorm_workspace(5, 64)
    assert need == 20
    assert call(wbytes=need - 1) == size and str(need).encode() in L.fa_last_error()
    assert call(wbytes=0) == size and call(wbytes=-5) == size
    assert call(stack=FAKE + 4) == align and call(stack=FAKE + 8) == align
    assert call(stride=66) == align and call(col=2, ncols=8) == align
    assert call(center=FAKE + 4) == align and call(work=FAKE + 8) == align and call(out=FAKE + 4) == align
    assert b"aligned" in L.fa_last_error()
    assert call(n=0, stack=FAKE + 4) == arg  # an argument error wins over an alignment error, as for fa_fold


def test_clip_sum_refusals_need_no_gpu(L):
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")

    def call(stack=FAKE, stride=64, n=5, center=FAKE, scale=FAKE, acc=FAKE, col=0, ncols=64):
        rc = L.fa_clip_sum_f32(stack, stride, n, center, scale, acc, col, ncols, None)
        nothing_launched(L)
        return rc

    assert call(stack=None) == arg and call(center=None) == arg and call(scale=None) == arg and call(acc=None) == arg
    assert b"null" in L.fa_last_error()
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error()
    assert call(n=129) == arg and b"128" in L.fa_last_error()
    assert call(n=-1) == arg and call(n=2**31 - 1) == arg
    assert call(ncols=-1) == arg and b"window" in L.fa_last_error()
    assert call(col=-4) == arg and call(col=8, ncols=60) == arg
    big = 2**63 - 1
    assert call(col=big - 3, ncols=8) == arg and call(ncols=big) == arg
    assert call(stack=FAKE + 4) == align and call(stride=66) == align and call(col=2, ncols=8) == align
    assert call(center=FAKE + 8) == align and call(acc=FAKE + 4) == align and call(scale=FAKE + 2) == align
    assert b"aligned" in L.fa_last_error()
    assert call(scale=FAKE + 4, ncols=0) == 0 and call(ncols=0) == 0  # an empty window is a no-op: nothing launched
    assert call(n=0, stack=FAKE + 4) == arg


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


def uploads(n, dtype=np.float32, extra=None):
    rng = np.random.default_rng(n)
    out = []
    for _ in range(n):
        w = {"a.weight": rng.standard_normal((3, 5)).astype(dtype), "a.bias": rng.standard_normal(5).astype(dtype)}
        if extra:
            w.update(extra)
        out.append(w)
    return out


def test_binding_and_import_rule():
    from flearn_amd.aggregator import Aggregator

    assert Aggregator.ensemble_clipped is robustround.ensemble_clipped
    assert Aggregator.last_clip is None
    src = Path(robustround.__file__).read_text()
    assert not re.search(r"^\s*(from|import)\s+[.\w]*\b(aggregator|streaming)\b", src, flags=re.M)
    assert not re.search(r"^\s*from\s+\.\s+import\s+.*\b(aggregator|streaming)\b", src, flags=re.M)


def test_engine_refusals_touch_no_device():
    from flearn_amd.serverstate import DynState

    ups = uploads(7)
    good = {k: np.zeros_like(v) for k, v in ups[0].items()}
    with pytest.raises(ValueError, match="chunk_clients"):
        bare_engine(chunk_clients=4).ensemble_clipped(ups, 1.0, None, center=good)
    with pytest.raises(ValueError, match="group"):
        bare_engine(_dist=True).ensemble_clipped(ups, 1.0, None, center=good)
    with pytest.raises(ValueError, match="one device"):
        bare_engine(devices=[torch.device("cpu")] * 2).ensemble_clipped(ups, 1.0, None, center=good)
    with pytest.raises(TypeError, match="Dyn"):
        bare_engine().ensemble_clipped(ups, 1.0, None, server_opt=object.__new__(DynState), center=good)
    with pytest.raises(ValueError, match="128"):
        bare_engine().ensemble_clipped(uploads(129), 1.0, None, center=good)
    with pytest.raises(TypeError, match="float16"):
        bare_engine().ensemble_clipped(uploads(7, np.float16), 1.0, None, center=good)
    for tau, q in ((None, None), (1.0, 0.5), (0.0, None), (None, 1.5), (True, None), ("1", None)):
        with pytest.raises(ValueError):
            bare_engine().ensemble_clipped(ups, tau, q, center=good)
    with pytest.raises(ValueError, match="fp32 bucket"):
        bare_engine().ensemble_clipped(uploads(7, np.float64), 1.0, None, center=good)
    with pytest.raises(ValueError, match="fp32 bucket"):
        bare_engine().ensemble_clipped([{"n": np.array(3, np.int64)} for _ in range(7)], 1.0, None)
    with pytest.raises(ValueError, match="center"):
        bare_engine().ensemble_clipped(ups, 1.0, None, center=[1, 2])
    with pytest.raises(ValueError, match="center has no key"):
        bare_engine().ensemble_clipped(ups, 1.0, None, center={"a.weight": good["a.weight"]})
    with pytest.raises(ValueError, match="elements"):
        bare_engine().ensemble_clipped(ups, 1.0, None, center=dict(good, **{"a.bias": np.zeros(4, np.float32)}))
    with pytest.raises(AssertionError, match="touched its packer"):  # a good centre gets as far as the pack
        bare_engine().ensemble_clipped(ups, None, 0.5, center=good)


def test_strategy_surface_and_refusals():
    from flearn_amd.strategy import AVG, NormClip

    assert flearn_amd.NormClip is NormClip
    assert "NormClip" in flearn_amd.__all__ and "NormClip" in flearn_amd.strategy.__all__
    assert issubclass(NormClip, AVG) and NormClip.client is AVG.client and NormClip.client_receive is AVG.client_receive
    s = NormClip(tau=2)
    assert (s.tau, s.quantile, s.center, s.server_opt, s.output, s._prev_glob) == (2.0, None, "previous", None, "reference", None)
    s = NormClip(quantile=0.5, output="float32")
    assert (s.tau, s.quantile, s.output) == (None, 0.5, "float32")
    s = flearn_amd.setup_strategy("normclip", None, tau=3.0, output="device")
    assert type(s) is NormClip and (s.tau, s.quantile, s.output) == (3.0, None, "device")
    assert flearn_amd.setup_strategy("NormClip", None, quantile=0.9).quantile == 0.9
    for kw in ({}, {"tau": 1.0, "quantile": 0.5}, {"tau": 0.0}, {"tau": -1.0}, {"tau": math.nan}, {"tau": True},
               {"quantile": 0.0}, {"quantile": 1.01}, {"quantile": "x"}):
        with pytest.raises(ValueError):
            NormClip(**kw)
    with pytest.raises(ValueError, match="centre"):
        NormClip(tau=1.0, center=None)
    with pytest.raises(ValueError, match="center"):
        NormClip(tau=1.0, center="mean")
    with pytest.raises(ValueError, match="begin_round"):
        NormClip(tau=1.0).begin_round(0)
    with pytest.raises(ValueError, match="dict"):
        NormClip(tau=1.0).init_global([1, 2])
    g = {"a": np.ones(3, np.float32), "b": torch.ones(2)}
    s = NormClip(tau=1.0)
    s.init_global(g)
    g["a"][0] = 5.0
    assert s._prev_glob["a"][0] == 1.0 and s._prev_glob["b"] is not g["b"]  # a copy of its own
    assert "agg_weight" in NormClip.__doc__ and "undefended" in NormClip.__doc__.lower()


def test_strategy_errors_take_server_exceptions_route():
    from flearn_amd.strategy import NormClip

    def rounds(n, **kw):
        return [{"agg_weight": 1.0, "params": w} for w in uploads(n, **kw)]

    good = {k: np.zeros_like(v) for k, v in uploads(7)[0].items()}
    for strat, ups in ((NormClip(tau=1.0), rounds(7, dtype=np.float16)),
                       (NormClip(tau=1.0), rounds(7, dtype=np.float64)),  # no fp32 bucket
                       (NormClip(quantile=0.5), rounds(129)),
                       (NormClip(tau=1.0, chunk_clients=4), rounds(7)),
                       (NormClip(tau=1.0), rounds(7, extra={"c": np.zeros(2, np.float32)}))):  # a centre lacking a key
        strat.init_global(good)
        strat._engine = bare_engine(chunk_clients=strat.chunk_clients)
        with pytest.raises(SystemExit):
            strat.server(ups, 0)
        assert set(strat._prev_glob) == set(good)  # the centre is kept
    with pytest.raises(KeyError):  # agg_weight is required (and ignored)
        s = NormClip(tau=1.0)
        s._engine = bare_engine()
        s.server([{"params": w} for w in uploads(7)], 0)
