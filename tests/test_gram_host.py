"""Host-only: plan_gram_window (tests/gram_geometry_probe.cpp against flearn_amd/csrc/fa_geometry.hpp
alone, and its Python restatement tests/gram_ref.py), the ABI 19 surface and fa_gram_f32's refusals
(decided before any HIP call), krum_select against the brute-force restatement (tests/krum_ref.py),
and every refusal of Aggregator.ensemble_krum and the Krum / MultiKrum strategies, raised before the
engine touches a device.  No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import flearn_amd
import gram_ref as gr
import krum_ref as kr
from flearn_amd import _native as na
from flearn_amd import krum

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
HEADER = REPO / "include" / "flearn_amd.h"
CUS = (256, 304, 64)


def header_define(name):
    return int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", HEADER.read_text()).group(1))


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gram_geometry") / "gram_geometry_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "gram_geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(x) for x in f.split()] for f in out]

    return ask


WIDTHS = [1, 63, 64, 65, 127, 128, 129, 257, 511, 512, 513, 1023, 1024, 1025, 4099, 70001, 1 << 20, 25_610_152,
          (1 << 25) - 1, 1 << 25]


@pytest.mark.parametrize("cus", CUS)
def test_plan_gram_window(cus, probe):
    qs = [(n, w) for n in range(1, 129) for w in WIDTHS]
    plans = probe([f"plan {n} {w} {cus} 0" for n, w in qs])
    covers = probe([f"cover {n} {w} {cus} 0" for n, w in qs])
    for (n, w), got, (empty, breaks, widest) in zip(qs, plans, covers):
        np_, kc, lc, chunks, grid, share, chain, work = got
        assert tuple(got) == tuple(gr.plan(n, w, cus)), (n, w)  # the Python restatement the GPU tests use
        assert np_ >= n and np_ % 32 == 0 and np_ - 32 < n and np_ <= 128
        assert kc == {32: 512, 64: 256, 96: 128, 128: 128}[np_] and lc == 1024 and lc % kc == 0
        assert chunks == -(-w // kc) and (chunks - 1) * kc < w <= chunks * kc
        # the blocks' shares cover the window's chunks exactly once, none is empty, none wider than `share`
        assert empty == 0 and breaks == 0 and widest <= share
        assert 1 <= grid <= min(cus, chunks)
        assert work == grid * np_ * np_ * 4
        assert chain == lc + -(-share // lc)
        assert chain <= 8192  # the design condition: cus >= 64 and n_cols <= 2^25 on the natural grid
    if cus == 64:  # the worst case of the condition: 2^25 columns on 64 blocks
        assert max(p[6] for p in plans) == 1024 + (1 << 19) // 1024


def test_forced_grids_are_honoured(probe):
    for cus in CUS:
        got = probe([f"plan 100 25610152 {cus} 7", f"plan 9 4099 {cus} 3", f"plan 9 300 {cus} 3", f"plan 40 1025 {cus} 1",
                     f"plan 128 33554432 {cus} 2"])
        assert [g[4] for g in got] == [7, 3, 1, 1, 2]  # never more blocks than chunks
        assert got[4][6] == 1024 + (1 << 24) // 1024 > 8192  # a forced grid may exceed the condition
        cov = probe([f"cover 100 25610152 {cus} 7", f"cover 9 4099 {cus} 3", f"cover 33 1281 {cus} 3"])
        assert all(c[0] == 0 and c[1] == 0 for c in cov)
    assert [r[0] for r in probe(["plan 0 300 64 0", "plan 129 300 64 0", "plan -1 300 64 0"])] == [0, 0, 0]


# ---------------------------------------------------------------------------------------------
# ABI 19
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def L():
    return na.load()


def test_abi_surface(L):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+fa_gram_f32\s*\(", text) and re.search(r"\bint64_t\s+fa_gram_workspace\s*\(", text)
    for name in ("fa_gram_f32", "fa_gram_workspace"):
        assert name in na.EXPORTS and hasattr(L, name)
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 19
    assert header_define("FA_GRAM_MAX_CLIENTS") == na.GRAM_MAX_CLIENTS == gr.MAX_CLIENTS == 128
    out = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r"\bT\s+fa_gram_f32$", out, flags=re.M) and re.search(r"\bT\s+fa_gram_workspace$", out, flags=re.M)


def test_workspace_is_the_capped_plan(L):
    for n in (1, 32, 33, 64, 65, 100, 128):
        for w in (1, 513, 70001, 25_610_152):
            assert L.fa_gram_workspace(n, w) == gr.workspace_bytes(n, w)
            for cus in CUS + (1024,):  # whatever the device and the forced grid, a launch's partials fit
                for forced in (0, 1, 7, 100000):
                    assert gr.launch_plan(n, w, cus, forced).workspace_bytes <= gr.workspace_bytes(n, w)
    arg = header_define("FA_ERR_ARG")
    assert [L.fa_gram_workspace(n, 64) for n in (0, -1, 129)] == [arg] * 3
    assert L.fa_gram_workspace(5, 0) == arg and L.fa_gram_workspace(5, -7) == arg


FAKE = 0x100000  # never dereferenced: validation rejects the call first


def test_gram_refusals_need_no_gpu(L):
    arg, align, size = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN"), header_define("FA_ERR_SIZE")

    def call(stack=FAKE, stride=64, n=5, center=None, col=0, ncols=64, work=FAKE, wbytes=1 << 26, out=FAKE):
        rc = L.fa_gram_f32(stack, stride, n, center, col, ncols, work, wbytes, out, None)
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0  # nothing was launched
        return rc

    assert call(stack=None) == arg and call(work=None) == arg and call(out=None) == arg
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error()
    assert call(n=-3) == arg
    assert call(n=129) == arg and b"128" in L.fa_last_error()
    assert call(n=2**31 - 1) == arg
    assert call(ncols=0) == arg and b"n_cols" in L.fa_last_error()
    assert call(ncols=-1) == arg
    assert call(col=-4) == arg and call(col=8, ncols=60) == arg  # window > stride
    big = 2**63 - 1  # sums of these would overflow: the window check must not form them
    assert call(col=big - 3, ncols=8) == arg and call(ncols=big) == arg and call(stride=big - 3, col=64, ncols=big) == arg
    assert L.fa_gram_workspace(100, big) == L.fa_gram_workspace(100, 2**40) == 512 * 128 * 128 * 4
    need = L.fa_gram_workspace(5, 64)
    assert call(wbytes=need - 1) == size and str(need).encode() in L.fa_last_error()
    assert call(wbytes=0) == size and call(wbytes=-5) == size
    assert call(stack=FAKE + 4) == align and call(stack=FAKE + 8) == align
    assert call(stride=66) == align and call(col=2, ncols=8) == align
    assert call(center=FAKE + 4) == align and call(work=FAKE + 8) == align and call(out=FAKE + 4) == align
    # an argument error wins over an alignment error, as for fa_fold
    assert call(n=0, stack=FAKE + 4) == arg


# ---------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------


def random_gram(rng, n, kind):
    x = rng.standard_normal((n, 24)) * 10.0 ** rng.integers(-2, 3, (n, 1))
    if kind == "ties":  # duplicate uploads and integer data: equal distances and equal scores
        x = rng.integers(-2, 3, (n, 6)).astype(np.float64)
        x[n // 2] = x[0]
        x[n - 1] = x[1]
    with np.errstate(invalid="ignore", over="ignore"):
        g = x @ x.T
    if kind == "bad":
        for i in rng.choice(n, size=rng.integers(1, 3), replace=False):
            g[i, :] = g[:, i] = rng.choice([np.inf, -np.inf, np.nan])
            g[i, rng.integers(0, n)] = np.nan
    return g


@pytest.mark.parametrize("kind", ["plain", "ties", "bad"])
def test_krum_select_equals_the_brute_force_restatement(kind):
    rng = np.random.default_rng({"plain": 1, "ties": 2, "bad": 3}[kind])
    seen = 0
    for n in (3, 4, 5, 7, 10, 11, 33):
        fs = sorted({0, 1, (n - 3) // 2} & set(range(0, (n - 3) // 2 + 1)))  # f = 0 and N = 2 f + 3 among them
        for f in fs:
            for m in sorted({1, 2, n - f} & set(range(1, n - f + 1))):
                for _ in range(6):
                    g = random_gram(rng, n, kind)
                    try:
                        want_sel, want_sc = kr.select(g, f, m)
                    except ValueError:
                        with pytest.raises(ValueError, match="non-finite"):
                            krum.krum_select(g, f, m)
                        continue
                    sel, sc = krum.krum_select(g, f, m)
                    assert sel.tolist() == want_sel and sel.dtype == np.int64 and len(sel) == m
                    assert sc.dtype == np.float64 and sc.tobytes() == np.array(want_sc, np.float64).tobytes()
                    assert sel.tolist() == sorted(sel.tolist())  # upload order
                    seen += 1
    assert seen > 50


def test_krum_rules_on_a_case_by_hand():
    # points on a line at 0, 1, 2, 10 and a non-finite one; f = 1: each score sums the N - f - 2 = 2 nearest
    x = np.array([[0.0], [1.0], [2.0], [10.0], [np.inf]])
    with np.errstate(invalid="ignore"):
        g = x @ x.T
    d = krum.distances(g)
    assert d[0, 1] == 1 and d[0, 2] == 4 and d[1, 3] == 81 and np.isinf(d[4]).all() and np.isinf(d[:, 4]).all()
    sc = krum.scores(g, 1)
    assert sc.tolist() == [5.0, 2.0, 5.0, 64.0 + 81.0, np.inf]
    assert krum.krum_select(g, 1, 1)[0].tolist() == [1]
    assert krum.krum_select(g, 1, 2)[0].tolist() == [0, 1]  # the tie 0 / 2 goes to the lower index
    assert krum.krum_select(g, 1, 4)[0].tolist() == [0, 1, 2, 3]
    tiny = np.array([[1.0, 1.0 + 1e-17], [1.0 + 1e-17, 1.0]])
    assert (krum.distances(tiny) >= 0).all()  # rounding below zero is clamped
    g[3, :] = g[:, 3] = np.nan  # two bad uploads, f = 1: no 4 finite scores
    with pytest.raises(ValueError, match="non-finite"):
        krum.krum_select(g, 1, 4)
    assert krum.krum_select(g, 1, 3)[0].tolist() == [0, 1, 2]


@pytest.mark.parametrize("n,f,m", [(4, 1, 1), (2, 0, 1), (5, 2, 1), (5, 1, 0), (5, 1, 5), (5, -1, 1), (5, True, 1), (5, 1, True),
                                   (5, 1.0, 1), (5, 1, 2.0), (5, None, 1), (5, 1, None), (5, "1", 1), (5, 1, -1)])
def test_krum_select_argument_errors(n, f, m):
    with pytest.raises(ValueError):
        krum.krum_select(np.eye(n), f, m)
    with pytest.raises(ValueError):
        krum.check_counts(n, f, m)


def test_krum_select_takes_square_matrices_and_numpy_ints():
    with pytest.raises(ValueError):
        krum.krum_select(np.zeros((3, 4)), 0, 1)
    with pytest.raises(ValueError):
        krum.krum_select(np.zeros(9), 0, 1)
    sel, _ = krum.krum_select(np.eye(5), np.int64(1), np.int32(2))
    assert sel.tolist() == [0, 1]
    assert "torch" not in krum.__dict__ and "torch" not in Path(krum.__file__).read_text().split('"""', 2)[2]


# ---------------------------------------------------------------------------------------------
# the engine's and the strategies' refusals: before a device is touched
# ---------------------------------------------------------------------------------------------


class Untouchable:
    """Stands for the packer: any use is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine touched its packer ({name}) before refusing")


def bare_engine(**over):
    from flearn_amd.aggregator import Aggregator

    agg = object.__new__(Aggregator)  # no HIP library, no device
    agg.chunk_clients, agg._dist, agg.devices, agg.output = None, False, [torch.device("cpu")], "reference"
    agg.device, agg.packer, agg.last_plan, agg.last_krum = agg.devices[0], Untouchable(), None, None
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


def test_engine_refusals_touch_no_device():
    from flearn_amd.serverstate import DynState

    ups = uploads(7)
    with pytest.raises(ValueError, match="chunk_clients"):
        bare_engine(chunk_clients=4).ensemble_krum(ups, 1, 3)
    with pytest.raises(ValueError, match="group"):
        bare_engine(_dist=True).ensemble_krum(ups, 1, 3)
    with pytest.raises(ValueError, match="one device"):
        bare_engine(devices=[torch.device("cpu")] * 2).ensemble_krum(ups, 1, 3)
    with pytest.raises(TypeError, match="Dyn"):
        bare_engine().ensemble_krum(ups, 1, 3, server_opt=object.__new__(DynState))
    with pytest.raises(ValueError, match="128"):
        bare_engine().ensemble_krum(uploads(129), 1, 3)
    with pytest.raises(TypeError, match="float16"):
        bare_engine().ensemble_krum(uploads(7, np.float16), 1, 3)
    for f, m in ((3, 1), (-1, 1), (1, 0), (1, 7), (True, 1), (1, True), (1.0, 1), (1, None), ("1", 1)):
        with pytest.raises(ValueError):
            bare_engine().ensemble_krum(ups, f, m)
    with pytest.raises(ValueError, match="fp32 bucket"):
        bare_engine().ensemble_krum(uploads(7, np.float64), 1, 3)
    with pytest.raises(ValueError, match="fp32 bucket"):
        bare_engine().ensemble_krum([{"n": np.array(3, np.int64)} for _ in range(7)], 1, 3)
    with pytest.raises(ValueError, match="center"):
        bare_engine().ensemble_krum(ups, 1, 3, center=[1, 2])
    good = {k: np.zeros_like(v) for k, v in ups[0].items()}
    with pytest.raises(ValueError, match="center has no key"):
        bare_engine().ensemble_krum(ups, 1, 3, center={"a.weight": good["a.weight"]})
    with pytest.raises(ValueError, match="elements"):
        bare_engine().ensemble_krum(ups, 1, 3, center=dict(good, **{"a.bias": np.zeros(4, np.float32)}))
    with pytest.raises(AssertionError, match="touched its packer"):  # a good centre gets as far as the pack
        bare_engine().ensemble_krum(ups, 1, 3, center=good)


def test_strategy_surface_and_refusals():
    from flearn_amd.strategy import AVG, Krum, MultiKrum

    assert flearn_amd.Krum is Krum and flearn_amd.MultiKrum is MultiKrum
    assert "Krum" in flearn_amd.__all__ and "MultiKrum" in flearn_amd.__all__
    assert "Krum" in flearn_amd.strategy.__all__ and "MultiKrum" in flearn_amd.strategy.__all__
    assert issubclass(MultiKrum, AVG) and issubclass(Krum, MultiKrum)
    assert Krum.client is AVG.client and Krum.client_receive is AVG.client_receive
    k = Krum(2)
    assert (k.f, k.m, k.center, k.server_opt, k.output) == (2, 1, "previous", None, "reference")
    assert k.select_count(10) == 1
    mk = MultiKrum(2, output="float32", center=None)
    assert (mk.f, mk.m, mk.center, mk.output) == (2, None, None, "float32") and mk.select_count(10) == 8
    assert MultiKrum(1, 3).select_count(10) == 3
    assert type(flearn_amd.setup_strategy("krum", None, f=1)) is Krum
    s = flearn_amd.setup_strategy("MultiKrum", None, f=2, m=4, center=None, output="device")
    assert type(s) is MultiKrum and (s.f, s.m, s.center, s.output) == (2, 4, None, "device")
    for bad in (-1, True, 1.0, "1", None):
        with pytest.raises(ValueError, match="f must"):
            MultiKrum(bad)
    for bad in (0, -1, True, 2.0, "2"):
        with pytest.raises(ValueError, match="m must"):
            MultiKrum(1, bad)
    with pytest.raises(ValueError, match="center"):
        Krum(1, center="mean")
    with pytest.raises(ValueError, match="begin_round"):
        Krum(1).begin_round(0)
    assert "agg_weight" in Krum.__doc__ and "agg_weight" in MultiKrum.__doc__


def test_strategy_errors_take_server_exceptions_route(capsys):
    from flearn_amd.strategy import Krum, MultiKrum

    def rounds(n, **kw):
        return [{"agg_weight": 1.0, "params": w} for w in uploads(n, **kw)]

    for strat, ups in ((Krum(3), rounds(7)),  # N < 2 f + 3
                       (MultiKrum(1, 7), rounds(7)),  # m > N - f
                       (Krum(1), rounds(7, dtype=np.float16)),
                       (Krum(1), rounds(7, dtype=np.float64)),  # no fp32 bucket
                       (MultiKrum(1, chunk_clients=4), rounds(7))):
        strat._engine = bare_engine(chunk_clients=strat.chunk_clients)
        with pytest.raises(SystemExit):
            strat.server(ups, 0)
        assert strat._prev_glob is None
    with pytest.raises(KeyError):  # agg_weight is required (and ignored)
        s = Krum(1)
        s._engine = bare_engine()
        s.server([{"params": w} for w in uploads(7)], 0)
