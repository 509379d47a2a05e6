"""Host-only: the ABI 30 surface of the wide Gram matrix, fa_gram_f32_wide's refusals (decided before any
HIP call, so they need no GPU), plan_gram_wide (tests/gram_wide_geometry_probe.cpp against
flearn_amd/csrc/fa_gramwide_geometry.hpp, and its Python restatement tests/gram_wide_ref.py) and the Krum
strategies' `wide` switch."""
import re
import subprocess
from pathlib import Path

import pytest

import flearn_amd
import gram_wide_ref as gw
from flearn_amd import _build
from flearn_amd import _native as na

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
HEADER = REPO / "include" / "flearn_amd.h"
FAKE = 0x100000  # never dereferenced: validation rejects the call first
NS = (1, 128, 129, 160, 257, 1000, 1024)
WIDTHS = (1, 63, 64, 65, 1023, 2053, 4099, 70001, 4_194_304, 1 << 25)


def header_define(name):
    return int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", HEADER.read_text()).group(1))


@pytest.fixture(scope="module")
def L():
    return na.load()


def test_abi_surface(L):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+fa_gram_f32_wide\s*\(", text) and re.search(r"\bint64_t\s+fa_gram_wide_workspace\s*\(", text)
    exported = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ("fa_gram_f32_wide", "fa_gram_wide_workspace"):
        assert name in na.EXPORTS and hasattr(L, name) and re.search(rf"\bT\s+{name}$", exported, flags=re.M)
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 30
    assert header_define("FA_GRAM_WIDE_MAX_CLIENTS") == na.GRAM_WIDE_MAX_CLIENTS == gw.MAX_CLIENTS == 1024
    assert header_define("FA_GRAM_MAX_CLIENTS") == na.GRAM_MAX_CLIENTS == 128
    assert CSRC / "fa_gramwide.hip" in _build.SOURCES


def test_refusals_need_no_gpu(L):
    arg, align, size = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN"), header_define("FA_ERR_SIZE")

    def call(stack=FAKE, stride=64, n=300, center=None, col=0, ncols=64, work=FAKE, wbytes=1 << 28, out=FAKE):
        rc = L.fa_gram_f32_wide(stack, stride, n, center, col, ncols, work, wbytes, out, None)
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0  # nothing was launched
        return rc

    for n in (300, 5):  # past 128 clients, and the depths handed to fa_gram_f32: the same refusals
        assert call(n=n, stack=None) == arg and call(n=n, work=None) == arg and call(n=n, out=None) == arg
        assert call(n=n, ncols=0) == arg and b"n_cols" in L.fa_last_error()
        assert call(n=n, ncols=-1) == arg
        assert call(n=n, col=-4) == arg and call(n=n, col=8, ncols=60) == arg  # window > stride
        big = 2**63 - 1  # sums of these would overflow: the window check must not form them
        assert call(n=n, col=big - 3, ncols=8) == arg and call(n=n, ncols=big) == arg
        need = L.fa_gram_wide_workspace(n, 64)
        assert call(n=n, wbytes=need - 1) == size and str(need).encode() in L.fa_last_error()
        assert call(n=n, wbytes=0) == size
        assert call(n=n, stack=FAKE + 4) == align and call(n=n, stride=66) == align and call(n=n, col=2, ncols=8) == align
        assert call(n=n, center=FAKE + 4) == align and call(n=n, work=FAKE + 8) == align and call(n=n, out=FAKE + 4) == align
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error()
    assert call(n=-3) == arg and call(n=2**31 - 1) == arg
    assert call(n=1025) == arg and b"1024" in L.fa_last_error()
    assert call(n=0, stack=FAKE + 4) == arg  # an argument error wins over an alignment error
    assert [L.fa_gram_wide_workspace(n, 64) for n in (0, -1, 1025)] == [arg] * 3
    assert L.fa_gram_wide_workspace(300, 0) == arg and L.fa_gram_wide_workspace(300, -7) == arg


def test_workspace_is_monotone_and_enough_for_every_forced_grid(L):
    for n in (129, 160, 257, 1000, 1024):
        sizes = [L.fa_gram_wide_workspace(n, w) for w in WIDTHS + (2**40, 2**63 - 1)]
        assert sizes == sorted(sizes) and sizes[-1] == gw.UNIT_CAP * gw.SLOT
        assert sizes[: len(WIDTHS)] == [gw.workspace_bytes(n, w) for w in WIDTHS]
        for w, need in zip(WIDTHS, sizes):
            for cus in (64, 256, 304, 4096):
                for forced in (0, 1, 7, 100000):
                    assert gw.launch_plan(n, w, cus, forced).workspace_bytes <= need, (n, w, cus, forced)
    for w in WIDTHS:  # never smaller for more clients, the depths fa_gram_workspace answers included
        sizes = [L.fa_gram_wide_workspace(n, w) for n in (1, 100, 128, 129, 256, 257, 384, 385, 640, 897, 1024)]
        assert sizes == sorted(sizes)
        assert sizes[:3] == [L.fa_gram_workspace(n, w) for n in (1, 100, 128)]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gram_wide_geometry") / "gram_wide_geometry_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "gram_wide_geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join("%d %d %d %d\n" % q for q in queries), capture_output=True,
                             text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(x) for x in line.split()] for line in out]

    return ask


@pytest.mark.parametrize("cus,forced", [(256, 0), (304, 0), (64, 0), (256, 1), (256, 7), (256, 100000)])
def test_plan_gram_wide(cus, forced, probe):
    qs = [(n, w, cus, forced) for n in NS for w in WIDTHS]
    for (n, w, _, _), got in zip(qs, probe(qs)):
        *plan, sized, empty, breaks, widest = got
        tiles, panels, pairs, kc, lc, chunks, slices, share, chain, work = plan
        assert tuple(plan) == tuple(gw.plan(n, w, cus, forced)), (n, w)  # the restatement the GPU tests use
        assert tiles == -(-n // 32) and panels == -(-n // 128) <= 8 and pairs == panels * (panels + 1) // 2 <= 36
        assert kc == 64 and lc == 1024 and chunks == -(-w // kc)
        # every pair takes every slice: the slices cover the chunks exactly once, none is empty or wider than `share`
        assert empty == 0 and breaks == 0 and widest <= share
        assert 1 <= slices <= chunks and slices * pairs <= 2048 and (forced == 0 or slices == min(forced, 2048 // pairs, chunks))
        assert chain == lc + -(-share // lc) and work == slices * pairs * 65536 <= sized == gw.workspace_bytes(n, w)
        if forced == 0 and cus >= 64 and w <= 1 << 25:
            assert chain <= 8192  # section 13's design condition holds on the natural grid
    assert [r[0] for r in probe([(0, 300, 64, 0), (1025, 300, 64, 0), (-1, 300, 64, 0)])] == [0, 0, 0]


@pytest.mark.parametrize("name", ["krum", "multikrum"])
def test_setup_strategy_passes_wide(name):
    s = flearn_amd.setup_strategy(name, None, f=1, wide=True)
    assert s.wide is True and type(s).__name__.lower() == name
    assert flearn_amd.setup_strategy(name, None, f=1).wide is False
    assert flearn_amd.Krum(1, None, "previous", None, "float32").output == "float32"  # positional callers are unaffected
