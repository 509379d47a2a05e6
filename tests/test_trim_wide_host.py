"""Host-only: the ABI 25 surface of the wide trimmed sums, fa_trim_sum_wide's refusals (decided before
any HIP call, so they need no GPU) and the strategies' `wide` switch."""
import re
from pathlib import Path

import pytest

import flearn_amd
from flearn_amd import _native as na

HEADER = Path(__file__).resolve().parents[1] / "include" / "flearn_amd.h"
FAKE = 0x100000  # never dereferenced: validation rejects the call first


def header_define(name):
    return int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", HEADER.read_text()).group(1))


def test_abi_surface():
    L = na.load()
    assert re.search(r"\bint\s+fa_trim_sum_wide\s*\(", HEADER.read_text())
    assert "fa_trim_sum_wide" in na.EXPORTS and hasattr(L, "fa_trim_sum_wide")
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 25
    assert header_define("FA_TRIM_WIDE_MAX_CLIENTS") == na.TRIM_WIDE_MAX_CLIENTS == 1024
    assert header_define("FA_TRIM_MAX_CLIENTS") == na.TRIM_MAX_CLIENTS == 128


def test_refusals_need_no_gpu():
    L, arg, align = na.load(), header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")

    def call(kind=na.ACC_F32, stack=FAKE, stride=64, n=300, trim=1, acc=FAKE, col=0, ncols=64):
        return L.fa_trim_sum_wide(kind, stack, stride, n, trim, acc, col, ncols, None)

    for kind in (na.ACC_F32_W64, -1, 4):
        assert call(kind=kind) == arg
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error()
    assert call(n=-1) == arg
    assert call(n=1025, trim=3) == arg and b"1024" in L.fa_last_error()
    for n, t in ((300, -1), (300, 150), (1024, 512), (129, 65), (5, 3), (4, 2**30)):
        assert call(n=n, trim=t) == arg and b"trim" in L.fa_last_error(), (n, t)
    assert call(stack=None) == arg and call(acc=None) == arg
    assert call(ncols=-1) == arg and call(col=-4) == arg and call(col=8, ncols=60) == arg  # window > stride
    for kind in (na.ACC_F32, na.ACC_F64, na.ACC_I64):
        for bad in (dict(stack=FAKE + 4), dict(stack=FAKE + 8), dict(acc=FAKE + 8), dict(stride=66), dict(col=2, ncols=8)):
            assert call(kind=kind, **bad) == align, bad
        assert call(kind=kind, ncols=0) == 0  # a no-op, and nothing was launched
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0
    assert call(n=0, stack=FAKE + 4) == arg  # an argument error wins over an alignment error


@pytest.mark.parametrize("name,kw", [("median", {}), ("trimmedmean", {"trim": 3})])
def test_setup_strategy_passes_wide(name, kw):
    s = flearn_amd.setup_strategy(name, None, wide=True, **kw)
    assert s.wide is True and type(s).__name__.lower() == name
    assert flearn_amd.setup_strategy(name, None, **kw).wide is False
