"""Host-only: the robust aggregation rules' numpy restatement (tests/robust_ref.py), the ABI 18
surface and fa_trim_sum's refusals (decided before any HIP call), plan_trim_window and the sorting
network (tests/trim_geometry_probe.cpp against flearn_amd/csrc/fa_geometry.hpp alone), and the
strategies' surface.  No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flearn_amd
import robust_ref as rr
from flearn_amd import _native as na

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
HEADER = REPO / "include" / "flearn_amd.h"
CUS = (256, 304, 64)
DEPTHS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128)


def header_define(name):
    return int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", HEADER.read_text()).group(1))


# ---------------------------------------------------------------------------------------------
# robust_ref pinning
# ---------------------------------------------------------------------------------------------


def test_ref_equals_plain_sort_on_finite_data():
    """Without NaN and +-0 ties the totalOrder sort is np.sort, and the sum is sequential."""
    rng = np.random.default_rng(1)
    for n, t in ((1, 0), (4, 1), (7, 2), (10, 0), (10, 4), (33, 5)):
        x = (rng.standard_normal((n, 257)) * 10.0 ** rng.integers(-3, 4, (n, 257))).astype(np.float32)
        x[x == 0] = 1.0
        kept = np.sort(x, 0)[t : n - t]
        acc = kept[0].copy()
        for row in kept[1:]:
            acc = acc + row
        assert acc.dtype == np.float32
        assert rr.trimmed_sum(x, t).tobytes() == acc.tobytes()
        assert rr.trimmed_mean(x, t).tobytes() == (acc.astype(np.float64) / np.float64(n - 2 * t)).tobytes()
        assert rr.trimmed_mean(x, t).dtype == np.float64
        x64 = x.astype(np.float64) * 1.1
        kept = np.sort(x64, 0)[t : n - t]
        acc = kept[0].copy()
        for row in kept[1:]:
            acc = acc + row
        assert rr.trimmed_mean(x64, t).tobytes() == (acc / np.float64(n - 2 * t)).tobytes()


def test_ref_median_is_numpys():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 4, 9, 10):
        x = rng.standard_normal((n, 300)).astype(np.float32)
        got = rr.median(x)
        if n % 2:
            assert got.tobytes() == np.median(x, axis=0).astype(np.float64).tobytes()  # one kept value: exact
        else:  # numpy's mean of the two middle fp32 values: an fp32 sum, then a divide by 2 (exact)
            assert got.astype(np.float32).tobytes() == np.median(x, axis=0).tobytes()
    assert rr.median_trim(1) == 0 and rr.median_trim(2) == 0 and rr.median_trim(9) == 4 and rr.median_trim(10) == 4


def test_ref_total_order_and_signed_zero():
    nan_p, nan_n = np.uint32(0x7FC00001).view(np.float32), np.uint32(0xFFC00000).view(np.float32)
    vals = np.array([nan_p, np.inf, 3.0, 0.0, -0.0, -1e-45, -np.inf, nan_n], np.float32)
    s = rr.sorted_columns(vals[::-1].reshape(-1, 1))[:, 0]
    assert s.view(np.uint32).tolist() == vals[::-1].view(np.uint32).tolist()
    k = rr.total_order_keys(vals)
    assert rr.keys_to_values(k, np.float32).tobytes() == vals.tobytes()  # an involution on the bits
    allneg = np.full((5, 3), -0.0, np.float32)
    for t in (0, 1, 2):  # the first kept value initialises the sum: -0.0 stays -0.0
        assert np.signbit(rr.trimmed_sum(allneg, t)).all() and np.signbit(rr.trimmed_mean(allneg, t)).all()
    mixed = np.array([[-0.0], [0.0], [-0.0]], np.float32)  # sorted: -0 -0 +0; the median is -0
    assert np.signbit(rr.median(mixed)).all() and not np.signbit(rr.trimmed_mean(mixed, 0)).any()
    i = np.array([[2**62], [2**62], [5], [-7], [2**62]], np.int64)
    assert rr.trimmed_sum(i, 0).dtype == np.int64
    assert int(rr.trimmed_sum(i, 0)[0]) == 3 * 2**62 - 2 - 2**64  # wraps as numpy's int64 does
    assert int(rr.trimmed_sum(i, 1)[0]) == 5 + 2**63 - 2**64 and int(rr.trimmed_sum(i, 2)[0]) == 2**62
    with pytest.raises(ValueError):
        rr.trimmed_sum(i, 3)


def test_ref_permutation_invariance():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((9, 500)).astype(np.float32)
    x[rng.integers(0, 9, 60), rng.integers(0, 500, 60)] = np.nan
    x[rng.integers(0, 9, 60), rng.integers(0, 500, 60)] = np.inf
    x[rng.integers(0, 9, 60), rng.integers(0, 500, 60)] = -0.0
    for t in (0, 2, 4):
        want = rr.trimmed_mean(x, t)
        for _ in range(4):
            assert rr.same_bits(rr.trimmed_mean(x[rng.permutation(9)], t), want)
    assert not rr.same_bits(np.array([np.nan, 1.0]), np.array([1.0, 1.0]))
    assert rr.same_bits(np.array([np.nan, -0.0]), np.array([-np.nan, -0.0]))
    assert not rr.same_bits(np.array([0.0]), np.array([-0.0]))


# ---------------------------------------------------------------------------------------------
# ABI 18
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def L():
    return na.load()


def test_abi_surface(L):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+fa_trim_sum\s*\(", text)
    assert "fa_trim_sum" in na.EXPORTS and hasattr(L, "fa_trim_sum")
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 18
    assert header_define("FA_TRIM_MAX_CLIENTS") == na.TRIM_MAX_CLIENTS == 128
    out = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r"\bT\s+fa_trim_sum$", out, flags=re.M)


FAKE = 0x100000  # never dereferenced: validation rejects the call first


def test_trim_sum_refusals_need_no_gpu(L):
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")

    def call(kind=na.ACC_F32, stack=FAKE, stride=64, n=5, trim=1, acc=FAKE, col=0, ncols=64):
        return L.fa_trim_sum(kind, stack, stride, n, trim, acc, col, ncols, None)

    for kind in (na.ACC_F32_W64, -1, 4, 99):
        assert call(kind=kind) == arg
    assert call(n=0) == arg and b"n_clients" in L.fa_last_error()
    assert call(n=-3) == arg
    assert call(n=129, trim=3) == arg and b"128" in L.fa_last_error()
    assert call(n=2**31 - 1, trim=3) == arg
    assert call(trim=-1) == arg and b"trim" in L.fa_last_error()
    for n, t in ((1, 1), (2, 1), (5, 3), (128, 64), (4, 2**30)):
        assert call(n=n, trim=t) == arg, (n, t)
    assert call(stack=None) == arg and call(acc=None) == arg
    assert call(ncols=-1) == arg and call(col=-4) == arg and call(col=8, ncols=60) == arg  # window > stride
    for kind in (na.ACC_F32, na.ACC_F64, na.ACC_I64):
        assert call(kind=kind, stack=FAKE + 4) == align
        assert call(kind=kind, stack=FAKE + 8) == align
        assert call(kind=kind, acc=FAKE + 8) == align
        assert call(kind=kind, stride=66) == align
        assert call(kind=kind, col=2, ncols=8) == align
        assert call(kind=kind, ncols=0) == 0  # a no-op, and nothing was launched
        rec = na.LaunchRecord()
        assert L.fa_last_launch(rec) == 0 and rec.kernel is None and rec.launches == 0
    # an argument error wins over an alignment error, as for fa_fold
    assert call(n=0, stack=FAKE + 4) == arg


# ---------------------------------------------------------------------------------------------
# geometry and the sorting network
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("trim_geometry") / "trim_geometry_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "trim_geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(x) for x in f.split()] for f in out]

    return ask


def expected_np(n):
    return next(p for p in (4, 8, 16, 32, 64, 128) if p >= n)


@pytest.mark.parametrize("cus", CUS)
def test_plan_trim_window(cus, probe):
    widths = [1, 255, 256, 257, 1025, 4099, 256 * cus * 8, 256 * cus * 8 + 1, 25_610_152]
    qs = [(n, w) for n in DEPTHS for w in widths]
    for (n, w), (np_, pieces, grid, waves, elem) in zip(qs, probe([f"plan {n} {w} {cus} 0" for n, w in qs])):
        assert np_ == expected_np(n) and np_ >= n and (np_ == 4 or np_ // 2 < n)
        # cover: piece p is columns [256 p, 256 (p + 1)) cut at the window's end; block b takes
        # pieces b, b + grid, ...: every piece, so every column, is exactly one block's
        assert pieces == -(-w // 256) and (pieces - 1) * 256 < w <= pieces * 256
        if pieces <= 4096:
            assert sorted(p for b in range(grid) for p in range(b, pieces, grid)) == list(range(pieces))
        # the grid: one block per piece up to the blocks resident at once for this depth
        assert waves == (2 if np_ == 128 else 4 if np_ == 64 else 8)
        assert grid == min(pieces, cus * waves) and 1 <= grid
        assert elem == min(-(-w // 256), 4 * cus)
    # fa_set_reduce_grid applies, never more blocks than pieces
    assert [r[2] for r in probe([f"plan 9 4099 {cus} 3", f"plan 9 300 {cus} 3", f"plan 100 25610152 {cus} 7"])] == [3, 2, 7]
    assert probe([f"plan 9 10000000 {cus} 5"])[0][4] == 5
    # out of range: no instantiation
    assert [r[0] for r in probe([f"plan 0 300 {cus} 0", f"plan 129 300 {cus} 0", f"plan -1 300 {cus} 0"])] == [0, 0, 0]


def test_sorting_network_sorts(probe):
    """Batcher's odd-even merge sort as trim_net_pair lays it out: exhaustive 0/1 inputs up to 16
    slots, random keys with ties and padding at every depth; the exchange counts are Batcher's."""
    got = probe([f"net {p} {p} 400" for p in (4, 8, 16, 32, 64, 128)])
    assert [g[1] for g in got] == [0] * 6
    assert [g[0] for g in got] == [5, 19, 63, 191, 543, 1471]


# ---------------------------------------------------------------------------------------------
# strategies
# ---------------------------------------------------------------------------------------------


def test_strategy_surface():
    from flearn_amd.strategy import AVG, Median, TrimmedMean

    assert flearn_amd.TrimmedMean is TrimmedMean and flearn_amd.Median is Median
    assert "TrimmedMean" in flearn_amd.__all__ and "Median" in flearn_amd.__all__
    assert issubclass(TrimmedMean, AVG) and issubclass(Median, TrimmedMean)
    assert TrimmedMean.client is AVG.client and TrimmedMean.client_receive is AVG.client_receive
    s = flearn_amd.setup_strategy("trimmedmean", None)
    assert type(s) is TrimmedMean and s.trim == 0.1 and s.server_opt is None and s.output == "reference"
    s = flearn_amd.setup_strategy("TrimmedMean", None, trim=2, output="float32")
    assert s.trim == 2 and s.output == "float32" and s.trim_count(10) == 2 and s.trim_count(100) == 2
    assert type(flearn_amd.setup_strategy("median", None)) is Median
    assert [flearn_amd.Median().trim_count(n) for n in (1, 2, 3, 4, 9, 10, 128)] == [0, 0, 1, 1, 4, 4, 63]
    t = TrimmedMean(0.2)
    assert [t.trim_count(n) for n in (1, 4, 5, 9, 10, 100)] == [0, 0, 1, 1, 2, 20]
    assert TrimmedMean().trim == 0.1 and TrimmedMean(0.0).trim_count(7) == 0 and TrimmedMean(0.49).trim_count(100) == 49
    assert "agg_weight" in TrimmedMean.__doc__ and "agg_weight" in Median.__doc__


@pytest.mark.parametrize("bad", [0.5, 0.75, -0.1, float("nan"), float("inf"), -1, True, "0.1", None, [1]])
def test_trim_is_validated_at_construction(bad):
    with pytest.raises(ValueError, match="trim"):
        flearn_amd.TrimmedMean(bad)
