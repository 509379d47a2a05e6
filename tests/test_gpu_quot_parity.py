"""GPU: the mean's quotient, bit for bit against numpy's float64 divide and float32 cast.

The epilogues divide an fp32 sum by the launch's weight sum d in double.  For a d with a short
significand (fa::recip_quot_exact) the kernels take two fma steps on x * (1/d) instead of the IEEE
divide (fa_numerics.hpp: quot; the proof is in DESIGN.md §2).  Here every fp32 significand goes
through both forms:

  * numerators: all 2^24 significands (the 2^23 hidden-bit-clear ones of the subnormals included),
    both signs, at the exponents {subnormal, -126, 0, 127} (the quotient is scale-invariant in the
    normal range), and +-0, +-inf, NaN;
  * launch: mode W32_DIV64, one client of weight 1.0 (the sum is the numerator itself), window by
    window through the smallest row-major shapes with KG = 3 and KG = 2 and a narrow shape, out32
    alone, and out32 + out64 on the KG = 3 shape;
  * the same with a second client of -0.0 (x + -0.0 == x for every x, -0.0 and NaN included) on the
    row-major shapes: only a launch of two rows or more divides early, under the last row's loads
    (rowmajor_group);
  * denominators: 100, 3, 2^26 + 1, -7 (the reciprocal form), 2^27 + 1 and 0.001 (IEEE divide);
  * the reference: float64(x) / d in numpy, then astype(float32);
  * sentinels between the windows and behind every output must survive."""
import numpy as np
import pytest
import torch

from flearn_amd import _native as na
from flearn_amd import aggregator as agg
from instantiation_cases import chunk_cols, narrow_name, rowmajor_name
from test_gpu_epilogue_values import Windows, _window_stack

pytestmark = pytest.mark.gpu

MODE = na.MODE_W32_DIV64
DENOMS = (100.0, 3.0, 2.0**26 + 1, -7.0, 2.0**27 + 1, 0.001)
# shape -> (forced grid, window width, kernel)
SHAPES = {
    "kg3": (3, chunk_cols(64 * 3 * 2 + 7), rowmajor_name(MODE, 0, False, 3)),
    "kg2": (3, chunk_cols(64 * 3 * 1 + 7), rowmajor_name(MODE, 0, False, 2)),
    # one 1-KiB chunk per block on any chip with at least 64 CUs: the narrow kernel
    "narrow": (0, chunk_cols(48), narrow_name(MODE, 0, 16)),
}
# (shape, out64 too, clients)
RUNS = [("kg3", False, 1), ("kg2", False, 1), ("narrow", False, 1), ("kg3", True, 1), ("kg3", False, 2),
        ("kg2", False, 2)]
CASES = [(d, s, o, n) for d in DENOMS for (s, o, n) in RUNS]  # one denominator's cases in a row: the
#                                                               reference below is kept for the last one only

_STATE = {}


@pytest.fixture
def grid():
    """Sets fa_set_reduce_grid for one test and puts the previous value back."""
    prev = []

    def set_grid(g):
        prev.append(agg.set_reduce_grid(g))

    yield set_grid
    if prev:
        agg.set_reduce_grid(prev[0])


def numerators():
    if "x" not in _STATE:
        mant = np.arange(2**23, dtype=np.uint32)
        parts = [(np.uint32(s) << np.uint32(31)) | (np.uint32(e) << np.uint32(23)) | mant
                 for e in (0, 1, 127, 254) for s in (0, 1)]  # e = 0: the subnormals and +-0
        special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32)
        _STATE["x"] = np.concatenate(parts + [special]).view(np.float32)
    return _STATE["x"]


def reference(denom):
    """float64(x) / denom and its float32 cast, computed once per denominator."""
    if _STATE.get("denom") != denom:
        with np.errstate(all="ignore"):
            q = numerators().astype(np.float64) / np.float64(denom)
            _STATE.update(denom=denom, q64=q, q32=q.astype(np.float32))
    return _STATE["q64"], _STATE["q32"]


def device_stack(width, n_clients, cuda):
    """The numerators as windows of `width` columns (padded with 1.0), built once per (width, clients)."""
    key = ("stack", width, n_clients)
    if key not in _STATE:
        x = numerators()
        nwin = -(-len(x) // width)
        rows = np.full((n_clients, nwin * width), -0.0, np.float32)
        rows[0] = 1.0
        rows[0, : len(x)] = x
        _STATE[key] = (_window_stack(rows, nwin, width, cuda), nwin)
    return _STATE[key]


def same_bits(got, want, int_dtype):
    """On the device: equal bit for bit, or NaN where the reference has NaN."""
    return bool(((got.view(int_dtype) == want.view(int_dtype)) | (got.isnan() & want.isnan())).all())


@pytest.mark.parametrize("denom,shape,with64,n_clients", CASES,
                         ids=[f"d{d:g}-{s}{'-out64' if o else ''}-n{n}" for d, s, o, n in CASES])
def test_quotient_bit_for_bit(denom, shape, with64, n_clients, cuda, grid):
    g, width, kernel = SHAPES[shape]
    grid(g)
    xs, nwin = device_stack(width, n_clients, cuda)
    w = torch.ones(n_clients, dtype=torch.float32, device=cuda)
    out32 = Windows(nwin, width, torch.float32, cuda)
    out64 = Windows(nwin, width, torch.float64, cuda) if with64 else None
    for k in range(nwin):
        agg.reduce_stack(xs, w, MODE, denom, col_begin=k * out32.pitch, n_cols=width, out32=out32.at(k),
                         out64=out64.at(k) if with64 else None)
        if k in (0, nwin - 1):
            name, _, launches = agg.last_launch()
            assert name == kernel and launches == 1, f"window {k}: the shape no longer reaches its kernel: {name}"
    torch.cuda.synchronize()
    q64, q32 = reference(denom)
    m = len(q32)
    got32 = out32._cells(out32.t).reshape(-1)[:m]
    assert same_bits(got32, torch.from_numpy(q32).to(cuda), torch.int32), "out32 differs from float32(float64(x) / d)"
    assert out32.intact(), "out32: written outside a window"
    if with64:
        got64 = out64._cells(out64.t).reshape(-1)[:m]
        assert same_bits(got64, torch.from_numpy(q64).to(cuda), torch.int64), "out64 differs from float64(x) / d"
        assert out64.intact(), "out64: written outside a window"


def test_the_numerator_classes():
    x = numerators()
    bits = x.view(np.uint32)
    assert len(x) == 2**26 + 5
    classes = bits[: 2**26].reshape(8, 2**23)  # (exponent, sign) classes, every significand in each
    assert ((classes & 0x7FFFFF) == np.arange(2**23, dtype=np.uint32)).all()
    assert sorted(set((classes[:, 0] >> 23).tolist())) == [0, 1, 127, 254, 256, 257, 383, 510]
    assert np.isnan(x).sum() == 3 and np.isinf(x).sum() == 2 and (x == 0).sum() == 2
    assert ((np.abs(x) > 0) & (np.abs(x) < np.finfo(np.float32).tiny)).sum() == 2 * (2**23 - 1)
