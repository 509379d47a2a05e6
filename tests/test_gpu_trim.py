"""GPU: fa_trim_sum (trim_kernel_rows / trim_kernel_elem through ops.trim_sum_stack) against the
numpy restatement of the rules (tests/robust_ref.py), bit-exact with NaN positions equal — every
padded depth on both sides of its boundary, ragged widths, windows inside wider rows, several
pieces per block, the special values of the float format, the 8-byte sum types."""
import numpy as np
import pytest
import torch

import robust_ref as rr
from flearn_amd import _native as na
from flearn_amd import ops
from instantiation_cases import TRIM_ELEM, trim_rows_name

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128)
SENTINEL = np.float32(-123456.0)


def trims(n):
    m = (n - 1) // 2
    return sorted({0, 1, m, m // 2 + 1} & set(range(0, m + 1)))


def expected_np(n):
    return next(p for p in (4, 8, 16, 32, 64, 128) if p >= n)


def data(n, width, seed):
    """Mixed magnitudes with ties, signed zeros and a sprinkle of non-finite values."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, width)) * 10.0 ** rng.integers(-4, 5, (n, width))).astype(np.float32)
    x[rng.random((n, width)) < 0.05] = np.float32(0.5)  # ties
    x[rng.random((n, width)) < 0.02] = -0.0
    x[rng.random((n, width)) < 0.02] = 0.0
    x[rng.random((n, width)) < 0.01] = np.inf
    x[rng.random((n, width)) < 0.01] = -np.inf
    x[rng.random((n, width)) < 0.01] = np.nan
    return x


def run(stack_np, trim, cuda, kind=na.ACC_F32, col_begin=0, n_cols=None, n_clients=None, tail=8):
    """The kernel's accumulator for the window, with a sentinel tail that must stay untouched."""
    stack = torch.from_numpy(stack_np).to(cuda)
    ncols = stack_np.shape[1] - col_begin if n_cols is None else n_cols
    acc = torch.full((ncols + tail,), float(SENTINEL), dtype=stack.dtype, device=cuda)
    ops.trim_sum_stack(kind, stack, trim, acc, col_begin=col_begin, n_cols=ncols, n_clients=n_clients)
    out = acc.cpu().numpy()
    assert (out[ncols:] == stack_np.dtype.type(SENTINEL)).all(), "wrote past acc_out[0, n_cols)"
    return out[:ncols]


@pytest.mark.parametrize("n", DEPTHS)
def test_depths_both_sides_of_every_np(n, cuda):
    x = data(n, 300, 100 + n)
    for t in trims(n):
        got = run(x, t, cuda)
        assert rr.same_bits(got, rr.trimmed_sum(x, t)), (n, t)
        name, grid, launches = ops.last_launch()
        assert name == trim_rows_name(expected_np(n)) and grid == 2 and launches == 1


def test_trims_cover_the_issue_axis():
    assert trims(1) == [0] and trims(3) == [0, 1] and trims(5) == [0, 1, 2] and trims(9) == [0, 1, 3, 4]
    assert trims(128) == [0, 1, 32, 63]


@pytest.mark.parametrize("width", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_widths(width, cuda):
    stride = -(-width // 4) * 4
    x = np.full((9, stride), np.nan, np.float32)
    x[:, :width] = data(9, width, width)
    got = run(x, 2, cuda, n_cols=width)
    assert rr.same_bits(got, rr.trimmed_sum(x[:, :width], 2))
    assert ops.last_launch()[1] == -(-width // 256)


def test_window_inside_wider_rows(cuda):
    x = data(9, 1088, 7)
    for ncols in (1024, 1000, 301):
        got = run(x, 2, cuda, col_begin=64, n_cols=ncols)
        assert rr.same_bits(got, rr.trimmed_sum(x[:, 64 : 64 + ncols], 2))
    got = run(x, 1, cuda, col_begin=64, n_cols=512, n_clients=5)  # the first rows of a taller stack
    assert rr.same_bits(got, rr.trimmed_sum(x[:5, 64 : 64 + 512], 1))


def test_several_pieces_per_block(cuda):
    x = data(9, 4100, 11)
    prev = ops.set_reduce_grid(3)
    try:
        got = run(x, 2, cuda, n_cols=4099)
        name, grid, _ = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    assert grid == 3 and name == trim_rows_name(16)  # 17 pieces on 3 blocks
    assert rr.same_bits(got, rr.trimmed_sum(x[:, :4099], 2))
    assert rr.same_bits(run(x, 2, cuda, n_cols=4099), got) and ops.last_launch()[1] == 17


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_special_values(cuda):
    """N = 7, t = 2, one column per case: the three kept values are ranks 2, 3, 4 of the totalOrder."""
    nan = [0x7FC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFFFFFFFF, 0xFF800001]  # +-NaN payloads
    inf, ninf, big, tiny, sub = 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000001, 0x807FFFFF
    one, two, three = 0x3F800000, 0x40000000, 0x40400000
    pz, nz = 0x00000000, 0x80000000
    cols = [
        [nz] * 7, [pz] * 7, [nz, nz, nz, pz, pz, pz, nz], [pz, nz, pz, nz, pz, nz, pz],
        [one] * 7, [big] * 7, [sub] * 7, [tiny, sub, tiny, sub, pz, nz, tiny],
        [big, big, big, big, big, one, one],  # fp32 max summed: overflows to inf as the reference's sum does
        nan, [nan[0], nan[1], one, two, three, nan[4], nan[5]],  # exactly t non-finite per side: finite
        [inf, inf, one, two, three, ninf, ninf], [nan[3], inf, one, two, three, ninf, nan[6]],
        [nan[0], nan[1], nan[2], one, two, nan[4], nan[5]],  # t + 1 at the top: NaN
        [nan[0], nan[1], one, two, nan[6], nan[4], nan[5]],  # t + 1 at the bottom: NaN
        [inf, inf, inf, one, two, ninf, ninf], [inf, inf, one, two, ninf, ninf, ninf],  # +inf / -inf
        [inf, inf, inf, one, ninf, ninf, ninf],  # inf + -inf among the kept: NaN
        [0x7FFFFFFF] * 7,  # the padding key itself as data
        [big, 0xFF7FFFFF, big, 0xFF7FFFFF, one, big, 0xFF7FFFFF],
    ]
    x = np.zeros((7, 64), np.float32)
    x[:, : len(cols)] = f32(cols).T
    rng = np.random.default_rng(5)
    for perm in (np.arange(7), rng.permutation(7), rng.permutation(7)):
        xp = np.ascontiguousarray(x[perm])
        for t in (2, 0, 3):
            want = rr.trimmed_sum(xp, t)
            got = run(xp, t, cuda)
            assert rr.same_bits(got, want), (t, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)))
    want = rr.trimmed_sum(x, 2)[: len(cols)]
    assert np.signbit(want[0]) and want[0] == 0 and not np.signbit(want[1])
    assert np.isfinite(want[[10, 11, 12]]).all() and (want[[10, 11, 12]] == 6.0).all()
    assert np.isnan(want[[9, 13, 14, 17, 18]]).all() and want[15] == np.inf and want[16] == -np.inf and want[8] == np.inf


@pytest.mark.parametrize("n", [1, 4, 10])
def test_float64_and_int64_sums(n, cuda):
    rng = np.random.default_rng(n)
    x64 = data(n, 72, 40 + n).astype(np.float64) * 1.0000001
    x64[:, 3] = -0.0
    xi = rng.integers(-(2**62), 2**62, (n, 72), dtype=np.int64)  # sums of more than two wrap
    xi[:, :8] = rng.integers(-5, 5, (n, 8))  # ties
    xi[:, 9] = np.iinfo(np.int64).max
    for t in trims(n):
        got = run(x64, t, cuda, kind=na.ACC_F64, n_cols=70)
        assert rr.same_bits(got, rr.trimmed_sum(x64[:, :70], t)), ("f64", n, t)
        assert ops.last_launch() == (TRIM_ELEM[na.ACC_F64], 1, 1)
        got = run(xi, t, cuda, kind=na.ACC_I64, n_cols=70)
        assert rr.same_bits(got, rr.trimmed_sum(xi[:, :70], t)), ("i64", n, t)
        assert ops.last_launch() == (TRIM_ELEM[na.ACC_I64], 1, 1)
    if n == 10:
        assert (np.abs(xi[:, 10:].astype(np.float64)).sum(0) > 2.0**63).any()  # the int64 sums did wrap


@pytest.mark.parametrize("n,np_", [(4, 4), (5, 8), (17, 32), (100, 128)])
def test_instantiation_named_by_last_launch(n, np_, cuda):
    x = data(n, 64, n)
    run(x, 0, cuda)
    assert ops.last_launch() == (trim_rows_name(np_), 1, 1)


def test_finish_gives_the_trimmed_mean(cuda):
    """fa_fold_finish over the accumulator with denom = N - 2t: the float64 and fp32 results."""
    x = data(9, 300, 3)
    stack = torch.from_numpy(x).to(cuda)
    acc = torch.empty(300, dtype=torch.float32, device=cuda)
    ops.trim_sum_stack(na.ACC_F32, stack, 2, acc)
    out64 = torch.empty(300, dtype=torch.float64, device=cuda)
    out32 = torch.empty(300, dtype=torch.float32, device=cuda)
    ops.fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc, 5.0, 300, out32=out32, out64=out64)
    assert rr.same_bits(out64.cpu().numpy(), rr.trimmed_mean(x, 2))
    assert rr.same_bits(out32.cpu().numpy(), rr.trimmed_mean_f32(x, 2))


def test_python_checks(cuda):
    stack = torch.zeros((5, 64), dtype=torch.float32, device=cuda)
    acc = torch.zeros(64, dtype=torch.float32, device=cuda)
    with pytest.raises(ValueError, match="trim"):
        ops.trim_sum_stack(na.ACC_F32, stack, 3, acc)
    with pytest.raises(ValueError, match="trim"):
        ops.trim_sum_stack(na.ACC_F32, stack, -1, acc)
    with pytest.raises(ValueError):
        ops.trim_sum_stack(na.ACC_F32_W64, stack, 1, acc)
    with pytest.raises(TypeError):
        ops.trim_sum_stack(na.ACC_F64, stack, 1, acc)
    with pytest.raises(ValueError, match="acc_out"):
        ops.trim_sum_stack(na.ACC_F32, stack, 1, acc[:60])
    with pytest.raises(ValueError, match="128"):
        ops.trim_sum_stack(na.ACC_F32, torch.zeros((129, 64), dtype=torch.float32, device=cuda), 1, acc)
    with pytest.raises(ValueError, match="window"):
        ops.trim_sum_stack(na.ACC_F32, stack, 1, acc, col_begin=32, n_cols=64)
