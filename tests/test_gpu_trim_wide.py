"""GPU: fa_trim_sum_wide (merge_trim_kernel through ops.trim_sum_stack(wide=True)) against the numpy
restatement of the rules (tests/robust_ref.py), bit-exact with NaN positions equal: 129 .. 1024
clients on both sides of every padded depth, ragged widths, windows inside wider rows, several
pieces per block, the special values of the float format, sums that cross the runs' seams, the 8-byte
kinds, and the depths fa_trim_sum serves."""
import numpy as np
import pytest
import torch

import robust_ref as rr
from flearn_amd import _native as na
from flearn_amd import ops

pytestmark = pytest.mark.gpu
SENTINEL = -123456.0


def np_of(n):
    return next(p for p in (256, 512, 1024) if p >= n)


def piece_cols(n):  # plan_trim_wide_window's C: 256 threads, one run of 128 slots each
    return 256 * 128 // np_of(n)


def data(n, width, seed):
    """Mixed magnitudes with ties, signed zeros and a sprinkle of non-finite values."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, width)) * 10.0 ** rng.integers(-4, 5, (n, width))).astype(np.float32)
    for p, v in ((0.05, 0.5), (0.02, -0.0), (0.02, 0.0), (0.01, np.inf), (0.01, -np.inf), (0.01, np.nan)):
        x[rng.random((n, width)) < p] = v
    return x


def run(x, trim, cuda, kind=na.ACC_F32, col_begin=0, n_cols=None, wide=True):
    """The accumulator for the window, with a sentinel tail that must stay untouched."""
    stack = torch.from_numpy(x).to(cuda)
    ncols = x.shape[1] - col_begin if n_cols is None else n_cols
    acc = torch.full((ncols + 8,), SENTINEL, dtype=stack.dtype, device=cuda)
    ops.trim_sum_stack(kind, stack, trim, acc, col_begin=col_begin, n_cols=ncols, wide=wide)
    out = acc.cpu().numpy()
    assert (out[ncols:] == x.dtype.type(SENTINEL)).all(), "wrote past acc_out[0, n_cols)"
    return out[:ncols]


@pytest.mark.parametrize("n", [129, 130, 255, 256, 257, 300, 511, 512, 513, 1000, 1023, 1024])
def test_depths_both_sides_of_every_np(n, cuda):
    x, m = data(n, 100, n), (n - 1) // 2
    for t in (0, 1, m // 2 + 1, m):
        assert rr.same_bits(run(x, t, cuda), rr.trimmed_sum(x, t)), (n, t)
        assert ops.last_launch() == (f"merge_trim_kernel<{np_of(n)},true>", -(-100 // piece_cols(n)), 1)


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("pieces,more", [(0, 1), (1, -1), (1, 0), (1, 1), (2, 1), (0, 1025)])
def test_widths_inside_wider_rows(pieces, more, n, cuda):
    width, t = pieces * piece_cols(n) + more, n // 10
    x = np.full((n, 36 + -(-width // 4) * 4 + 4), np.nan, np.float32)  # a window at column 36 of wider rows
    x[:, 36 : 36 + width] = data(n, width, width)
    got = run(x, t, cuda, col_begin=36, n_cols=width)
    assert rr.same_bits(got, rr.trimmed_sum(x[:, 36 : 36 + width], t))
    assert ops.last_launch()[1] == -(-width // piece_cols(n))


def test_several_pieces_per_block(cuda):
    x, w = data(300, 17 * piece_cols(300), 11), 17 * piece_cols(300) - 3
    prev = ops.set_reduce_grid(3)
    try:
        got = run(x, 30, cuda, n_cols=w)
        assert ops.last_launch()[1] == 3  # 17 pieces on 3 blocks
    finally:
        ops.set_reduce_grid(prev)
    assert rr.same_bits(got, rr.trimmed_sum(x[:, :w], 30))
    assert rr.same_bits(run(x, 30, cuda, n_cols=w), got) and ops.last_launch()[1] == 17


def test_special_values(cuda):
    """test_gpu_trim.py's N = 7 columns between 96 rows of -FLT_MAX and 97 rows of FLT_MAX: N = 200, and
    the kept ranks of t = 95, 98, 99 straddle the seven (those of them that are finite)."""
    nan = [0x7FC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFFFFFFFF, 0xFF800001]  # +-NaN payloads
    inf, ninf, big, tiny, sub = 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000001, 0x807FFFFF
    one, two, three, pz, nz = 0x3F800000, 0x40000000, 0x40400000, 0x00000000, 0x80000000
    cols = [
        [nz] * 7, [pz] * 7, [nz, nz, nz, pz, pz, pz, nz], [pz, nz, pz, nz, pz, nz, pz], [one] * 7, [big] * 7, [sub] * 7,
        [tiny, sub, tiny, sub, pz, nz, tiny], [big, big, big, big, big, one, one], nan,
        [nan[0], nan[1], one, two, three, nan[4], nan[5]], [inf, inf, one, two, three, ninf, ninf],
        [nan[3], inf, one, two, three, ninf, nan[6]], [nan[0], nan[1], nan[2], one, two, nan[4], nan[5]],
        [nan[0], nan[1], one, two, nan[6], nan[4], nan[5]], [inf, inf, inf, one, two, ninf, ninf],
        [inf, inf, one, two, ninf, ninf, ninf], [inf, inf, inf, one, ninf, ninf, ninf], [0x7FFFFFFF] * 7,
        [big, 0xFF7FFFFF, big, 0xFF7FFFFF, one, big, 0xFF7FFFFF],
    ]
    x = np.concatenate([np.full((96, len(cols)), np.finfo(np.float32).min), np.array(cols, np.uint32).view(np.float32).T,
                        np.full((97, len(cols)), np.finfo(np.float32).max)])
    rng = np.random.default_rng(5)
    for perm in (np.arange(200), rng.permutation(200), rng.permutation(200)):
        xp = np.ascontiguousarray(x[perm])
        for t in (95, 98, 99):
            want = rr.trimmed_sum(xp, t)
            assert rr.same_bits(run(xp, t, cuda), want), t
    assert np.signbit(want[0]) and want[0] == 0 and want[4] == 2  # t = 99 kept ranks 99, 100


@pytest.mark.parametrize("n", [300, 1024])
@pytest.mark.parametrize("t", [127, 128, 129])
def test_sum_crosses_the_runs_seams(n, t, cuda):
    """Rows 128 j .. 128 j + 127 hold the value j, permuted: rank r holds r // 128 and the kept sum
    is known in closed form, its first and last terms one rank before, at and after a seam."""
    x = np.repeat((np.arange(n) // 128).astype(np.float32)[:, None], 40, 1)
    x = np.ascontiguousarray(x[np.random.default_rng(t).permutation(n)])
    assert (run(x, t, cuda) == np.float32(sum(r // 128 for r in range(t, n - t)))).all()


def test_float64_and_int64_sums(cuda):
    rng = np.random.default_rng(130)
    x64 = data(130, 72, 41).astype(np.float64) * 1.0000001
    xi = rng.integers(-(2**62), 2**62, (130, 72), dtype=np.int64)  # the sums wrap
    xi[:, :8] = rng.integers(-5, 5, (130, 8))  # ties
    for t in (0, 33, 64):
        assert rr.same_bits(run(x64, t, cuda, kind=na.ACC_F64, n_cols=70), rr.trimmed_sum(x64[:, :70], t)), t
        assert ops.last_launch() == ("trim_kernel_elem<double>", 1, 1)
        assert rr.same_bits(run(xi, t, cuda, kind=na.ACC_I64, n_cols=70), rr.trimmed_sum(xi[:, :70], t)), t
        assert ops.last_launch() == ("trim_kernel_elem<long>", 1, 1)


@pytest.mark.parametrize("n", [100, 128])
def test_depths_of_the_register_sort_take_its_launch(n, cuda):
    x = data(n, 300, n)
    got = run(x, 5, cuda)
    assert ops.last_launch() == ("trim_kernel_rows<128,4,true>", 2, 1)
    assert rr.same_bits(got, run(x, 5, cuda, wide=False)) and rr.same_bits(got, rr.trimmed_sum(x, 5))


def test_python_checks(cuda):
    acc = torch.zeros(64, dtype=torch.float32, device=cuda)
    with pytest.raises(ValueError, match="1024"):
        ops.trim_sum_stack(na.ACC_F32, torch.zeros((1025, 64), dtype=torch.float32, device=cuda), 1, acc, wide=True)
    stack = torch.zeros((300, 64), dtype=torch.float32, device=cuda)
    for t in (150, -1, True):
        with pytest.raises(ValueError, match="trim"):
            ops.trim_sum_stack(na.ACC_F32, stack, t, acc, wide=True)
    with pytest.raises(ValueError):
        ops.trim_sum_stack(na.ACC_F32_W64, stack, 1, acc, wide=True)
    with pytest.raises(TypeError):
        ops.trim_sum_stack(na.ACC_F64, stack, 1, acc, wide=True)
