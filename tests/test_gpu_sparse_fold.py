"""GPU: ops.sparse_fold_stack (fa_sparse_fold_f32) against tests/sparse_ref.py, bit for bit.  The rows are
fixed by hand around the kernel's seams: an empty row, a single entry, entries at w0 - 1, w0 and w0 + WC - 1
of every window, runs of more than 64 and more than 128 consecutive entries in one window, a column every
row holds (values whose sum depends on the order), a column whose sum stays denormal, +-inf and NaN, and
entries outside the launch's window."""
import numpy as np
import pytest
import torch

import sparse_ref as ref
from flearn_amd import _native as na
from flearn_amd import ops

pytestmark = pytest.mark.gpu

WC = na.SPARSE_WINDOW
D = 8  # rows in flight; test_natural_and_forced_grids pins it to the kernel's name
KERNEL = f"window_fold_kernel<{WC},{D},4>"
ORDER = [2.0 ** 24, 1.0, -(2.0 ** 24), 1.0, 3.0, -0.5]  # fl32(2^24 + 1) = 2^24: another order, other bits


def hand_rows(n, ncols, cb):
    """n rows over the bucket columns [cb - 1, cb + ncols]; (rows, weights)."""
    end = cb + ncols
    rows = []
    for i in range(n):
        e = {}
        if i != 1:  # row 1 is empty
            e[cb] = ORDER[i % len(ORDER)]  # the column every row holds
            if ncols > 1:
                e[cb + 1] = 2.0 ** -140 * (i + 1)  # products and sums are denormal
        if i == 2:
            e = {cb + min(ncols - 1, WC): 7.0}  # a single entry
        if i in (0, n - 1) and i not in (1, 2):
            for w0 in range(cb + WC, end, WC):  # every window seam inside the launch
                for c in (w0 - 1, w0, w0 + WC - 1):
                    if c < end:
                        e[c] = 1.5 + i
            e.update({c: 0.25 * (c - cb) for c in range(cb + 10, min(end, cb + 10 + 200))})  # > 128 in window 0
            e.update({c: -1.0 - i for c in range(cb + WC + 5, min(end, cb + WC + 5 + 70))})  # > 64 in window 1
            if cb:
                e[cb - 1] = 99.0  # below the window: dropped
            e[end] = 99.0  # past it: dropped
            if ncols > 5:
                e[cb + 3], e[cb + 5] = (np.inf, np.nan) if i == 0 else (-np.inf, 1.0)
        for t in range(12 if i not in (1, 2) else 0):
            e.setdefault(cb + (i * 37 + 101 * t * t) % ncols, 0.01 * (t + 1) - 0.05 * i)
        cols = np.array(sorted(e), np.uint32)
        rows.append((cols, np.array([e[int(c)] for c in cols], np.float32)))
    return rows, [0.5, 1.0, 2.25, 0.125, 3.0, 1.0, 0.75][:n] + [1.0 + 0.25 * j for j in range(max(0, n - 7))]


def run(rows, weights, ncols, cb, center=None, wsum=0.0, acc_in=None, dev="cuda"):
    acc = torch.full((ncols,), 123.0, dtype=torch.float32, device=dev)
    ops.sparse_fold_stack(torch.from_numpy(ref.pairs(rows).view(np.int32)).to(dev), torch.tensor(weights, dtype=torch.float32, device=dev),
                          None if acc_in is None else torch.from_numpy(acc_in).to(dev), acc,
                          center=None if center is None else torch.from_numpy(center).to(dev), wsum=wsum, col_begin=cb)
    return acc.cpu().numpy()


def centre_of(ncols, cb):
    return (np.random.default_rng(5).standard_normal(cb + ncols) * 3).astype(np.float32)


@pytest.mark.parametrize("cb", [0, 8])
@pytest.mark.parametrize("with_center", [False, True])
@pytest.mark.parametrize("ncols", [1, WC - 1, WC, WC + 1, 3 * WC + 5])
@pytest.mark.parametrize("n", [1, 3, D + 1, 2 * D + 3])
def test_fold_is_the_rule_bit_for_bit(n, ncols, with_center, cb, cuda):
    rows, w = hand_rows(n, ncols, cb)
    g = centre_of(ncols, cb) if with_center else None
    want = ref.fold(rows, w, ncols, cb, g, 6.625)
    assert ref.same_bits(run(rows, w, ncols, cb, g, 6.625), want)
    assert ops.last_launch() == (KERNEL, 1, 2)  # at most four windows: one block; the bounds launch and the fold
    if ncols > 9:  # inf and NaN touch only their own columns
        assert np.isnan(want[5]) and not np.isfinite(want[3]) and np.isfinite(want[6:9]).all()


@pytest.mark.parametrize("with_center", [False, True])
def test_rows_chained_through_acc_in_leave_one_launch_s_bits(with_center, cuda):
    n, ncols, cb = 2 * D + 3, WC + 77, 8
    rows, w = hand_rows(n, ncols, cb)
    g = centre_of(ncols, cb) if with_center else None
    first = run(rows[: D + 2], w[: D + 2], ncols, cb, g, 2.5)
    both = run(rows[D + 2 :], w[D + 2 :], ncols, cb, None, 0.0, acc_in=first)
    assert ref.same_bits(both, run(rows, w, ncols, cb, g, 2.5)) and ref.same_bits(both, ref.fold(rows, w, ncols, cb, g, 2.5))


def test_natural_and_forced_grids_give_the_same_bits(cuda):
    n, ncols = 2 * D + 3, 13 * WC + 5  # 14 windows: four blocks of four waves
    rows, w = hand_rows(n, ncols, 0)
    want = ref.fold(rows, w, ncols)
    assert ref.same_bits(run(rows, w, ncols, 0), want) and ops.last_launch() == (KERNEL, 4, 2)
    for grid in (1, 3):
        prev = ops.set_reduce_grid(grid)
        try:
            got = run(rows, w, ncols, 0)
            assert ops.last_launch() == (KERNEL, grid, 2)
        finally:
            ops.set_reduce_grid(prev)
        assert ref.same_bits(got, want)
