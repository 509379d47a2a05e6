"""GPU: fa_deq_fold_q1 (ops.deq_fold_q1_stack) against tests/quant1_ref.py's row-by-row restatement, bit
for bit where the reference is not NaN and NaN where it is: windows around the load, the scale block, the
chunk and the piece inside wider rows of garbage, row counts around the pipeline depth, forced grids under
which one block sweeps several pieces, chains through acc_in, and a centre."""
import numpy as np
import pytest
import torch

import quant1_ref as q1r
from flearn_amd import ops

pytestmark = pytest.mark.gpu

C = q1r.CHUNK
PIECE = q1r.PIECE_CHUNKS * C + C + 5  # a full piece, a chunk and 5 columns: a short last piece under any grid
WIDTHS = (1, 31, 33, 127, 129, 2047, 2049, PIECE)
COLS = 7 * C  # a row: the widest window behind a col_begin of 2048, and a chunk of garbage more
ROWS = (1, 2, q1r.D, 2 * q1r.D + 1, 100)
GUARD = 64  # columns past a window in its accumulator: they hold 7.0 and must stay
SPECIAL = np.array([0.0, -0.0, 1e-45, 1.0, 2.0 ** 100], dtype=np.float32)


@pytest.fixture(scope="module")
def data(cuda):
    """[100, COLS / 8] random bytes, scales per (row, block) log-uniform over 2^+-20 with SPECIAL drawn into
    a fifth of them, weights with 2^30 (times 2^100: inf), -1, 0 and -0.0 forced in, a centre with two NaNs."""
    rng = np.random.default_rng(43)
    q1 = rng.integers(0, 256, (max(ROWS), COLS // 8), dtype=np.uint8)
    scales = np.exp2(rng.uniform(-20, 20, (max(ROWS), COLS // q1r.BLOCK))).astype(np.float32)
    pick = rng.random(scales.shape) < 0.2
    scales[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
    scales[0, :5] = SPECIAL
    weights = rng.standard_normal(max(ROWS)).astype(np.float32)
    weights[:4] = (2.0 ** 30, -1.0, 0.0, -0.0)
    g = rng.standard_normal(COLS).astype(np.float32)
    g[[5, C + 7]] = np.nan
    return q1, scales, weights, g, torch.from_numpy(q1).to(cuda)


def fold(data, cuda, rows, w, c0=0, center=False, acc_in=None, forced=0, in_place=False):
    """One launch over rows [rows[0], rows[1]) and columns [c0, c0 + w); returns (accumulator tensor, the
    restatement continued from acc_in).  Scale blocks the window does not touch are NaN: read, they show."""
    q1, scales, weights, g, dq = data
    a, b = rows
    s = scales[a:b].copy()
    s[:, : c0 // q1r.BLOCK] = np.nan
    s[:, -(-(c0 + w) // q1r.BLOCK):] = np.nan
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)  # noqa: E731
    acc = acc_in if in_place else torch.full((w + GUARD,), 7.0, dtype=torch.float32, device=cuda)
    before = None if acc_in is None else acc_in.cpu().numpy()[:w].copy()
    prev = ops.set_reduce_grid(forced)
    try:
        ops.deq_fold_q1_stack(dq[a:b], dev(s), dev(weights[a:b]), acc_in, acc, center=dev(g) if center else None,
                              col_begin=c0, n_cols=w, n_clients=b - a)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    assert launches == 1 and kernel == q1r.INSTANCE and grid == q1r.grid(w, 256, forced)
    assert (acc.cpu().numpy()[w:] == 7.0).all(), "guard columns were written"
    want = q1r.deq_fold1(before, q1[a:b], scales[a:b], weights[a:b], w, g[c0 : c0 + w] if center else None, c0)
    return acc, want


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("w", WIDTHS)
def test_windows_row_counts_and_grids(w, center, data, cuda):
    seen_inf = seen_nan = False
    for n in ROWS:
        for c0, forced in ((0, 0), (C, 1), (0, 3)):  # grid 1: every piece in one block; 3: pieces 0 and 1 of 2 or 3
            acc, want = fold(data, cuda, (0, n), w, c0=c0, center=center, forced=forced)
            assert q1r.same_bits(acc.cpu().numpy()[:w], want), (n, w, center, c0, forced)
            seen_inf |= bool(np.isinf(want).any())
            seen_nan |= bool(np.isnan(want).any())
    assert seen_inf or w < 2047  # 2^100 under 2^30 (row 0, columns 512..639) does reach +-inf
    assert seen_nan == (center and w > 5)  # the centre's NaN, and no inf - inf without it


@pytest.mark.parametrize("w", [33, PIECE])
def test_chain_opening_continuing_and_in_place(w, data, cuda):
    n, lo = 2 * q1r.D + 1, 4  # rows 4..: finite weights
    for center in (False, True):
        one, want = fold(data, cuda, (lo, lo + n), w, center=center)
        assert q1r.same_bits(one.cpu().numpy()[:w], want)
        for in_place in (False, True):
            acc = None
            for a, b in ((0, 1), (1, q1r.D + 2), (q1r.D + 2, n)):
                acc, step = fold(data, cuda, (lo + a, lo + b), w, center=center, acc_in=acc, in_place=in_place and acc is not None)
                assert q1r.same_bits(acc.cpu().numpy()[:w], step)
            assert q1r.same_bits(acc.cpu().numpy()[:w], want), (center, in_place)  # the chain is the one launch
