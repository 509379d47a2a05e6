"""GPU: fa_fold_bf16 (ops.fold_bf16_stack) against tests/bf16_ref.py, bit for bit (NaN where it is NaN):
special values, widths around the load, the chunk and every piece, row counts around every depth, chains."""
import numpy as np
import pytest
import torch

import bf16_ref as br
from flearn_amd import ops

pytestmark = pytest.mark.gpu

C = br.CHUNK
PIECES = [C * br.W * v + d for v in br.VS for d in (-1, 0, 1)]
NMAX, STRIDE, GUARD = 2 * br.depth(1) + 1, C * br.W * br.MAX_V + 1 + C + 7, 64
SPECIAL = np.array([0x0000, 0x8000, 0x0001, 0x807F, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0], dtype=np.uint16)
ROWS = sorted({n for v in br.VS for d in [br.depth(v)] for n in (1, 2, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1)})


@pytest.fixture(scope="module")
def data(cuda):
    rng = np.random.default_rng(26)  # 40 binades, 3% specials, column 0 all -0.0, column 3 all the largest finite value
    x = (rng.standard_normal((NMAX, STRIDE)) * 2.0 ** rng.integers(-20, 20, (NMAX, STRIDE))).astype(np.float32)
    u = (x.view(np.uint32) >> 16).astype(np.uint16)
    hit = rng.random(u.shape) < 0.03
    u[hit] = SPECIAL[rng.integers(0, len(SPECIAL), int(hit.sum()))]
    u[:, 0], u[:, 3] = 0x8000, 0x7F7F
    weights = np.resize(np.array([0.3, 1.7, 0.0], dtype=np.float32), NMAX)
    want = br.fold(None, u, weights)  # the data does reach the special sums
    assert want[0:1].view(np.uint32)[0] == 0x80000000 and np.isinf(want[3]) and np.isnan(want).any()
    assert (np.abs(br.widen(u)[br.widen(u) != 0]) < 2.0 ** -126).any()  # bfloat16 subnormals among the rows
    return u, weights, torch.from_numpy(u.view(np.int16)).to(cuda), torch.from_numpy(weights).to(cuda)


def fold(data, rows, w, cuda, c0=0, acc_in=None, forced=0, in_place=False):
    """One launch over rows [a, b) -> (accumulator, kernel name); GUARD columns past the window hold 7.0 and must stay."""
    _, _, du, dw = data
    a, b = rows
    acc = acc_in if in_place else torch.full((w + GUARD,), 7.0, dtype=torch.float32, device=cuda)
    prev = ops.set_reduce_grid(forced)
    try:
        ops.fold_bf16_stack(du[a:b], dw[a:b], acc_in, acc, col_begin=c0, n_cols=w, n_clients=b - a)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    assert launches == 1 and (not forced or grid == min(forced, -(-w // C)))
    assert (acc.cpu().numpy()[w:] == 7.0).all(), "columns past n_cols were written"
    return acc, kernel


@pytest.mark.parametrize("w", [1, 7, 8, 9, C - 1, C, C + 1] + PIECES)
def test_widths_and_row_counts(w, data, cuda):
    u, weights = data[:2]
    forced = 1 if w > C + 1 else 0  # one block: the piece widths reach their V on any device
    v = br.plan_v(w, 256, forced)[0]
    for n in ROWS:
        acc, kernel = fold(data, (0, n), w, cuda, forced=forced)
        assert kernel == br.instance(v), (n, kernel)
        assert br.same_bits(acc.cpu().numpy()[:w], br.fold(None, u[:n, :w], weights[:n])), n
    if w in PIECES[:-1]:  # up to a full piece of V chunks per wave: that V; one past the widest: two rounds
        assert v == next(x for x in br.VS if w <= C * br.W * x)


@pytest.mark.parametrize("forced", [1, 3])
def test_several_pieces_per_block(forced, cuda):
    rng = np.random.default_rng(5)
    n, w = 5, 100 * C + 5  # 101 chunks: a grid of 1 sweeps 7 pieces of 15 chunks, a grid of 3 three pieces of 12 each
    u = rng.integers(0, 1 << 16, (n, w + 3), dtype=np.uint16)
    weights = np.array([0.3, 1.7, 0.0, -1.0, 1e-3], dtype=np.float32)
    d = (u, weights, torch.from_numpy(u.view(np.int16)).to(cuda), torch.from_numpy(weights).to(cuda))
    acc, kernel = fold(d, (0, n), w, cuda, forced=forced)
    assert kernel == br.instance(4) and br.same_bits(acc.cpu().numpy()[:w], br.fold(None, u[:, :w], weights))


@pytest.mark.parametrize("c0", [0, 8, C])
def test_window_inside_wider_rows_and_chains(c0, data, cuda):
    """Outside the window the rows hold NaN (read, it shows); chunks of K rows chained equal the one-launch fold."""
    u, weights, du, dw = data
    n = 11
    for w in (9, C + 1, 4 * C + 3):
        dirty = u.copy()
        dirty[:, c0 + w :] = 0x7FC0
        dirty[:, :c0] = 0x7FC0
        d = (dirty, weights, torch.from_numpy(dirty.view(np.int16)).to(cuda), dw)
        one, _ = fold(d, (0, n), w, cuda, c0=c0)
        assert br.same_bits(one.cpu().numpy()[:w], br.fold(None, u[:n, c0 : c0 + w], weights[:n])), w
        for k in (1, 4, 5):
            for in_place in (False, True):
                acc = None
                for lo in range(0, n, k):
                    before = None if acc is None else acc.clone()
                    out, _ = fold(d, (lo, min(n, lo + k)), w, cuda, c0=c0, acc_in=acc, in_place=in_place and acc is not None)
                    assert in_place or before is None or torch.equal(acc.view(torch.int32), before.view(torch.int32))
                    acc = out
                assert one.cpu().numpy()[:w].tobytes() == acc.cpu().numpy()[:w].tobytes(), (w, k, in_place)
