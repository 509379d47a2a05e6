"""GPU: fa_deq_fold_mx (ops.deq_fold_mx_stack) against tests/mx_ref.py's row-by-row restatement, bit for bit
where the reference is not NaN and NaN where it is, for MXFP4 and MXFP8: windows around the scale block, the
chunk and the piece inside wider rows, row counts around the pipeline depth, chains through acc_in, a centre,
every code in every position of a lane's load, and a row past the 4 GiB byte offset."""
import numpy as np
import pytest
import torch

import mx_ref as mxr
from flearn_amd import ops

pytestmark = pytest.mark.gpu

C = mxr.CHUNK
PIECE = mxr.W * mxr.V * C + C + 5  # a full piece, a chunk and 5 columns: several pieces per block at grid 1, a ragged end
WIDTHS = (1, 31, 32, 33, 2047, 2048, 2049, PIECE)
COLS = 7 * C  # a row: the widest window behind a col_begin of 2048, and a chunk more
ROWS = 2 * max(mxr.D.values()) + 1
GUARD = 64  # columns on either side of a window's accumulator: they hold 7.0 and must stay
SCALES = np.array([27, 227, 127, 120, 134, 100, 150], dtype=np.uint8)


def row_counts(elem):
    d = mxr.D[elem]
    return (1, 2, d - 1, d, d + 1, 2 * d + 1)


@pytest.fixture(scope="module", params=[4, 8], ids=["fp4", "fp8"])
def data(request, cuda):
    """[ROWS, COLS] random codes (every byte value: E4M3's NaNs and both zeros included), scale bytes drawn
    from SCALES so that neighbouring blocks differ, weights with 2^30 (times 448 * 2^100: inf), -1, 0 and -0.0
    forced in, a centre with two NaNs."""
    elem = request.param
    rng = np.random.default_rng(43 + elem)
    codes = rng.integers(0, 256, (ROWS, COLS * elem // 8), dtype=np.uint8)
    scales = SCALES[(np.arange(COLS // mxr.BLOCK)[None, :] + 3 * np.arange(ROWS)[:, None]) % len(SCALES)]
    weights = rng.standard_normal(ROWS).astype(np.float32)
    weights[:4] = (2.0 ** 30, -1.0, 0.0, -0.0)
    g = rng.standard_normal(COLS).astype(np.float32)
    g[[5, C + 7]] = np.nan
    return elem, codes, scales, weights, g, torch.from_numpy(codes).to(cuda)


def fold(data, cuda, rows, w, c0=0, center=False, acc_in=None, forced=0, in_place=False):
    """One launch over rows [rows[0], rows[1]) and columns [c0, c0 + w); returns (the window of the accumulator,
    the restatement continued from acc_in).  Scale blocks the window does not touch are 255: read, they show."""
    elem, codes, scales, weights, g, dq = data
    a, b = rows
    s = scales[a:b].copy()
    s[:, : c0 // mxr.BLOCK] = 255
    s[:, -(-(c0 + w) // mxr.BLOCK):] = 255
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)  # noqa: E731
    buf = torch.full((w + 2 * GUARD,), 7.0, dtype=torch.float32, device=cuda)
    acc = acc_in if in_place else buf[GUARD : GUARD + w]
    before = None if acc_in is None else acc_in.cpu().numpy().copy()
    prev = ops.set_reduce_grid(forced)
    try:
        ops.deq_fold_mx_stack(dq[a:b], dev(s), dev(weights[a:b]), acc_in, acc, center=dev(g) if center else None,
                              col_begin=c0, n_cols=w, n_clients=b - a, elem=elem)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    assert launches == 1 and kernel == f"mx_fold_kernel<{elem},{mxr.V},{mxr.D[elem]},{mxr.W},true>", kernel
    assert grid == max(1, min(forced, -(-w // C))) or not forced
    assert (buf.cpu().numpy()[:GUARD] == 7.0).all() and (buf.cpu().numpy()[GUARD + w:] == 7.0).all(), "guard columns were written"
    want = mxr.deq_fold(before, codes[a:b], scales[a:b], weights[a:b], w, elem, g[c0 : c0 + w] if center else None, c0)
    return acc, want


@pytest.mark.parametrize("center", [False, True])
def test_windows_and_row_counts(center, data, cuda):
    seen_inf = False
    for n in row_counts(data[0]):
        for w in WIDTHS:
            for c0, forced in ((0, 0), (C, 1)) if w in (33, 2049, PIECE) else ((0, 0),):  # grid 1: every piece in one block
                acc, want = fold(data, cuda, (0, n), w, c0=c0, center=center, forced=forced)
                assert mxr.same_bits(acc.cpu().numpy(), want), (n, w, center, c0, forced)
                seen_inf |= bool(np.isinf(want).any())
    assert seen_inf  # a large code under scale byte 227 and weight 2^30


@pytest.mark.parametrize("w", [33, PIECE])
def test_chain_opening_continuing_and_in_place(w, data, cuda):
    d = mxr.D[data[0]]
    n, lo = 2 * d - 3, 4  # rows 4..: finite weights
    for center in (False, True):
        one, want = fold(data, cuda, (lo, lo + n), w, center=center)
        assert mxr.same_bits(one.cpu().numpy(), want)
        for in_place in (False, True):
            acc = None
            for a, b in ((0, 1), (1, d + 2), (d + 2, n)):
                acc, step = fold(data, cuda, (lo + a, lo + b), w, center=center, acc_in=acc, in_place=in_place and acc is not None)
                assert mxr.same_bits(acc.cpu().numpy(), step)
            assert mxr.same_bits(acc.cpu().numpy(), want), (center, in_place)  # the chain is the one launch


@pytest.mark.parametrize("elem", [4, 8])
def test_every_code_in_every_position(elem, cuda):
    """Four rows of two chunks: at position p of a lane's 32 columns the 64 lanes of a chunk hold 64 consecutive
    codes and the rows are 64 apart, so every position sees all 256 (mod 16: all 16) codes.  Neighbouring scale
    blocks differ and include 27 and 227; the weights are negative, zero, one, and 2^30 (overflow to inf)."""
    cols = np.arange(2 * C)
    code = ((cols // 32 + 7 * (cols % 32))[None, :] + 64 * np.arange(4)[:, None]) % (1 << elem)
    for p in range(32):
        assert len(np.unique(code[:, :C][:, cols[:C] % 32 == p])) == 1 << elem
    stack = code.astype(np.uint8) if elem == 8 else (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    scales = SCALES[(np.arange(2 * C // 32)[None, :] + np.arange(4)[:, None]) % 3]  # 27, 227, 127 in turn
    g = np.linspace(-3, 3, 2 * C).astype(np.float32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)  # noqa: E731
    for weights in ([-1.0, 0.0, 1.0, 0.75], [2.0 ** 30, -0.0, -2.5, 1.0]):
        for center in (None, g):
            acc = torch.empty(2 * C, dtype=torch.float32, device=cuda)
            w = np.array(weights, dtype=np.float32)
            ops.deq_fold_mx_stack(dev(stack), dev(scales), dev(w), None, acc, center=None if center is None else dev(center), elem=elem)
            want = mxr.deq_fold(None, stack, scales, w, 2 * C, elem, center)
            assert mxr.same_bits(acc.cpu().numpy(), want), (weights, center is not None)
            assert np.isnan(want).any() == (elem == 8) and (np.isinf(want).any() or weights[0] < 2)


@pytest.mark.parametrize("elem", [4, 8])
def test_a_row_past_4_gib(elem, cuda):
    """Rows 2^31 + 4096 bytes apart: row 2's window begins past the 4 GiB byte offset.  Only the windows are
    written; the window sits one chunk into the row."""
    stride, w, n = (1 << 31) + 4096, C + 37, 3
    if torch.cuda.mem_get_info(cuda)[0] < 3 * stride + (1 << 30):
        pytest.skip("needs 7 GiB of free device memory")
    rng = np.random.default_rng(elem)
    nbytes = -(-w * elem // 8)
    host = rng.integers(0, 127 if elem == 8 else 256, (n, nbytes), dtype=np.uint8)  # no E4M3 NaN: every sum is compared
    c0 = C
    raw = torch.empty(2 * stride + 4 * C, dtype=torch.uint8, device=cuda)
    stack = torch.as_strided(raw, (n, (c0 + w) * elem // 8 + 1), (stride, 1))
    stack[:, c0 * elem // 8 : c0 * elem // 8 + nbytes] = torch.from_numpy(host).to(cuda)
    blocks = -(-(c0 + w) // 32)
    scales = SCALES[rng.integers(0, len(SCALES), (n, -(-blocks // 4) * 4))]
    weights = np.array([1.5, -0.25, 3.0], dtype=np.float32)
    acc = torch.empty(w, dtype=torch.float32, device=cuda)
    ops.deq_fold_mx_stack(stack, torch.from_numpy(scales).to(cuda), torch.from_numpy(weights).to(cuda), None, acc,
                          col_begin=c0, n_cols=w, elem=elem)
    full = np.zeros((n, (c0 + w) * elem // 8 + 1), dtype=np.uint8)
    full[:, c0 * elem // 8 : c0 * elem // 8 + nbytes] = host
    assert mxr.same_bits(acc.cpu().numpy(), mxr.deq_fold(None, full, scales, weights, w, elem, None, c0))
