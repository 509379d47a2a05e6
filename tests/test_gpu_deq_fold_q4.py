"""GPU: fa_deq_fold_q4 (ops.deq_fold_q4_stack) against tests/quant4_ref.py's row-by-row restatement,
bit for bit where the reference is not NaN and NaN where it is: windows around the load, the scale block,
the chunk and the piece inside wider rows of garbage, row counts around the pipeline depth, chains
through acc_in, a centre, and the identity with the shipped fp32 fold on the dequantized rows."""
import numpy as np
import pytest
import torch

import quant4_ref as q4r
from flearn_amd import _native as na
from flearn_amd import ops

pytestmark = pytest.mark.gpu

C = q4r.CHUNK
PIECE = q4r.PIECE_CHUNKS * C + 3  # the widest shipped piece and 3 columns: two pieces under a forced grid of 1
WIDTHS = (1, 31, 33, 127, 129, 2047, 2049, PIECE)
COLS = 7 * C  # a row: the widest window behind a col_begin of 4096, and a chunk of garbage more
NMAX = 130
GUARD = 64
SPECIAL = np.array([0.0, -0.0, 2.0 ** -100, 1.0, 2.0 ** 100], dtype=np.float32)
ROWS = sorted({q4r.depth(v) * m + d for v in q4r.VS for m, d in ((1, -1), (1, 0), (1, 1), (2, 0), (2, 1))} | {NMAX})


@pytest.fixture(scope="module")
def data(cuda):
    """[130, COLS / 2] random bytes, scales per (row, block) log-uniform over 2^+-20 with SPECIAL drawn
    into a fifth of them, weights with 2^30, -1 and 0 forced in, a random centre."""
    rng = np.random.default_rng(41)
    q4 = rng.integers(0, 256, (NMAX, COLS // 2), dtype=np.uint8)
    codes = q4r.unpack(q4[:8, :64], 128)
    assert all(set(codes[:, p::2].reshape(-1).tolist()) == set(range(-8, 8)) for p in (0, 1))
    scales = np.exp2(rng.uniform(-20, 20, (NMAX, COLS // q4r.BLOCK))).astype(np.float32)
    pick = rng.random(scales.shape) < 0.2
    scales[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
    scales[0, :5] = SPECIAL
    assert len({s.tobytes() for s in scales[:3, :16].reshape(-1)}) > 30  # the blocks of a chunk and the rows differ
    weights = rng.standard_normal(NMAX).astype(np.float32)
    weights[:3] = (2.0 ** 30, -1.0, 0.0)
    g = rng.standard_normal(COLS).astype(np.float32)
    return q4, scales, weights, g, torch.from_numpy(q4).to(cuda)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def fold(data, cuda, rows, w, c0=0, center=False, acc_in=None, forced=0, in_place=False):
    """One launch over rows [rows[0], rows[1]) and columns [c0, c0 + w); returns (accumulator tensor,
    the restatement continued from acc_in).  Scale blocks the window does not touch are NaN: read into
    a result, they show.  The accumulator has GUARD columns past the window holding 7.0, which must stay."""
    q4, scales, weights, g, dq = data
    a, b = rows
    s = scales[a:b].copy()
    s[:, : c0 // q4r.BLOCK] = np.nan
    s[:, -(-(c0 + w) // q4r.BLOCK):] = np.nan
    acc = acc_in if in_place else torch.full((w + GUARD,), 7.0, dtype=torch.float32, device=cuda)
    before = None if acc_in is None else acc_in.cpu().numpy()[:w].copy()
    prev = ops.set_reduce_grid(forced)
    try:
        ops.deq_fold_q4_stack(dq[a:b], dev(s, cuda), dev(weights[a:b], cuda), acc_in, acc, center=dev(g, cuda) if center else None,
                              col_begin=c0, n_cols=w, n_clients=b - a)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    assert launches == 1 and kernel == q4r.instance(q4r.plan(w, 256, forced).V) and kernel in q4r.TARGETS
    assert grid == min(forced, -(-w // C)) if forced else grid == q4r.plan(w, 256).grid  # few chunks: one block each
    assert (acc.cpu().numpy()[w:] == 7.0).all(), "guard columns were written"
    want = q4r.deq_fold4(before, q4[a:b], scales[a:b], weights[a:b], w, g[c0 : c0 + w] if center else None, c0)
    return acc, want


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("w", WIDTHS)
def test_windows_and_row_counts(w, center, data, cuda):
    seen_inf = False
    for n in ROWS:
        acc, want = fold(data, cuda, (0, n), w, center=center, forced=1 if w == PIECE else 0)
        assert q4r.same_bits(acc.cpu().numpy()[:w], want), (n, w, center)
        seen_inf |= bool(np.isinf(want).any())
    assert seen_inf or w < 2047  # 2^100 under 2^30 (row 0, columns 512..639) does reach +-inf


@pytest.mark.parametrize("c0", [C, 2 * C])
def test_window_inside_wider_rows(c0, data, cuda):
    for w in (1, 33, 129, C + 1, PIECE):
        for center in (False, True):
            acc, want = fold(data, cuda, (3, 14), w, c0=c0, center=center)
            assert q4r.same_bits(acc.cpu().numpy()[:w], want), (c0, w, center)


@pytest.mark.parametrize("w", [33, C + 129])
def test_chain_split_at_every_row_boundary(w, data, cuda):
    n, lo = 5, 4
    for center in (False, True):
        one, want = fold(data, cuda, (lo, lo + n), w, center=center)
        assert q4r.same_bits(one.cpu().numpy()[:w], want)
        for cuts in [(s,) for s in range(1, n)] + [tuple(range(1, n))]:
            for in_place in (False, True):
                acc, bounds = None, [0, *cuts, n]
                for a, b in zip(bounds, bounds[1:]):
                    acc, step = fold(data, cuda, (lo + a, lo + b), w, center=center, acc_in=acc, in_place=in_place and acc is not None)
                    assert q4r.same_bits(acc.cpu().numpy()[:w], step)
                assert one.cpu().numpy()[:w].tobytes() == acc.cpu().numpy()[:w].tobytes(), (cuts, in_place)


@pytest.mark.parametrize("center", [False, True])
def test_identity_with_the_fp32_fold_on_the_dequantized_rows(center, data, cuda):
    """ops.fold_stack(ACC_F32) over the rows dequantized on the host leaves the same bytes, opening and
    continuing a sum (rows 20..41 with their 2^100 scales tamed: finite data, every byte is compared)."""
    q4, scales, weights, g, dq = data
    lo, n, w = 20, 21, PIECE
    tame = (q4, np.where(scales > 2.0 ** 50, np.float32(0.37), scales), weights, g, dq)
    deq = np.stack([q4r.dequantize(q4[lo + i], COLS, tame[1][lo + i], g if center else None) for i in range(n)])
    dx, dw = torch.from_numpy(deq).to(cuda), dev(weights[lo : lo + n], cuda)
    for splits in ((0, n), (0, 8, n)):
        f32 = torch.empty(w, dtype=torch.float32, device=cuda)
        acc, prev = None, None
        for a, b in zip(splits, splits[1:]):
            ops.fold_stack(na.ACC_F32, dx[a:b], dw[a:b], prev, f32, n_cols=w)
            prev = f32
            acc, _ = fold(tame, cuda, (lo + a, lo + b), w, center=center, acc_in=acc)
        assert f32.cpu().numpy().tobytes() == acc.cpu().numpy()[:w].tobytes(), splits
        assert np.isfinite(f32.cpu().numpy()).all()
