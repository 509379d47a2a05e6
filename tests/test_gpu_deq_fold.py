"""GPU: fa_deq_fold_q8 (ops.deq_fold_stack) against tests/quant_ref.py's row-by-row restatement, bit
for bit where the reference is not NaN and NaN where it is.  Codes over all 256 values, scales from 0
over subnormal products to sums that reach +-inf, negative, zero and huge weights; windows around the
16-column load, the 1024-column chunk and the piece; row counts around every shipped pipeline depth
and past 128; every shipped instantiation named by fa_last_launch; chains through acc_in; delta
uploads' centre; and the identity with the shipped fp32 fold on the dequantized rows."""
import numpy as np
import pytest
import torch

import quant_ref as qr
from flearn_amd import _native as na
from flearn_amd import ops

pytestmark = pytest.mark.gpu

B = qr.BLOCK
WIDTHS = (1, 15, 16, 17, 1023, 1024, 1025, 4 * B + 3)
STRIDE = 6 * B  # the next multiple of 1024 past the widest window, plus 1024
NMAX = 130
GUARD = 64
SPECIAL = np.array([0.0, 2.0 ** -140, 1.0, 2.0 ** 100, 0.0123, 3.5], dtype=np.float32)
WSPECIAL = np.array([-1.0, 0.0, 2.0 ** 30, 0.25, 1.0, -3.0, 1e-3], dtype=np.float32)


def rows_around(d):
    return {1, 2, d - 1, d, d + 1, 2 * d, 2 * d + 1, 130}


@pytest.fixture(scope="module")
def data(cuda):
    """[130, STRIDE] codes over all 256 values with -128 and 0 forced in, scales per (row, block)
    drawn from SPECIAL (row 3: all 0), weights from WSPECIAL, a random centre."""
    rng = np.random.default_rng(23)
    codes = rng.integers(-128, 128, (NMAX, STRIDE), dtype=np.int8)
    codes[:, 0] = -128
    codes[:, 1] = 0
    codes[::2, 2] = -128
    codes[1::2, 2] = 127
    codes[:, 5] = 0  # an all-zero-code column
    scales = SPECIAL[rng.integers(0, len(SPECIAL), (NMAX, STRIDE // B))]
    scales[3] = 0.0
    scales[0, 0] = 2.0 ** 100  # row 0 opens the sums at +-2^137 = +-inf under weight 2^30
    weights = WSPECIAL[rng.integers(0, len(WSPECIAL), NMAX)]
    weights[0] = 2.0 ** 30
    weights[1] = -1.0
    weights[2] = 0.0
    g = rng.standard_normal(STRIDE).astype(np.float32)
    return codes, scales, weights, g, torch.from_numpy(codes).to(cuda)


def dev(a, cuda, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(cuda)


def garbage_outside(scales, c0, w):
    """`scales` with every block the window does not touch set to NaN: read into a result, it shows."""
    s = scales.copy()
    b0, b1 = c0 // B, -(-(c0 + w) // B)
    s[:, :b0] = np.nan
    s[:, b1:] = np.nan
    return s


def fold(dq, scales, weights, rows, w, cuda, c0=0, center=None, acc_in=None, forced=0, in_place=False):
    """One launch over rows [rows[0], rows[1]) of the stack; returns (accumulator tensor, kernel).  The
    accumulator written has GUARD columns past the window holding 7.0, which must stay; an
    out-of-place acc_in must come back as it went in."""
    a, b = rows
    before = None if acc_in is None else acc_in.clone()
    acc = acc_in if in_place else torch.full((w + GUARD,), 7.0, dtype=torch.float32, device=cuda)
    ds = dev(garbage_outside(scales[a:b], c0, w), cuda)
    prev = ops.set_reduce_grid(forced)
    try:
        ops.deq_fold_stack(dq[a:b], ds, dev(weights[a:b], cuda), acc_in, acc, center=center, col_begin=c0, n_cols=w,
                           n_clients=b - a)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    assert launches == 1 and kernel in qr.TARGETS
    if forced:
        assert grid == min(forced, -(-w // B))
    out = acc.cpu().numpy()
    assert (out[w:] == 7.0).all(), "guard columns were written"
    if before is not None and not in_place:
        assert qr.same_bits(acc_in.cpu().numpy(), before.cpu().numpy()), "acc_in was modified"
    return acc, kernel


@pytest.mark.parametrize("w", WIDTHS)
def test_windows_and_row_counts(w, data, cuda):
    codes, scales, weights, g, dq = data
    dg = dev(g, cuda)
    seen_inf = False
    for n in sorted(rows_around(16) | rows_around(8)):
        for center in (None, g):
            acc, kernel = fold(dq, scales, weights, (0, n), w, cuda, center=None if center is None else dg)
            want = qr.deq_fold(None, codes[:n, :w], scales[:n], weights[:n], None if center is None else g[:w])
            assert qr.same_bits(acc.cpu().numpy()[:w], want), (n, w, center is not None)
            assert kernel == qr.instance(qr.plan(w, 256, 0).V)  # few chunks: one per block on any device
            seen_inf |= bool(np.isinf(want).any())
    assert seen_inf  # the data does reach +-inf


def test_every_shipped_instantiation_around_its_depth(data, cuda):
    codes, scales, weights, g, dq = data
    seen = set()
    for v, (w, forced) in qr.COVER.items():
        for n in sorted(rows_around(qr.depth(v))):
            acc, kernel = fold(dq, scales, weights, (0, n), w, cuda, forced=forced)
            assert kernel == qr.instance(v), (v, n)
            assert qr.same_bits(acc.cpu().numpy()[:w], qr.deq_fold(None, codes[:n, :w], scales[:n], weights[:n])), (v, n)
            seen.add(kernel)
    assert seen == qr.TARGETS


@pytest.mark.parametrize("c0", [B, 2 * B])
def test_window_inside_wider_rows(c0, data, cuda):
    codes, scales, weights, g, dq = data
    dg = dev(g, cuda)
    n = 11
    for w in (1, 17, B + 1, STRIDE - c0 - B + 3, STRIDE - c0):
        for center in (None, g):
            acc, _ = fold(dq, scales, weights, (0, n), w, cuda, c0=c0, center=None if center is None else dg)
            want = qr.deq_fold(None, codes[:n, c0 : c0 + w], scales[:n], weights[:n],
                               None if center is None else g[c0 : c0 + w], col_begin=c0)
            assert qr.same_bits(acc.cpu().numpy()[:w], want), (c0, w, center is not None)


def test_several_pieces_per_block_and_several_blocks(cuda):
    """20 chunks and 5 columns: under a forced grid of 1 / 3 / 4 a block sweeps 3 / 1 / 1 pieces of
    7 / 7 / 6 chunks (V = 2), under 7 one of 3 (V = 1); the default grid gives every chunk a block."""
    rng = np.random.default_rng(4)
    n, w = 5, 20 * B + 5
    codes = rng.integers(-128, 128, (n, 21 * B), dtype=np.int8)
    scales = SPECIAL[rng.integers(0, len(SPECIAL), (n, 21))]
    weights = np.array([0.5, -1.0, 0.0, 3.0, 1e-3], dtype=np.float32)
    g = rng.standard_normal(21 * B).astype(np.float32)
    dq, dg = torch.from_numpy(codes).to(cuda), dev(g, cuda)
    want = qr.deq_fold(None, codes[:, :w], scales, weights, g[:w])
    kernels = set()
    for forced in (0, 1, 3, 4, 7):
        acc, kernel = fold(dq, scales, weights, (0, n), w, cuda, center=dg, forced=forced)
        assert qr.same_bits(acc.cpu().numpy()[:w], want), forced
        assert kernel == qr.instance(qr.plan(w, 256, forced).V)
        kernels.add(kernel)
    assert kernels == qr.TARGETS


@pytest.mark.parametrize("w", [17, B + 1, 4 * B + 3])
def test_chain_split_at_every_row_boundary(w, data, cuda):
    codes, scales, weights, g, dq = data
    dg = dev(g, cuda)
    n = 5
    lo = 4  # rows 4..8: none of the forced specials of rows 0..3
    for center in (None, g):
        dc = None if center is None else dg
        one, _ = fold(dq, scales, weights, (lo, lo + n), w, cuda, center=dc)
        want = qr.deq_fold(None, codes[lo : lo + n, :w], scales[lo : lo + n], weights[lo : lo + n],
                           None if center is None else g[:w])
        assert qr.same_bits(one.cpu().numpy()[:w], want)
        for cuts in [(s,) for s in range(1, n)] + [tuple(range(1, n))]:
            for in_place in (False, True):
                acc = None
                bounds = [0, *cuts, n]
                for a, b in zip(bounds, bounds[1:]):
                    acc, _ = fold(dq, scales, weights, (lo + a, lo + b), w, cuda, center=dc, acc_in=acc,
                                  in_place=in_place and acc is not None)
                assert one.cpu().numpy()[:w].tobytes() == acc.cpu().numpy()[:w].tobytes(), (cuts, in_place)


def test_ragged_end_reads_nothing_past_n_cols(data, cuda):
    """acc_in holds NaN past n_cols: were it read into a column that is stored, the sums would show it."""
    codes, scales, weights, g, dq = data
    for w in (1, 15, 17, 1023, B + 1):
        first, _ = fold(dq, scales, weights, (4, 7), w, cuda)
        acc_in = first.clone()
        acc_in[w:] = float("nan")
        out, _ = fold(dq, scales, weights, (7, 12), w, cuda, acc_in=acc_in)
        want = qr.deq_fold(None, codes[4:12, :w], scales[4:12], weights[4:12])
        assert qr.same_bits(out.cpu().numpy()[:w], want), w


def test_centres_and_negative_zero(data, cuda):
    codes, scales, weights, g, dq = data
    n, w = 9, B + 17
    neg = np.full(STRIDE, -0.0, dtype=np.float32)
    results = {}
    for name, c in (("none", None), ("random", g), ("negzero", neg)):
        acc, _ = fold(dq, scales, weights, (0, n), w, cuda, center=None if c is None else dev(c, cuda))
        got = acc.cpu().numpy()[:w]
        assert qr.same_bits(got, qr.deq_fold(None, codes[:n, :w], scales[:n], weights[:n], None if c is None else c[:w])), name
        results[name] = got
    assert not qr.same_bits(results["none"], results["random"])
    # weights of -1 over the all-zero-code column: every product is -0.0 and so is the sum — the first
    # product is stored, not added to +0.0.  A centre of -0.0 turns the dequantized +0.0 ... into +0.0 + -0.0 = +0.0.
    minus = np.full(n, -1.0, dtype=np.float32)
    ones = np.ones_like(scales)
    acc, _ = fold(dq, ones, minus, (0, n), w, cuda)
    got = acc.cpu().numpy()[:w]
    assert got[5:6].view(np.uint32)[0] == 0x80000000 and got[1:2].view(np.uint32)[0] == 0x80000000
    assert qr.same_bits(got, qr.deq_fold(None, codes[:n, :w], ones[:n], minus))
    acc, _ = fold(dq, ones, minus, (0, n), w, cuda, center=dev(neg, cuda))
    assert qr.same_bits(acc.cpu().numpy()[:w], qr.deq_fold(None, codes[:n, :w], ones[:n], minus, neg[:w]))


@pytest.mark.parametrize("with_center", [False, True])
def test_identity_with_the_fp32_fold_on_the_dequantized_rows(with_center, data, cuda):
    """ops.fold_stack(ACC_F32) over the rows dequantized on the host leaves the same bytes, opening and
    continuing a sum (finite data: every byte is compared)."""
    codes, _, _, g, dq = data
    rng = np.random.default_rng(8)
    n, w = 21, 4 * B + 3
    scales = np.array([0.0, 2.0 ** -140, 1.0, 0.37], dtype=np.float32)[rng.integers(0, 4, (n, STRIDE // B))]
    weights = rng.standard_normal(n).astype(np.float32)
    weights[[2, 5]] = (0.0, -2.0)
    deq = np.stack([qr.dequantize(codes[i], scales[i], g if with_center else None) for i in range(n)])
    dx, dw = torch.from_numpy(deq).to(cuda), dev(weights, cuda)
    dg = dev(g, cuda) if with_center else None
    for splits in ((0, n), (0, 8, n)):
        f32 = torch.empty(w, dtype=torch.float32, device=cuda)
        acc, prev = None, None
        for a, b in zip(splits, splits[1:]):
            ops.fold_stack(na.ACC_F32, dx[a:b], dw[a:b], prev, f32, n_cols=w)
            prev = f32
            acc, _ = fold(dq, scales, weights, (a, b), w, cuda, center=dg, acc_in=acc)
        assert f32.cpu().numpy().tobytes() == acc.cpu().numpy()[:w].tobytes(), splits
        assert np.isfinite(f32.cpu().numpy()).all()


def test_python_side_checks(data, cuda):
    codes, scales, weights, g, dq = data
    ds, dw, dg = dev(scales, cuda), dev(weights, cuda), dev(g, cuda)
    acc = torch.empty(STRIDE, dtype=torch.float32, device=cuda)
    with pytest.raises(TypeError, match="int8"):
        ops.deq_fold_stack(dq.to(torch.uint8), ds, dw, None, acc)
    with pytest.raises(ValueError, match="stack_i8"):
        ops.deq_fold_stack(dq[0], ds, dw, None, acc)
    with pytest.raises(ValueError, match="scales"):
        ops.deq_fold_stack(dq, ds[:, :5], dw, None, acc)
    with pytest.raises(ValueError, match="scales"):
        ops.deq_fold_stack(dq, ds[:100], dw, None, acc)
    with pytest.raises(ValueError, match="scales"):
        ops.deq_fold_stack(dq, ds.double(), dw, None, acc)
    with pytest.raises(ValueError, match="weights"):
        ops.deq_fold_stack(dq, ds, dw[:5], None, acc)
    with pytest.raises(ValueError, match="center"):
        ops.deq_fold_stack(dq, ds, dw, None, acc, center=dg[:100])
    with pytest.raises(ValueError, match="acc_out"):
        ops.deq_fold_stack(dq, ds, dw, None, acc[:100])
    with pytest.raises(ValueError, match="acc_in"):
        ops.deq_fold_stack(dq, ds, dw, acc.double(), acc)
    with pytest.raises(ValueError, match="window"):
        ops.deq_fold_stack(dq, ds, dw, None, acc, col_begin=B, n_cols=STRIDE)
    with pytest.raises(na.NativeError, match="1024"):
        ops.deq_fold_stack(dq, ds, dw, None, acc, col_begin=512, n_cols=16)
    with pytest.raises(na.NativeError, match="overlap"):  # neither the same array nor a disjoint one
        ops.deq_fold_stack(dq, ds, dw, acc[4:], acc, n_cols=100)
    ops.deq_fold_stack(dq, ds, dw, acc, acc, n_cols=0)  # a no-op
    assert ops.last_launch()[0] is None
