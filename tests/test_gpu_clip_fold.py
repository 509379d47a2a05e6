"""GPU: fa_clip_fold_f32 (ops.clip_fold_stack), bit for bit.  Opening a round (acc_in None) it is
fa_clip_sum_f32; continuing one it adds every row of the chunk to the carried sum, so a chain of
chunks leaves the bits of one fa_clip_sum_f32 over all their rows.  test_gpu_clip_sum.py's data
recipe and scale patterns; splits around every shipped pipeline depth, every shipped instantiation
named by fa_last_launch; the ragged end, a window inside wider rows, rows that must not be read,
and fa_fold_finish over the chained accumulator."""
import numpy as np
import pytest
import torch

import clip_ref as cr
import clipfold_ref as cf
import robust_ref as rr
from flearn_amd import _native as na
from flearn_amd import ops

pytestmark = pytest.mark.gpu

P = cr.piece_cols(16)
NS = (1, 2, 3, 63, 64, 65, 100, 128)
WIDTHS = (1, 3, 4, 255, P - 1, P, P + 1, 3 * P + 5)
STRIDE = 3 * P + 8
GUARD = 64
MIXED = np.array([1.0, 0.37, 0.0, 2.0, -1.0, np.nan, 0.999, 1e-3, np.inf, -0.0, 1e-40], dtype=np.float32)


@pytest.fixture(scope="module")
def data(cuda):
    """[128, STRIDE] random rows around a random centre; a few columns carry denormals, values near
    the fp32 overflow (one sign only: no inf - inf) and an all -0.0 column."""
    rng = np.random.default_rng(11)
    g = rng.standard_normal(STRIDE).astype(np.float32)
    x = (g[None, :] + (rng.standard_normal((128, STRIDE)) * 10.0 ** rng.integers(-2, 3, (128, 1)))).astype(np.float32)
    x[:, 2] = -0.0
    g[2] = -0.0
    x[:, 7] = rng.integers(1, 1000, 128).astype(np.uint32).view(np.float32)  # denormals
    g[7] = 0.0
    x[::3, 9] = 3.0e38
    x[1, 11] = 3.3e38
    return x, g, torch.from_numpy(x).to(cuda), torch.from_numpy(g).to(cuda)


def pattern(n, seed):
    rng = np.random.default_rng(seed)
    return MIXED[rng.integers(0, len(MIXED), n)]


def dev(a, like):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(like.device)


def clip_sum(dx, dg, scale, n, w, forced=0, c0=0):
    """The existing kernel over rows [0, n): the yardstick."""
    acc = torch.empty(w, dtype=torch.float32, device=dx.device)
    prev = ops.set_reduce_grid(forced)
    try:
        ops.clip_sum_stack(dx, dg, dev(scale[:n], dx), acc, n_clients=n, col_begin=c0, n_cols=w)
    finally:
        ops.set_reduce_grid(prev)
    return acc.cpu().numpy()


def fold(dx, dg, scale, rows, w, acc_in=None, forced=0, c0=0, in_place=False):
    """One clip_fold launch over rows [rows[0], rows[1]); returns (sums, kernel).  The accumulator
    written has GUARD columns past the window holding 7.0, which must stay; an out-of-place acc_in
    must come back as it went in."""
    a, b = rows
    before = None if acc_in is None else acc_in.clone()
    if in_place:
        acc = acc_in
    else:
        acc = torch.full((w + GUARD,), 7.0, dtype=torch.float32, device=dx.device)
    prev = ops.set_reduce_grid(forced)
    try:
        ops.clip_fold_stack(dx[a:b], dg, dev(scale[a:b], dx), acc_in, acc, n_clients=b - a, col_begin=c0, n_cols=w)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    assert launches == 1 and kernel.startswith("clip_fold_kernel<")
    out = acc.cpu().numpy()
    assert (out[w:] == 7.0).all(), "guard columns were written"
    if before is not None and not in_place:
        assert rr.same_bits(acc_in.cpu().numpy(), before.cpu().numpy()), "acc_in was modified"
    return acc, kernel


def chain(dx, dg, scale, n, w, splits, forced=0, c0=0, in_place=False):
    acc, kernels = None, set()
    for rows in cf.chunks_of(n, splits):
        acc, kernel = fold(dx, dg, scale, rows, w, acc, forced, c0, in_place and acc is not None)
        kernels.add(kernel)
    return acc.cpu().numpy()[:w], kernels


@pytest.mark.parametrize("w", WIDTHS)
def test_opening_launch_is_clip_sum(w, data):
    x, g, dx, dg = data
    for n, forced in [(n, 0) for n in NS] + [(100, 2)]:
        sc = pattern(n, n * 1000 + w)
        got, _ = chain(dx, dg, sc, n, w, (), forced)
        assert rr.same_bits(got, clip_sum(dx, dg, sc, n, w, forced)), (n, w, forced)
        assert rr.same_bits(got, cr.clipped_sum(x[:n, :w], g[:w], sc)), (n, w, forced)


def test_every_shipped_instantiation_continues_around_its_depth(data):
    x, g, dx, dg = data
    seen = set()
    for v, (w, forced) in cf.COVER.items():
        d = 16 // v
        n = 2 * d + 3
        sc = pattern(n, 31 * v)
        want = clip_sum(dx, dg, sc, n, w, forced)
        assert rr.same_bits(want, cf.fold_chain(x[:n, :w], g[:w], sc, ()))
        for s in sorted({1, d - 1, d, d + 1, n - 1} - {0}):
            for in_place in (False, True):
                got, kernels = chain(dx, dg, sc, n, w, (s,), forced, in_place=in_place)
                assert kernels == {cr.instance(cf.FAMILY, v)}, (v, s)
                assert rr.same_bits(got, want), (v, s, in_place)
                seen |= kernels
    assert seen == cf.TARGETS


@pytest.mark.parametrize("w", [255, P + 1, 3 * P + 5])
def test_three_chunks_and_singletons(w, data):
    x, g, dx, dg = data
    n = 20
    sc = pattern(n, 20 + w)
    want = clip_sum(dx, dg, sc, n, w)
    for splits in ((7, 13), (1, 19), tuple(range(1, n))):
        for in_place in (False, True):
            got, _ = chain(dx, dg, sc, n, w, splits, in_place=in_place)
            assert rr.same_bits(got, want), (splits, in_place)
    got, _ = chain(dx, dg, sc, n, w, (5, 9), forced=2)  # the pieces of a chain need not be the one launch's
    assert rr.same_bits(got, want)
    assert rr.same_bits(want, cf.fold_chain(x[:n, :w], g[:w], sc, (7, 13)))


@pytest.mark.parametrize("s0", [0.0, 0.25, 1.0])
def test_continuing_chunk_row_0_under_each_branch(s0, data):
    x, g, dx, dg = data
    n, s, w = 30, 11, P + 1
    sc = pattern(n, 3)
    sc[s] = s0
    got, _ = chain(dx, dg, sc, n, w, (s,))
    assert rr.same_bits(got, clip_sum(dx, dg, sc, n, w))
    assert rr.same_bits(got, cr.clipped_sum(x[:n, :w], g[:w], sc))


def test_continuing_chunk_of_unread_rows(data):
    """Every scale of the continuing chunk is 0 and its rows are NaN / inf: they are not read, and the
    result is acc_in plus k adds of the centre."""
    x, g, dx, dg = data
    n, s, w = 14, 9, 3 * P + 5
    k = n - s
    sc = pattern(n, 8)
    sc[s:] = 0.0
    bad = dx[:n].clone()
    bad[s::2] = float("nan")
    bad[s + 1 :: 2] = float("inf")
    acc_in, _ = fold(bad, dg, sc, (0, s), w)
    acc_in = acc_in[:w].clone()
    out, _ = fold(bad, dg, sc, (s, n), w, acc_in)
    want = acc_in.cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(k):
            want = (want + g[:w]).astype(np.float32)
    assert rr.same_bits(out.cpu().numpy()[:w], want)
    assert rr.same_bits(want, cr.clipped_sum(x[:n, :w], g[:w], sc))


def test_window_inside_wider_rows(data):
    x, g, dx, dg = data
    n, w, c0 = 9, 777, 260
    sc = pattern(n, 9)
    for in_place in (False, True):
        got, _ = chain(dx, dg, sc, n, w, (4,), c0=c0, in_place=in_place)
        assert rr.same_bits(got, cr.clipped_sum(x[:n, c0 : c0 + w], g[c0 : c0 + w], sc))
        assert rr.same_bits(got, clip_sum(dx, dg, sc, n, w, c0=c0))


@pytest.mark.parametrize("w", [1, 3, 255, P - 1, P + 1])
def test_ragged_end_reads_and_writes_nothing_past_n_cols(w, data):
    """acc_in holds NaN past n_cols: were it read into a column that is stored, the sums would show
    it; the guard columns of acc_out (checked by fold) keep their 7.0; acc_in is unmodified."""
    x, g, dx, dg = data
    n, s = 12, 5
    sc = pattern(n, w)
    first, _ = fold(dx, dg, sc, (0, s), w)
    acc_in = first.clone()
    acc_in[w:] = float("nan")
    out, _ = fold(dx, dg, sc, (s, n), w, acc_in)
    assert rr.same_bits(out.cpu().numpy()[:w], clip_sum(dx, dg, sc, n, w))


@pytest.mark.parametrize("op", ["mean", "avgm", "adagrad", "yogi", "adam"])
def test_fold_finish_over_chained_and_one_launch_accumulators(op, data, cuda):
    x, g, dx, dg = data
    n, w = 20, 4099
    sc = pattern(n, 77)
    sc[sc != sc] = 0.0
    one = torch.empty(w, dtype=torch.float32, device=cuda)
    ops.clip_sum_stack(dx, dg, dev(sc, dx), one, n_clients=n, n_cols=w)
    chained = torch.empty(w, dtype=torch.float32, device=cuda)
    acc_in = None
    for a, b in cf.chunks_of(n, (6, 7, 15)):
        ops.clip_fold_stack(dx[a:b], dg, dev(sc[a:b], dx), acc_in, chained, n_cols=w)
        acc_in = chained
    outs = []
    for acc in (chained, one):
        prev = torch.from_numpy(g[:w].copy()).to(cuda)
        v = torch.from_numpy(np.full(w, 0.01)).to(cuda)  # float64 state: the result precision of _DIV64
        out32 = torch.empty(w, dtype=torch.float32, device=cuda)
        out64 = torch.empty(w, dtype=torch.float64, device=cuda)
        epi = None if op == "mean" else ops._epilogue(na.OP_BY_NAME[op], prev, v)
        ops.fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc, float(n), w, out32=out32, out64=out64, epi=epi)
        outs.append([t.cpu().numpy() for t in (out32, out64, v)])
    for a, b in zip(*outs):
        assert rr.same_bits(a, b)
    if op == "mean":
        assert rr.same_bits(outs[0][1], cr.clipped_mean(x[:n, :w], g[:w], sc))


def test_python_side_checks(data, cuda):
    x, g, dx, dg = data
    acc = torch.empty(STRIDE, dtype=torch.float32, device=cuda)
    sc = torch.ones(128, device=cuda)
    with pytest.raises(ValueError, match="at most 128"):
        ops.clip_fold_stack(torch.zeros((129, 8), device=cuda), dg, sc, None, acc)
    with pytest.raises(ValueError, match="center"):
        ops.clip_fold_stack(dx, dg[:100], sc, None, acc)
    with pytest.raises(ValueError, match="center"):
        ops.clip_fold_stack(dx, None, sc, None, acc)
    with pytest.raises(ValueError, match="scale"):
        ops.clip_fold_stack(dx, dg, sc[:5], None, acc)
    with pytest.raises(ValueError, match="acc_out"):
        ops.clip_fold_stack(dx, dg, sc, None, acc[:100])
    with pytest.raises(ValueError, match="acc_in"):
        ops.clip_fold_stack(dx, dg, sc, acc[:100], acc)
    with pytest.raises(ValueError, match="acc_in"):
        ops.clip_fold_stack(dx, dg, sc, acc.double(), acc)
    with pytest.raises(TypeError):
        ops.clip_fold_stack(dx.double(), dg, sc, None, acc)
    with pytest.raises(na.NativeError, match="overlap"):  # neither the same array nor a disjoint one
        ops.clip_fold_stack(dx, dg, sc, acc[4:], acc, n_cols=100)
    ops.clip_fold_stack(dx, dg, sc, acc, acc, n_cols=0)  # a no-op
    assert ops.last_launch()[0] is None
