"""GPU: fa_clip_sum_f32 (ops.clip_sum_stack), bit for bit against tests/clip_ref.py's clipped_sum:
the running fp32 sum in list order of the rows under the three-way rule (s >= 1 the row, 0 < s < 1
fl32(g + fl32(s * fl32(x - g))), else the centre with the row unread).  Client counts around the
64-row boundaries and around every shipped pipeline depth's ramp and drain, widths around the piece
boundaries, every shipped instantiation named by fa_last_launch; then fa_fold_finish over the
accumulator with every fused op, against the fold path's accumulator."""
import numpy as np
import pytest
import torch

import clip_ref as cr
import robust_ref as rr
from flearn_amd import _native as na
from flearn_amd import ops

pytestmark = pytest.mark.gpu

P = cr.piece_cols(16)
NS = (1, 2, 3, 63, 64, 65, 100, 128)
WIDTHS = (1, 3, 4, 255, P - 1, P, P + 1, 3 * P + 5)
STRIDE = (3 * P + 5 + 3) // 4 * 4
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


def run(dx, dg, scale, n, w, forced=0, c0=0):
    acc = torch.full((w + GUARD,), 7.0, dtype=torch.float32, device=dx.device)
    ds = torch.from_numpy(np.ascontiguousarray(scale[:n], dtype=np.float32)).to(dx.device)
    prev = ops.set_reduce_grid(forced)
    try:
        ops.clip_sum_stack(dx, dg, ds, acc, n_clients=n, col_begin=c0, n_cols=w)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    out = acc.cpu().numpy()
    assert (out[w:] == 7.0).all(), "guard columns were written"
    assert launches == 1 and kernel.startswith("clip_sum_kernel<")
    return out[:w], kernel


def check(x, g, dx, dg, scale, n, w, forced=0, where=""):
    got, kernel = run(dx, dg, scale, n, w, forced)
    want = cr.clipped_sum(x[:n, :w], g[:w], scale)
    assert rr.same_bits(got, want), (where, n, w, forced, kernel)
    return got, kernel


def pattern(n, seed):
    rng = np.random.default_rng(seed)
    return MIXED[rng.integers(0, len(MIXED), n)]


@pytest.mark.parametrize("w", WIDTHS)
def test_mixed_scales_over_the_ladder(w, data):
    x, g, dx, dg = data
    for n in NS:
        check(x, g, dx, dg, pattern(n, n * 1000 + w), n, w, 0, "mixed")
    check(x, g, dx, dg, pattern(100, w), 100, w, 2, "mixed, 2 blocks")


def test_every_shipped_instantiation_and_its_ramp_and_drain(data):
    x, g, dx, dg = data
    seen = set()
    for v, (w, forced) in cr.COVER.items():
        d = 16 // v
        for n in sorted({1, 2, d - 1, d, d + 1, 2 * d, 2 * d + 1, 3 * d + 2} - {0}):
            for seed in (0, 1):
                _, kernel = check(x, g, dx, dg, pattern(n, 31 * n + seed), n, w, forced, "ramp/drain")
                assert kernel == cr.instance("clip_sum_kernel", v)
                seen.add(kernel)
    assert seen == {t for t in cr.TARGETS if t.startswith("clip_sum_kernel")}


@pytest.mark.parametrize("n,w", [(1, 255), (17, 4099), (64, P + 1), (100, 3001)])
def test_scale_patterns(n, w, data, cuda):
    x, g, dx, dg = data
    ones = np.ones(n, np.float32)
    got, _ = check(x, g, dx, dg, ones, n, w, 0, "all 1")
    acc = torch.empty(w, dtype=torch.float32, device=cuda)
    ops.fold_stack(na.ACC_F32, dx, torch.from_numpy(ones).to(cuda), None, acc, n_cols=w, n_clients=n)
    assert rr.same_bits(got, acc.cpu().numpy())  # the unit-weight fold's bits
    assert np.signbit(got[2]) and got[2] == 0  # an all -0.0 column stays -0.0
    zeros, _ = check(x, g, dx, dg, np.zeros(n, np.float32), n, w, 0, "all 0")
    chain = g[:w].copy()
    for _ in range(1, n):
        chain = (chain + g[:w]).astype(np.float32)
    assert rr.same_bits(zeros, chain)
    for s0 in (0.0, 0.25, 1.0):  # row 0 initialises the sum under each branch
        sc = pattern(n, n + w)
        sc[0] = s0
        check(x, g, dx, dg, sc, n, w, 0, f"row 0 at {s0}")
    alt = np.where(np.arange(n) % 2 == 0, np.float32(1.0), np.float32(0.5)).astype(np.float32)
    check(x, g, dx, dg, alt, n, w, 0, "alternating")
    check(x, g, dx, dg, alt[::-1].copy() * np.float32(0.5), n, w, 0, "alternating 0.5 / 0.25")


def test_the_three_way_rule_on_odd_scales(data):
    x, g, dx, dg = data
    n, w = 12, 1000
    for s, like in ((1.0, 1.0), (1.5, 1.0), (np.inf, 1.0), (0.0, 0.0), (-0.0, 0.0), (-3.0, 0.0), (np.nan, 0.0),
                    (-np.inf, 0.0)):
        a, _ = run(dx, dg, np.full(n, s, np.float32), n, w)
        b, _ = run(dx, dg, np.full(n, like, np.float32), n, w)
        assert rr.same_bits(a, b), s
    tiny = np.full(n, 1e-42, np.float32)  # a denormal scale is a scale in (0, 1)
    check(x, g, dx, dg, tiny, n, w, 0, "denormal scale")


def test_rows_with_scale_zero_are_not_read(data):
    x, g, dx, dg = data
    n, w = 33, P + 1
    sc = pattern(n, 5)
    sc[[0, 4, 32]] = 0.0
    bad = dx[:n].clone()
    bad[0] = float("nan")
    bad[4] = float("inf")
    bad[32, ::2] = float("-inf")
    got, _ = run(bad, dg, sc, n, w)
    want = cr.clipped_sum(x[:n, :w], g[:w], sc)  # the clean rows: a replaced row's values do not matter
    assert rr.same_bits(got, want)
    finite_cols = np.isfinite(want)
    assert np.isfinite(got[finite_cols]).all()


def test_window_inside_wider_rows(data):
    x, g, dx, dg = data
    n, w, c0 = 9, 777, 260
    sc = pattern(n, 9)
    got, _ = run(dx, dg, sc, n, w, 0, c0)
    assert rr.same_bits(got, cr.clipped_sum(x[:n, c0 : c0 + w], g[c0 : c0 + w], sc))


@pytest.mark.parametrize("op", ["mean", "avgm", "adagrad", "yogi", "adam"])
def test_fold_finish_takes_the_accumulator(op, data, cuda):
    """The clipped sum against the fold of the clipped rows (computed by clip_ref, uploaded), then
    fa_fold_finish with the fused op over both accumulators: the same bits in w, v and prev."""
    x, g, dx, dg = data
    n, w = 20, 4099
    sc = pattern(n, 77)
    sc[sc != sc] = 0.0
    yhat = np.stack([cr.clipped_upload(x[i, :w], g[:w], sc[i]) for i in range(n)])
    dy = torch.from_numpy(np.ascontiguousarray(np.pad(yhat, ((0, 0), (0, -w % 4))))).to(cuda)
    acc_fold = torch.empty(w, dtype=torch.float32, device=cuda)
    ops.fold_stack(na.ACC_F32, dy, torch.ones(n, device=cuda), None, acc_fold, n_cols=w, n_clients=n)
    acc_clip = torch.empty(w, dtype=torch.float32, device=cuda)
    ops.clip_sum_stack(dx, dg, torch.from_numpy(sc).to(cuda), acc_clip, n_clients=n, n_cols=w)
    assert rr.same_bits(acc_clip.cpu().numpy(), acc_fold.cpu().numpy())
    outs = []
    for acc in (acc_clip, acc_fold):
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
        ops.clip_sum_stack(torch.zeros((129, 8), device=cuda), dg, sc, acc)
    with pytest.raises(ValueError, match="center"):
        ops.clip_sum_stack(dx, dg[:100], sc, acc)
    with pytest.raises(ValueError, match="center"):
        ops.clip_sum_stack(dx, None, sc, acc)
    with pytest.raises(ValueError, match="scale"):
        ops.clip_sum_stack(dx, dg, sc[:5], acc)
    with pytest.raises(ValueError, match="acc_out"):
        ops.clip_sum_stack(dx, dg, sc, acc[:100])
    with pytest.raises(TypeError):
        ops.clip_sum_stack(dx.double(), dg, sc, acc)
    ops.clip_sum_stack(dx, dg, sc, acc, n_cols=0)  # a no-op
    assert ops.last_launch()[0] is None
