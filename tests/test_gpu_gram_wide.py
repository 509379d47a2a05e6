"""GPU: fa_gram_f32_wide (panel_pair_kernel + panel_finish_kernel through ops.gram_stack(wide=True))
against numpy (tests/gram_ref.py), 129 .. 1024 clients.  Small-integer rows make every product and sum
exact, so the matrix must EQUAL the integer Gram; random floats are held to the derived bound
gamma(chain) S + slices 2^-52 S with chain and slices from the restated plan of the launch
(tests/gram_wide_ref.py).  Every run has guard words around gram_out and past the workspace."""
import numpy as np
import pytest
import torch

import gram_ref as gr
import gram_wide_ref as gw
from flearn_amd import ops
from test_gpu_gram import float_rows

pytestmark = pytest.mark.gpu

GUARD = 8
SENT64, SENT8 = -123456.0, 0xA5


@pytest.fixture(scope="module")
def cus(cuda):
    return torch.cuda.get_device_properties(cuda).multi_processor_count


def run(x, cuda, cus, c=None, col_begin=0, n_cols=None, forced=0):
    """(G, the restated plan) of one launch over the window; guards and the launch record checked."""
    n = x.shape[0]
    ncols = x.shape[1] - col_begin if n_cols is None else n_cols
    stack = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    center = None if c is None else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(cuda)
    need = ops.gram_workspace(n, ncols, wide=True)
    assert need == gw.workspace_bytes(n, ncols)
    out = torch.full((n * n + 2 * GUARD,), SENT64, dtype=torch.float64, device=cuda)
    work = torch.full((need + 64,), SENT8, dtype=torch.uint8, device=cuda)
    prev = ops.set_reduce_grid(forced)
    try:
        g = ops.gram_stack(stack, center=center, col_begin=col_begin, n_cols=ncols, out=out[GUARD : GUARD + n * n],
                           workspace=work[:need], wide=True)
        name, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    got = g.cpu().numpy().copy()
    host = out.cpu().numpy()
    assert (host[:GUARD] == SENT64).all() and (host[GUARD + n * n :] == SENT64).all(), "wrote outside gram_out[0, n^2)"
    assert (work[need:].cpu().numpy() == SENT8).all(), "wrote past the workspace"
    p = gw.launch_plan(n, ncols, cus, forced)
    assert name == f"panel_pair_kernel<{'true' if c is not None else 'false'}>" and launches == 2
    assert grid == p.slices * p.pairs and got.shape == (n, n)
    return got, p


def int_rows(shape, seed):
    """Integers in -7..7: with a centre likewise |y| <= 14, so 2053 products sum exactly in fp32."""
    return np.random.default_rng(seed).integers(-7, 8, shape).astype(np.float32)


def int_gram(x, c=None):
    """The integer Gram, exact in float64 (every sum is far below 2^53)."""
    y = x.astype(np.float64) - (0 if c is None else c.astype(np.float64)[None, :])
    return y @ y.T


# a last panel of one row, a ragged tile, exact panels, three panels (one row in the last), ragged and full size
@pytest.mark.parametrize("n", [129, 160, 256, 257, 1000, 1024])
def test_exact_integers(n, cuda, cus):
    """One column, the LDS chunk on both sides, two inner chains and a ragged end; the natural grid, one
    slice (crossing an Lc flush at width 2053) and three slices."""
    for width in (1, gw.KC - 1, gw.KC + 1, 2 * gw.LC + 5):
        stride = -(-width // 4) * 4
        x = np.full((n, stride), np.nan, np.float32)
        x[:, :width] = int_rows((n, width), n + width)
        x[:, 0] = (np.arange(n) % 15) - 7  # row i is recognisable
        c = np.full(stride, np.nan, np.float32)
        c[:width] = int_rows(width, width)
        for centre in (None, c):
            want = int_gram(x[:, :width], None if centre is None else c[:width])
            for forced in (0, 1, 3):
                got, p = run(x, cuda, cus, centre, n_cols=width, forced=forced)
                assert np.array_equal(got, want), (n, width, centre is not None, forced)
                assert forced == 0 or p.slices == min(forced, p.chunks)


@pytest.mark.parametrize("n,width,forced", [(200, 4099, 0), (513, 2600, 1), (1024, 3001, 0)])
def test_random_floats_within_the_derived_bound(n, width, forced, cuda, cus):
    stride = -(-width // 4) * 4
    xs = np.zeros((n, stride), np.float32)
    xs[:, :width] = float_rows(n, width, n + width)
    got, p = run(xs, cuda, cus, n_cols=width, forced=forced)
    err, tol = np.abs(got - gr.gram(xs[:, :width])), gw.bound(xs[:, :width], None, p)
    print(f"n={n} width={width} slices={p.slices} chain={p.chain} max err/bound={np.max(err / tol):.3e}")
    assert (err <= tol).all()
    # centred: models of one round, g + delta with delta much smaller than g
    rng = np.random.default_rng(width)
    c = rng.standard_normal(stride).astype(np.float32)
    xc = (c[None, :] + 1e-2 * rng.standard_normal((n, stride))).astype(np.float32)
    got, p = run(xc, cuda, cus, c, n_cols=width, forced=forced)
    err, tol = np.abs(got - gr.gram(xc[:, :width], c[:width])), gw.bound(xc[:, :width], c[:width], p)
    print(f"  centred max err/bound={np.max(err / np.maximum(tol, 1e-300)):.3e}")
    assert (err <= tol).all()


def test_bitwise_properties(cuda, cus):
    n, width = 200, 2049  # a ragged last panel: 72 rows
    x = np.zeros((n, -(-width // 4) * 4), np.float32)
    x[:, :width] = float_rows(n, width, 3 * n)
    g1, _ = run(x, cuda, cus, n_cols=width)
    g2, _ = run(x, cuda, cus, n_cols=width)
    assert g1.tobytes() == g2.tobytes()  # the same inputs and plan: the same bits
    assert g1.tobytes() == np.ascontiguousarray(g1.T).tobytes()  # symmetric bit for bit
    perm = np.random.default_rng(n).permutation(n)
    gp, _ = run(x[perm], cuda, cus, n_cols=width)
    assert gp.tobytes() == np.ascontiguousarray(g1[np.ix_(perm, perm)]).tobytes()  # G'[i][j] == G[p_i][p_j]


def test_non_finite_rows_touch_their_rows_and_columns_only(cuda, cus):
    n, width = 300, 1500
    x = float_rows(n, width, 11 * n)
    bad_inf, bad_nan = 5, 290  # panels 0 and 2
    poisoned, zeroed = x.copy(), x.copy()
    poisoned[bad_inf] = np.inf
    poisoned[bad_nan, 777] = np.nan
    zeroed[[bad_inf, bad_nan]] = 0
    gp, _ = run(poisoned, cuda, cus)
    gz, _ = run(zeroed, cuda, cus)
    bad = np.zeros((n, n), bool)
    bad[[bad_inf, bad_nan], :] = True
    bad[:, [bad_inf, bad_nan]] = True
    assert (~np.isfinite(gp[bad])).all() and np.isfinite(gp[~bad]).all()
    assert gp[~bad].tobytes() == gz[~bad].tobytes()


def test_window_inside_wider_rows(cuda, cus):
    """col_begin > 0 and a stride past the window, NaN on both sides, in the stack and in the centre."""
    n = 260
    for col, ncols in ((64, 1000), (128, 1280 - 3), (4, 1)):
        x = np.full((n, 1408), np.nan, np.float32)
        c = np.full(1408, np.nan, np.float32)
        x[:, col : col + ncols] = int_rows((n, ncols), n + col)
        c[col : col + ncols] = int_rows(ncols, col)
        assert np.array_equal(run(x, cuda, cus, col_begin=col, n_cols=ncols)[0], int_gram(x[:, col : col + ncols]))
        assert np.array_equal(run(x, cuda, cus, c, col_begin=col, n_cols=ncols)[0],
                              int_gram(x[:, col : col + ncols], c[col : col + ncols]))


def test_python_refusals_and_the_narrow_depths(cuda):
    with pytest.raises(ValueError, match="1024"):
        ops.gram_stack(torch.zeros((1025, 64), dtype=torch.float32, device=cuda), wide=True)
    with pytest.raises(ValueError, match="128"):
        ops.gram_stack(torch.zeros((129, 64), dtype=torch.float32, device=cuda))
    x = torch.ones((100, 64), dtype=torch.float32, device=cuda)
    g = ops.gram_stack(x, wide=True)  # up to 128 clients the wide entry is fa_gram_f32's launch
    assert ops.last_launch()[0].startswith("gram_kernel_tile<128,") and (g.cpu().numpy() == 64.0).all()
