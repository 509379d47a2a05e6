"""GPU: fa_gram_f32 (gram_kernel_tile + gram_finish_kernel through ops.gram_stack) against numpy
(tests/gram_ref.py).  Small-integer rows make every product and sum exact, so the matrix must EQUAL
the integer Gram — rows different per client and asymmetric, which is what catches swapped operand
rows / columns and a wrong k map; random floats are held to the derived bound
gamma(chain) S + grid 2^-52 S with chain and grid from the plan of the launch.  Every run has guard
words around gram_out and past the workspace."""
import numpy as np
import pytest
import torch

import gram_ref as gr
from flearn_amd import ops
from instantiation_cases import gram_name

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 3, 31, 32, 33, 64, 65, 100, 128)
GUARD = 8
SENT64, SENT8 = -123456.0, 0xA5


@pytest.fixture(scope="module")
def cus(cuda):
    return torch.cuda.get_device_properties(cuda).multi_processor_count


def run(x, cuda, c=None, col_begin=0, n_cols=None, forced=0):
    """(G, kernel name, grid) of one launch over the window; guards checked."""
    n = x.shape[0]
    ncols = x.shape[1] - col_begin if n_cols is None else n_cols
    stack = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    center = None if c is None else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(cuda)
    need = ops.gram_workspace(n, ncols)
    assert need == gr.workspace_bytes(n, ncols)
    out = torch.full((n * n + 2 * GUARD,), SENT64, dtype=torch.float64, device=cuda)
    work = torch.full((need + 64,), SENT8, dtype=torch.uint8, device=cuda)
    prev = ops.set_reduce_grid(forced)
    try:
        g = ops.gram_stack(stack, center=center, col_begin=col_begin, n_cols=ncols, out=out[GUARD : GUARD + n * n],
                           workspace=work[:need])
        name, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    got = g.cpu().numpy().copy()
    host = out.cpu().numpy()
    assert (host[:GUARD] == SENT64).all() and (host[GUARD + n * n :] == SENT64).all(), "wrote outside gram_out[0, n^2)"
    assert (work[need:].cpu().numpy() == SENT8).all(), "wrote past the workspace"
    assert launches == 2 and got.shape == (n, n)
    return got, name, grid


def int_rows(n, width, seed):
    """Small integers in -8..8, every row different, G far from symmetric in any accidental way."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (n, width)).astype(np.float32)
    x[:, 0] = (np.arange(n) % 17) - 8  # row i is recognisable
    return x


def int_gram(x, c=None):
    y = x.astype(np.int64) - (0 if c is None else c.astype(np.int64)[None, :])
    return (y @ y.T).astype(np.float64)


@pytest.mark.parametrize("n", DEPTHS)
def test_exact_integers_every_depth(n, cuda, cus):
    x = int_rows(n, 1000, n)
    c = np.random.default_rng(1000 + n).integers(-8, 9, 1000).astype(np.float32)
    for centre in (None, c):
        got, name, grid = run(x, cuda, centre)
        assert np.array_equal(got, int_gram(x, centre)), (n, centre is not None)
        p = gr.launch_plan(n, 1000, cus)
        assert name == gram_name(p.np_, centre is not None)
        assert grid == p.grid and p.np_ >= n


def test_exact_integers_widest(cuda):
    x = int_rows(100, 4096, 5)
    c = np.random.default_rng(6).integers(-8, 9, 4096).astype(np.float32)
    assert np.array_equal(run(x, cuda)[0], int_gram(x))
    assert np.array_equal(run(x, cuda, c)[0], int_gram(x, c))


@pytest.mark.parametrize("n", [3, 64, 70, 100])  # NP 32, 64, 96, 128
def test_widths(n, cuda, cus):
    """Ragged ends, one column, the LDS chunk and the inner chain on both sides, unequal shares."""
    kc = gr.gram_kc(gr.gram_np(n))
    cases = [(w, 0) for w in (1, 63, 64, 65, 257, kc - 1, kc, kc + 1, 2 * kc + 1)]
    cases += [(gr.LC - 1, 1), (gr.LC, 1), (gr.LC + 1, 1), (2 * gr.LC + kc + 3, 1), (4 * kc + 5, 3)]  # 5 chunks on 3 blocks
    for width, forced in cases:
        stride = -(-width // 4) * 4
        x = np.full((n, stride), np.nan, np.float32)
        x[:, :width] = int_rows(n, width, width + n)
        got, _, grid = run(x, cuda, n_cols=width, forced=forced)
        assert np.array_equal(got, int_gram(x[:, :width])), (n, width, forced)
        p = gr.launch_plan(n, width, cus, forced)
        assert grid == p.grid, (n, width, forced)
        if forced == 3:
            assert grid == 3 and p.chunks % 3 != 0  # unequal shares
        if forced == 1:
            assert grid == 1


def test_window_inside_wider_rows(cuda):
    """col_begin > 0, NaN on both sides of the window, in the stack and in the centre."""
    for n in (5, 100):
        x = np.full((n, 1408), np.nan, np.float32)
        c = np.full(1408, np.nan, np.float32)
        for col, ncols in ((64, 1000), (128, 1280 - 3), (4, 1)):
            x[:] = np.nan
            c[:] = np.nan
            x[:, col : col + ncols] = int_rows(n, ncols, n + col)
            c[col : col + ncols] = np.random.default_rng(col).integers(-8, 9, ncols)
            assert np.array_equal(run(x, cuda, col_begin=col, n_cols=ncols)[0], int_gram(x[:, col : col + ncols]))
            assert np.array_equal(run(x, cuda, c, col_begin=col, n_cols=ncols)[0],
                                  int_gram(x[:, col : col + ncols], c[col : col + ncols]))


def float_rows(n, width, seed):
    """|x| in [2^-20, 2^20], signs mixed: no product underflows or overflows."""
    rng = np.random.default_rng(seed)
    return (np.ldexp(rng.uniform(1.0, 2.0, (n, width)), rng.integers(-20, 20, (n, width)))
            * rng.choice([-1.0, 1.0], (n, width))).astype(np.float32)


@pytest.mark.parametrize("n,width,forced", [(10, 5000, 0), (33, 3001, 2), (100, 4099, 0), (128, 2600, 1), (7, 70001, 0)])
def test_random_floats_within_the_derived_bound(n, width, forced, cuda, cus):
    x = float_rows(n, width, n + width)
    stride = -(-width // 4) * 4
    xs = np.zeros((n, stride), np.float32)
    xs[:, :width] = x
    p = gr.launch_plan(n, width, cus, forced)
    got, _, grid = run(xs, cuda, n_cols=width, forced=forced)
    assert grid == p.grid
    err, tol = np.abs(got - gr.gram(x)), gr.bound(x, None, p)
    print(f"n={n} width={width} grid={grid} chain={p.chain} max err/bound={np.max(err / tol):.3e}")
    assert (err <= tol).all()
    # centred: models of one round, g + delta with delta much smaller than g
    rng = np.random.default_rng(width)
    c = rng.standard_normal(stride).astype(np.float32)
    xc = (c[None, :] + 1e-2 * rng.standard_normal((n, stride))).astype(np.float32)
    got, _, _ = run(xc, cuda, c, n_cols=width, forced=forced)
    err, tol = np.abs(got - gr.gram(xc[:, :width], c[:width])), gr.bound(xc[:, :width], c[:width], p)
    print(f"  centred max err/bound={np.max(err / np.maximum(tol, 1e-300)):.3e}")
    assert (err <= tol).all()


@pytest.mark.parametrize("n,width", [(10, 3000), (100, 2049)])
def test_bitwise_properties(n, width, cuda):
    x = np.zeros((n, -(-width // 4) * 4), np.float32)
    x[:, :width] = float_rows(n, width, 3 * n)
    g1, _, _ = run(x, cuda, n_cols=width)
    g2, _, _ = run(x, cuda, n_cols=width)
    assert g1.tobytes() == g2.tobytes()  # the same inputs and plan: the same bits
    assert g1.tobytes() == np.ascontiguousarray(g1.T).tobytes()  # symmetric bit for bit
    perm = np.random.default_rng(n).permutation(n)
    gp, _, _ = run(x[perm], cuda, n_cols=width)
    assert gp.tobytes() == np.ascontiguousarray(g1[np.ix_(perm, perm)]).tobytes()  # G'[i][j] == G[p_i][p_j]


@pytest.mark.parametrize("n", [10, 70])
def test_non_finite_rows_touch_their_rows_and_columns_only(n, cuda):
    width = 1500
    x = float_rows(n, width, 11 * n)
    bad_inf, bad_nan = 2, n - 3
    poisoned = x.copy()
    poisoned[bad_inf] = np.inf
    poisoned[bad_nan, 777] = np.nan
    zeroed = x.copy()
    zeroed[bad_inf] = 0
    zeroed[bad_nan] = 0
    gp, _, _ = run(poisoned, cuda)
    gz, _, _ = run(zeroed, cuda)
    bad = np.zeros((n, n), bool)
    bad[[bad_inf, bad_nan], :] = True
    bad[:, [bad_inf, bad_nan]] = True
    assert (~np.isfinite(gp[bad])).all()
    assert np.isfinite(gp[~bad]).all()
    assert gp[~bad].tobytes() == gz[~bad].tobytes()


def test_checks_follow_trim_sum_stack(cuda):
    x = torch.zeros((4, 64), dtype=torch.float32, device=cuda)
    with pytest.raises(TypeError):
        ops.gram_stack(x.double())
    with pytest.raises(ValueError):
        ops.gram_stack(x.cpu())
    with pytest.raises(ValueError):
        ops.gram_stack(x, col_begin=60, n_cols=8)
    with pytest.raises(ValueError):
        ops.gram_stack(x, n_cols=0)
    with pytest.raises(ValueError):
        ops.gram_stack(x, center=torch.zeros(32, dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        ops.gram_stack(x, out=torch.zeros(15, dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        ops.gram_stack(torch.zeros((129, 64), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        ops.gram_stack(x, workspace=torch.zeros(16, dtype=torch.uint8, device=cuda))
    g = ops.gram_stack(x + 1.0)
    assert g.dtype == torch.float64 and g.shape == (4, 4) and (g.cpu().numpy() == 64.0).all()
