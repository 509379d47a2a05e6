"""GPU: fa_rownorm2_f32 (ops.rownorm2_stack), the clients' squared update norms.

Integer data whose every partial sum stays below 2^24 makes the result independent of the summation
order, so it must EQUAL numpy's float64 sum bit for bit: client counts around the 64-lane running-sum
registers, widths around the piece boundaries, natural and forced grids.  Random floats are held to the
DERIVED bound (gamma(chain) + grid * 2^-52) * d2_ref with chain and grid from the plan
(tests/clip_ref.py, checked against the C++ by tests/test_clip_host.py), with no measured slack."""
import numpy as np
import pytest
import torch

import clip_ref as cr
from flearn_amd import ops

pytestmark = pytest.mark.gpu

P = cr.piece_cols(16)  # the columns of the widest piece
NS = (1, 2, 3, 63, 64, 65, 100, 128)
WIDTHS = (1, 3, 4, 255, P - 1, P, P + 1, 3 * P + 5)
STRIDE = (3 * P + 5 + 3) // 4 * 4


@pytest.fixture(scope="module")
def ints(cuda):
    """[128, STRIDE] rows of integers in [-3, 3] and a centre in [-2, 2]: squares <= 25, and 25 * STRIDE
    < 2^24, so every fp32 partial sum is an exact integer."""
    rng = np.random.default_rng(7)
    x = rng.integers(-3, 4, (128, STRIDE)).astype(np.float32)
    g = rng.integers(-2, 3, STRIDE).astype(np.float32)
    assert 25 * STRIDE < 2**24
    return x, g, torch.from_numpy(x).to(cuda), torch.from_numpy(g).to(cuda)


@pytest.fixture(scope="module")
def cus(cuda):
    return torch.cuda.get_device_properties(cuda).multi_processor_count


def exact(x, g, n, c0, w):
    d = x[:n, c0 : c0 + w].astype(np.int64) - (0 if g is None else g[c0 : c0 + w].astype(np.int64))
    return (d * d).sum(axis=1).astype(np.float64)


def launch(dx, dg, n, w, forced, c0=0, cus=None):
    prev = ops.set_reduce_grid(forced)
    try:
        out = ops.rownorm2_stack(dx, center=dg, n_clients=n, col_begin=c0, n_cols=w)
        kernel, grid, launches = ops.last_launch()
    finally:
        ops.set_reduce_grid(prev)
    if cus is not None:
        p = cr.launch_plan(n, w, cus, forced)
        assert kernel == cr.instance("rownorm_kernel", p.V) and grid == p.grid and launches == 2
    return out.cpu().numpy()


@pytest.mark.parametrize("w", WIDTHS)
def test_exact_integers(w, ints, cus):
    x, g, dx, dg = ints
    for n in NS:
        want = exact(x, g, n, 0, w)
        for forced in (0, 1, 2):
            got = launch(dx, dg, n, w, forced, cus=cus)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (n, w, forced)
    got = launch(dx, None, 65, w, 0, cus=cus)  # no centre: y = x
    assert got.tobytes() == exact(x, None, 65, 0, w).tobytes()


def test_every_shipped_instantiation_is_launched(ints, cus):
    x, g, dx, dg = ints
    seen = set()
    for v, (w, forced) in cr.COVER.items():
        for n in (1, 16 // v + 1, 100):
            prev = ops.set_reduce_grid(forced)
            try:
                got = ops.rownorm2_stack(dx, center=dg, n_clients=n, n_cols=w).cpu().numpy()
                kernel, grid, launches = ops.last_launch()
            finally:
                ops.set_reduce_grid(prev)
            assert kernel == cr.instance("rownorm_kernel", v) and (grid, launches) == (1, 2)
            assert got.tobytes() == exact(x, g, n, 0, w).tobytes(), (v, n)
            seen.add(kernel)
    assert seen == {t for t in cr.TARGETS if t.startswith("rownorm_kernel")}


def test_window_inside_wider_rows(cuda, cus):
    rng = np.random.default_rng(8)
    stride, c0, w = 1400, 260, 777
    x = rng.integers(-3, 4, (9, stride)).astype(np.float32)
    g = rng.integers(-2, 3, stride).astype(np.float32)
    want = exact(x, g, 9, c0, w)
    for sentinel in (np.nan, np.inf, 1e30):
        xs, gs = x.copy(), g.copy()
        xs[:, :c0] = sentinel
        xs[:, c0 + w :] = sentinel
        gs[:c0] = sentinel
        gs[c0 + w :] = -sentinel
        got = launch(torch.from_numpy(xs).to(cuda), torch.from_numpy(gs).to(cuda), 9, w, 0, c0, cus)
        assert got.tobytes() == want.tobytes(), sentinel


@pytest.mark.parametrize("n,w,forced", [(10, 5000, 0), (33, 3001, 2), (100, 4099, 0), (128, 2600, 1)])
def test_random_floats_within_the_derived_bound(n, w, forced, cuda, cus):
    rng = np.random.default_rng(n)
    stride = (w + 3) // 4 * 4
    x = (rng.standard_normal((n, stride)) * 10.0 ** rng.integers(-3, 4, (n, 1))).astype(np.float32)
    g = rng.standard_normal(stride).astype(np.float32)
    want = cr.norm2(x[:, :w], g[:w])
    bound = cr.norm_bound(cr.launch_plan(n, w, cus, forced))
    got = launch(torch.from_numpy(x).to(cuda), torch.from_numpy(g).to(cuda), n, w, forced, cus=cus)
    err = np.abs(got - want) / want
    print(f"rownorm {n} x {w} grid {forced}: worst error {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all(), (err.max(), bound)
    again = launch(torch.from_numpy(x).to(cuda), torch.from_numpy(g).to(cuda), n, w, forced, cus=cus)
    assert again.tobytes() == got.tobytes()  # the same inputs and grid give the same bits


def test_a_non_finite_value_touches_its_own_row_only(ints, cus):
    x, g, dx, dg = ints
    n, w = 100, P + 1
    clean = launch(dx, dg, n, w, 0, cus=cus)
    for forced in (0, 2):
        bad = dx[:n].clone()
        where = {3: (np.nan, 0), 64: (np.inf, w - 1), 77: (-np.inf, 5000), 99: (np.nan, P)}
        for i, (v, c) in where.items():
            bad[i, c] = v
        bad[5, w] = np.nan  # outside the window: nobody's norm
        got = launch(bad, dg, n, w, forced, cus=cus)
        for i in range(n):
            if i in where:
                assert not np.isfinite(got[i]), i
            else:
                assert got[i] == clean[i], i
    assert np.isnan(launch(bad, dg, n, w, 0, cus=cus)[3]) and np.isinf(launch(bad, dg, n, w, 0, cus=cus)[64])


def test_python_side_checks(ints, cuda):
    x, g, dx, dg = ints
    with pytest.raises(ValueError, match="at most 128"):
        ops.rownorm2_stack(torch.zeros((129, 8), device=cuda))
    with pytest.raises(ValueError, match="empty"):
        ops.rownorm2_stack(dx, n_cols=0)
    with pytest.raises(TypeError):
        ops.rownorm2_stack(dx.double())
    with pytest.raises(ValueError, match="center"):
        ops.rownorm2_stack(dx, center=dg[:100])
    with pytest.raises(ValueError, match="workspace"):
        ops.rownorm2_stack(dx, n_cols=4096, workspace=torch.empty(8, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError, match="out"):
        ops.rownorm2_stack(dx, out=torch.empty(4, dtype=torch.float64, device=cuda))
    assert ops.rownorm_workspace(100, 25_610_152) == 512 * 100 * 4
