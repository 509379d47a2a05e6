"""GPU: every float16 reduce instantiation the library ships (reduce_kernel_rows_h16, 27 of them),
launched on a forced grid against the numpy restatement of the float16 table.

Each H16 case of tests/instantiation_cases.py names the kernel it means to reach; the launch record
(fa_last_launch) must name exactly that kernel on exactly the expected grid, and out64, out32 and
out16 must each be half_ref.same_bits to half_ref.reduce_rows — the restatement that
tests/test_half_host.py pins to the fixtures captured from the reference.  tests/test_kernel_inventory.py
closes the loop on a CPU box: the cases' targets are exactly the float16 kernels in the built library.

The inputs are those of tests/test_gpu_half.py (its helpers run the launch and the comparison):
make_stack's subnormals, +-0, near-overflow columns, inf and NaN; non-representable weights resolved
by semantics.resolve_half; a non-zero col_begin, NaN halves on both sides of the window in every row,
an odd column count with a partial last oct, and 96 sentinel elements after every output.  The
windows are a forced grid of 3 blocks x `share` one-KiB chunks: at most ~200 K halves, n <= 33."""
import numpy as np
import pytest
import torch

import half_ref
import test_gpu_half as th
from flearn_amd import aggregator as agg
from instantiation_cases import (H16_CASES, H16_MODE_NAMES, H16_MODES, h16_chunk_cols, h16_chunks, h16_plan_name,
                                 h16_rounds)

pytestmark = pytest.mark.gpu


@pytest.fixture
def grid():
    """Sets fa_set_reduce_grid for one test and puts the previous value back."""
    prev = []

    def set_grid(g):
        prev.append(agg.set_reduce_grid(g))

    yield set_grid
    if prev:
        agg.set_reduce_grid(prev[0])


def window_stack(n, col_begin, n_cols, seed):
    """make_stack's values in [col_begin, col_begin + n_cols), NaN in every row on both sides."""
    stride = th.round_up(col_begin + n_cols + 40, 8)
    x = th.make_stack(n, stride, seed)
    x[:, :col_begin] = np.float16(np.nan)
    x[:, col_begin + n_cols :] = np.float16(np.nan)
    return x


def _case_id(i):
    c = H16_CASES[i]
    return f"{i}-{H16_MODE_NAMES[c.mode]}-s{c.share}-n{c.n}"


@pytest.mark.parametrize("i", range(len(H16_CASES)), ids=_case_id)
def test_h16_instantiation_against_half_ref(i, cuda, grid):
    c = H16_CASES[i]
    assert c.n_cols % 2 == 1 and 0 < c.n_cols % 8 < 8 and c.col_begin > 0 and c.col_begin % 8 == 0
    want_grid = min(c.grid, h16_chunks(c.n_cols))
    x = window_stack(c.n, c.col_begin, c.n_cols, seed=2000 + i)
    assert np.isnan(x[:, c.col_begin - 1]).all() and np.isnan(x[:, c.col_begin + c.n_cols]).all()
    grid(c.grid)
    for outs in (("out64", "out32", "out16"),) + ((("out16",), ("out32",), ("out64",)) if c.alone else ()):
        th.check(cuda, H16_MODE_NAMES[c.mode], x, c.col_begin, c.n_cols, outs)  # bits and sentinels
        rec = agg.last_launch()
        print(f"case {i}: {rec}")
        assert rec == (c.target, want_grid, 1), f"the shape no longer reaches its kernel: launched {rec}"
    if c.share == 130:  # several rounds per block, pieces narrower than the slot
        v, w = (int(t) for t in c.target[:-1].split(",")[2:5:2])
        k = h16_rounds(c.target, want_grid, c.n_cols)
        pc = -(-h16_chunks(c.n_cols) // (want_grid * k))
        assert k >= 3 and pc < w * v, (k, pc)


def test_the_cases_launch_every_policy_alone():
    assert sorted(c.mode for c in H16_CASES if c.alone) == sorted(H16_MODES)


# ---------------------------------------------------------------------------------------------
# "Results never depend on it" (fa_set_reduce_grid), float16
# ---------------------------------------------------------------------------------------------

GRIDS = (0, 1, 2, 3, 5)


@pytest.mark.parametrize("mode_name", H16_MODE_NAMES)
@pytest.mark.parametrize("chunks", [27, 70])
def test_h16_results_do_not_depend_on_the_grid(chunks, mode_name, cuda, grid):
    """The same 9 clients over an odd window of 27 (and 70) chunks on the natural grid and on forced
    grids of 1, 2, 3 and 5 blocks: identical bytes in out64, out32 and out16, the natural grid's equal
    to half_ref.  On one block the 70-chunk window takes several rounds under every policy (its widest
    piece is 64, 32 or 16 chunks); the 27-chunk window fits the 32-chunk piece of the policies with
    VMAX >= 8 and takes two rounds under AccH16W64 (VMAX 4), which k, computed from the launched
    instantiation's V and W and the grid as the kernel computes it, shows."""
    mode = th.MODES[mode_name]
    n, col_begin, n_cols = 9, 72, h16_chunk_cols(chunks)
    x = window_stack(n, col_begin, n_cols, seed=chunks)
    num = th.weights_for(mode_name, n)
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    results, names = [], set()
    for g in GRIDS:
        grid(g)
        got = th.run_kernel(cuda, mode, x, num, col_begin, n_cols)
        name, launched_grid, launches = agg.last_launch()
        print(f"grid {g}: {name} on {launched_grid}")
        assert (name, launched_grid) == h16_plan_name(mode, n_cols, cus, g) and launches == 1
        assert launched_grid == (min(g, chunks) if g else min(int(cus * 0.75 + 0.5), chunks))
        k = h16_rounds(name, launched_grid, n_cols)
        if g == 1:
            assert (k >= 2) == (chunks == 70 or H16_MODES[mode][2] < 8), k
        names.add(name)
        results.append(got)
        for key, fill in (("out64", -7.0), ("out32", -7.0), ("out16", np.int16(0x1234).view(np.float16))):
            assert len(got[key]) == n_cols + th.SENTINEL
            assert (got[key][n_cols:] == fill).all(), (g, key, "stored past the window")
    q = half_ref.reduce_rows(mode, np.ascontiguousarray(x[:, col_begin : col_begin + n_cols]), num.weights, num.denom)
    for key, want in zip(("out64", "out32", "out16"), half_ref.outputs(q)):
        assert half_ref.same_bits(results[0][key][:n_cols], want), (mode_name, key)
        for g, got in zip(GRIDS[1:], results[1:]):
            assert got[key].tobytes() == results[0][key].tobytes(), (mode_name, key, g)
    assert len(names) >= 2, names  # the grids did take different kernels
