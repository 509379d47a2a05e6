"""GPU: fa_set_reduce_grid is one setting for the whole library.

The entry that stores the forced grid and the entries that read it are compiled as different units
(flearn_amd/_build.py SOURCES; the shared state is in fa_host.hpp).  With a grid of 2 forced, one
fa_reduce_f32 (plain mean), one fa_fold (FA_ACC_F32, a round's first chunk) and one fa_trim_sum
(FA_ACC_F32) over 3 clients x 4096 fp32 columns, and one fa_reduce_f16 (np.float32 weights) over the
same 3 clients x 8192 halves — 16 one-KiB chunks per row, which plan_f32_window, plan_fold_window,
plan_trim_window and plan_f16_window (fa_geometry.hpp) put on 16 blocks when left alone and on
exactly the forced 2 otherwise — must each report grid 2 in fa_last_launch, with results bit-equal
to the references the neighbouring tests use."""
import numpy as np
import pytest
import torch

import half_ref
import oracle
import robust_ref as rr
from flearn_amd import _native as na
from flearn_amd import ops, semantics

pytestmark = pytest.mark.gpu

N, NCOLS, FORCED = 3, 4096, 2
NHALVES = 8192  # the same 16 one-KiB chunks of a row in float16


def running_sum_f32(x, w):
    """acc = w0*x0; acc += wi*xi in list order, every product and sum rounded to fp32."""
    acc = w[0] * x[0]
    for i in range(1, len(w)):
        acc = acc + w[i] * x[i]
    return acc


def test_forced_grid_reaches_reduce_fold_and_trim(cuda):
    rng = np.random.default_rng(20)
    x = (rng.standard_normal((N, NCOLS)) * np.exp(rng.uniform(-6, 6, (N, NCOLS)))).astype(np.float32)
    w = rng.uniform(0.25, 3.0, N).astype(np.float32)
    denom = float(np.sum(w.astype(np.float64)))
    stack, weights = torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda)
    out64 = torch.empty(NCOLS, dtype=torch.float64, device=cuda)
    folded = torch.empty(NCOLS, dtype=torch.float32, device=cuda)
    trimmed = torch.empty(NCOLS, dtype=torch.float32, device=cuda)
    x16 = (rng.standard_normal((N, NHALVES)) * np.exp(rng.uniform(-6, 6, (N, NHALVES)))).astype(np.float16)
    num = semantics.resolve_half([np.float32(v) for v in w], "numpy")
    assert num.mode == na.MODE_H16_W32
    stack16, weights16 = torch.from_numpy(x16).to(cuda), torch.from_numpy(num.weights.astype(np.float32)).to(cuda)
    half32 = torch.empty(NHALVES, dtype=torch.float32, device=cuda)

    def launches():
        ops.reduce_stack(stack, weights, na.MODE_W32_DIV64, denom, out64=out64)
        yield ops.last_launch()
        ops.fold_stack(na.ACC_F32, stack, weights, None, folded)
        yield ops.last_launch()
        ops.trim_sum_stack(na.ACC_F32, stack, 1, trimmed)
        yield ops.last_launch()
        ops.reduce_stack_f16(stack16, weights16, num.mode, num.denom, out32=half32)
        yield ops.last_launch()

    natural = list(launches())
    assert [g for _, g, _ in natural] == [16, 16, 16, 16], natural  # one block per chunk when nothing is forced
    prev = ops.set_reduce_grid(FORCED)
    try:
        forced = list(launches())
    finally:
        ops.set_reduce_grid(0)
    assert prev == 0
    print("forced launches:", forced)
    families = ("reduce_kernel_rows<", "fold_kernel_rows<", "trim_kernel_rows<", "reduce_kernel_rows_h16<")
    assert len(forced) == len(families)
    for (name, grid, n), family in zip(forced, families):
        assert name.startswith(family) and grid == FORCED and n == 1, (name, grid, n)
    assert rr.same_bits(out64.cpu().numpy(), oracle.c_reduce(oracle.MODE_W32_DIV64, x, w, denom))
    assert rr.same_bits(folded.cpu().numpy(), running_sum_f32(x, w))
    assert rr.same_bits(trimmed.cpu().numpy(), rr.trimmed_sum(x, 1))
    q = half_ref.reduce_rows(num.mode, x16, num.weights, num.denom)
    assert q.dtype == np.float32 and half_ref.same_bits(half32.cpu().numpy(), q)
