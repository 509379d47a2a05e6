"""GPU: every kernel family on operands whose addresses lie past the 2 GiB and 4 GiB offsets from
the pointers the entry is given (tests/far_operands.py carves them out of one sentinel-filled arena).

Each entry goes through its flearn_amd.ops call and is compared bit for bit, NaN positions equal, with
the restatement the suite already has (the C oracle, robust_ref, gram_ref, clip_ref, clipfold_ref,
quant_ref, quant4_ref, half_ref) and with the same entry run on a compact copy of the same window.
After every test the whole arena must be back on its sentinel: a kernel that wrote anywhere it was
not asked to fails the test.  The far layouts keep every wrapped address inside the arena, so a
32-bit slip shows as a mismatch."""
import numpy as np
import pytest
import torch

import clip_ref as cr
import clipfold_ref as cfr
import far_operands as fo
import gram_ref as gr
import half_ref
import oracle
import quant4_ref as q4r
import quant_ref as qr
import robust_ref as rr
from flearn_amd import _native as na
from flearn_amd import ops

pytestmark = pytest.mark.gpu

LAYOUTS = ("far_rows", "far_window")
WIDTHS = (1, 1003, 40_003)  # one column, ragged, several pieces under the forced grid of 3
ACC_NP = {na.ACC_F32: np.float32, na.ACC_F32_W64: np.float64, na.ACC_F64: np.float64, na.ACC_I64: np.int64}


@pytest.fixture(scope="module")
def arena(cuda):
    reason = fo.skip_reason(cuda)
    if reason:
        pytest.skip(reason)
    torch.cuda.reset_peak_memory_stats(cuda)
    a = fo.Arena(cuda)
    yield a
    print(f"\nfar-address tests: peak device memory {torch.cuda.max_memory_allocated(cuda) / fo.GIB:.2f} GiB")
    del a.words, a._typed
    torch.cuda.empty_cache()


@pytest.fixture
def far(arena):
    """The arena, restored to its sentinel whatever becomes of the test; the forced grid undone."""
    prev = ops.set_reduce_grid(0)
    yield arena
    ops.set_reduce_grid(prev)
    torch.cuda.synchronize()
    arena.restore()


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.cpu().numpy()


def grid_for(width):
    ops.set_reduce_grid(3 if width > 4096 else 0)


# The reduce families the cases mean to reach (fa_last_launch's spelling).  apply_update, apply_dyn,
# fill_uniform and fa_copy record no launch: nothing can be asserted for them.
SMALL_REDUCE = "reduce_kernel_narrow<"  # a window of at most a few chunks
PIECES_REDUCE = "reduce_kernel_rows<"  # 157 chunks on a forced grid of 3
LONG_REDUCE = "reduce_kernel_rowmajor<"  # 2^30 columns


def launched(family):
    kernel, grid, launches = ops.last_launch()
    assert kernel is not None and kernel.startswith(family) and grid >= 1, (kernel, family)
    return kernel


def lay_out(far, layout, x, **kw):
    """(stack, col_begin) of host window x in the layout."""
    if layout == "far_rows":
        return fo.far_rows(far, x, **kw)
    return fo.far_window(far, x, **kw)


def compact(x, cuda, col_begin=8):
    """The same window at column 8 of an ordinary small stack, NaN (or a large integer) around it."""
    n, w = x.shape
    stride = -(-(col_begin + w + 16) // 16) * 16
    full = np.full((n, stride), np.nan if x.dtype.kind == "f" else 0x7A5A5A5A5A5A5A5A, x.dtype)
    full[:, col_begin : col_begin + w] = x
    return dev(full, cuda), col_begin


def centre_for(far, layout, g, col_begin, cuda):
    """The centre row an entry indexes by absolute column: on a far window it is read 4 GiB in."""
    if layout == "far_rows":
        return far.place(g)
    return far.far_row_vector(g, col_begin, fo.MARGIN + 64 * fo.MIB)


def compact_centre(g, col_begin, cuda):
    full = np.full(col_begin + g.size, np.nan, np.float32)
    full[col_begin:] = g
    return dev(full, cuda)


def values(rng, n, w, dtype=np.float32):
    if np.dtype(dtype).kind == "i":
        return rng.integers(-2 ** 62, 2 ** 62, (n, w), dtype=np.int64)
    return (rng.standard_normal((n, w)) * np.exp(rng.uniform(-3, 3, (n, w)))).astype(dtype)


def assert_clean(far):
    assert far.settle() == 0, "a kernel wrote outside its outputs"


# ---------------------------------------------------------------------------------------------
# the helper itself
# ---------------------------------------------------------------------------------------------


def test_the_arena_reports_stray_writes_and_wrapped_reads_are_finite(far, cuda):
    x = np.arange(10, dtype=np.float32).reshape(5, 2)
    stack, c0 = fo.far_rows(far, x)
    assert stack.data_ptr() == far.words.data_ptr() + fo.MARGIN and stack.stride(0) * 4 == fo.ROW_STRIDE
    assert host(stack[:, :2]).tobytes() == x.tobytes()
    for i in range(5):  # truncated and sign-extended row offsets hold finite decoys or another row
        for rel in fo.wrapped_offsets(i * fo.ROW_STRIDE, 0):
            v = host(far.typed(torch.float32)[(fo.MARGIN + rel) // 4 : (fo.MARGIN + rel) // 4 + 2])
            assert np.isfinite(v).all(), (i, rel)
    assert far.settle() == 0
    far.words[7 * fo.GIB // 4 + 5] = 0  # a stray write, nowhere near an operand
    assert far.settle() == 1
    far.words[7 * fo.GIB // 4 + 5] = fo.SENTINEL
    assert far.settle() == 0
    with pytest.raises(AssertionError, match="margin"):
        far.view(fo.MARGIN - 16, torch.float32, (4,))


# ---------------------------------------------------------------------------------------------
# reduce_stack (fp32): plain mean in the three modes, epilogues, FedDyn, split-N
# ---------------------------------------------------------------------------------------------

MODES = ((na.MODE_W32_DIV64, np.float32, np.float64), (na.MODE_W32_DIV32, np.float32, np.float32),
         (na.MODE_W64, np.float64, np.float64))


def _weights(rng, n, wdt, mode):
    w = rng.uniform(0.25, 3.0, n).astype(wdt)
    denom = float(np.sum(w.astype(np.float64)))
    return w, float(np.float32(denom)) if mode == na.MODE_W32_DIV32 else denom


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_reduce_mean(layout, width, far, cuda):
    n = 5 if layout == "far_rows" else 3
    rng = np.random.default_rng(width + n)
    x = values(rng, n, width)
    stack, c0 = lay_out(far, layout, x)
    small, s0 = compact(x, cuda)
    grid_for(width)
    for mode, wdt, rdt in MODES:
        w, denom = _weights(rng, n, wdt, mode)
        want = oracle.c_reduce(mode, x, w, denom)
        o32, o64 = far.out(torch.float32, width), far.out(torch.float64, width)
        ops.reduce_stack(stack, dev(w, cuda), mode, denom, col_begin=c0, n_cols=width, out32=o32, out64=o64)
        launched(PIECES_REDUCE if width > 4096 else SMALL_REDUCE)
        c32, c64 = torch.empty(width, device=cuda), torch.empty(width, dtype=torch.float64, device=cuda)
        ops.reduce_stack(small, dev(w, cuda), mode, denom, col_begin=s0, n_cols=width, out32=c32, out64=c64)
        with np.errstate(over="ignore", under="ignore"):
            assert fo.same_bits(host(o32), want.astype(np.float32)), (mode, "out32")
        assert fo.same_bits(host(o64), want.astype(np.float64)), (mode, "out64")
        assert host(o32).tobytes() == host(c32).tobytes() and host(o64).tobytes() == host(c64).tobytes(), mode
    assert_clean(far)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", ["avgm", "dyn"])
def test_reduce_epilogue_double_buffered(op, layout, far, cuda):
    """One optimizer epilogue with v_out, and FedDyn (h in place, theta to v_out): every per-column
    array sits in the arena."""
    n, width = (5 if layout == "far_rows" else 3), 1003
    rng = np.random.default_rng(17)
    x = values(rng, n, width)
    stack, c0 = lay_out(far, layout, x)
    mode, wdt, _ = MODES[0]
    w, denom = _weights(rng, n, wdt, mode)
    g = oracle.c_reduce(mode, x, w, denom)
    l32, v = rng.standard_normal(width).astype(np.float32), rng.standard_normal(width)
    l_d, v_d, v_out = far.place(l32), far.place(v), far.out(torch.float64, width)
    o32, o64 = far.out(torch.float32, width), far.out(torch.float64, width)
    v_want, l_want = v.copy(), l32.copy()
    if op == "dyn":
        ops.reduce_stack(stack, dev(w, cuda), mode, denom, col_begin=c0, n_cols=width, out32=o32, out64=o64,
                         op=na.OP_DYN, h=l_d, v=v_d, v_out=v_out, alpha=0.01)
        want = oracle.c_update_dyn(g, l_want, v_want, n)
    else:
        ops.reduce_stack(stack, dev(w, cuda), mode, denom, col_begin=c0, n_cols=width, out32=o32, out64=o64,
                         op=na.OP_AVGM, prev=l_d, v=v_d, v_out=v_out, beta=0.7)
        want = oracle.c_update("avgm", g, l32, v_want, beta=0.7)
    launched(SMALL_REDUCE)
    assert fo.same_bits(host(o64), want) and fo.same_bits(host(o32), want.astype(np.float32))
    assert fo.same_bits(host(v_out), v_want) and fo.same_bits(host(v_d), v) and fo.same_bits(host(l_d), l_want)
    # the same launch on a compact copy
    small, s0 = compact(x, cuda)
    cl, cv, cvo = dev(l32, cuda), dev(v, cuda), torch.empty(width, dtype=torch.float64, device=cuda)
    c64 = torch.empty(width, dtype=torch.float64, device=cuda)
    kw = dict(op=na.OP_DYN, h=cl, alpha=0.01) if op == "dyn" else dict(op=na.OP_AVGM, prev=cl, beta=0.7)
    ops.reduce_stack(small, dev(w, cuda), mode, denom, col_begin=s0, n_cols=width, out64=c64, v=cv, v_out=cvo, **kw)
    assert host(o64).tobytes() == host(c64).tobytes() and host(v_out).tobytes() == host(cvo).tobytes()
    assert host(l_d).tobytes() == host(cl).tobytes()
    assert_clean(far)


def test_reduce_reorder_far_rows(far, cuda):
    """reorder=True over 9 far rows reaches the split-N kernel; its order is the oracle's."""
    n, width = 9, 517
    rng = np.random.default_rng(9)
    x = values(rng, n, width)
    stack, c0 = fo.far_rows(far, x, stride_bytes=fo.ROW9_STRIDE)
    small, s0 = compact(x, cuda)
    mode, wdt, _ = MODES[0]
    w, denom = _weights(rng, n, wdt, mode)
    o64, c64 = far.out(torch.float64, width), torch.empty(width, dtype=torch.float64, device=cuda)
    ops.reduce_stack(stack, dev(w, cuda), mode, denom, col_begin=c0, n_cols=width, out64=o64, reorder=True)
    launched("reduce_kernel_splitn<")
    ops.reduce_stack(small, dev(w, cuda), mode, denom, col_begin=s0, n_cols=width, out64=c64, reorder=True)
    assert fo.same_bits(host(o64), oracle.c_reduce_splitn(mode, x, w, denom))
    assert host(o64).tobytes() == host(c64).tobytes()
    assert_clean(far)


def test_reduce_reorder_far_window(far, cuda):
    """reorder=True on a far window of 3 clients (too few to split: the launch is the ordered reduce)."""
    n, width = 3, 517
    rng = np.random.default_rng(10)
    x = values(rng, n, width)
    stack, c0 = fo.far_window(far, x)
    mode, wdt, _ = MODES[0]
    w, denom = _weights(rng, n, wdt, mode)
    o64 = far.out(torch.float64, width)
    ops.reduce_stack(stack, dev(w, cuda), mode, denom, col_begin=c0, n_cols=width, out64=o64, reorder=True)
    launched(SMALL_REDUCE)  # not the split-N kernel: the ordered sum, bit for bit
    assert fo.same_bits(host(o64), oracle.c_reduce(mode, x, w, denom))
    small, s0 = compact(x, cuda)
    c64 = torch.empty(width, dtype=torch.float64, device=cuda)
    ops.reduce_stack(small, dev(w, cuda), mode, denom, col_begin=s0, n_cols=width, out64=c64, reorder=True)
    assert host(o64).tobytes() == host(c64).tobytes()
    assert_clean(far)


# ---------------------------------------------------------------------------------------------
# the 8-byte and float16 reduces
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_reduce_8_byte(kind, layout, far, cuda):
    n = 5 if layout == "far_rows" else 3
    rng = np.random.default_rng(64)
    for width in WIDTHS[:2] + (10_001,):
        if kind == "f64":
            x, w = values(rng, n, width, np.float64), rng.uniform(0.25, 3.0, n)
        else:
            x, w = values(rng, n, width, np.int64), rng.integers(-5, 9, n, dtype=np.int64)
        denom = float(np.sum(w)) or 1.0
        stack, c0 = lay_out(far, layout, x)
        small, s0 = compact(x, cuda)
        o64, c64 = far.out(torch.float64, width), torch.empty(width, dtype=torch.float64, device=cuda)
        entry = ops.reduce_stack_f64 if kind == "f64" else ops.reduce_stack_i64
        entry(stack, dev(w, cuda), denom, o64, col_begin=c0, n_cols=width)
        launched("reduce_kernel_balanced<")
        entry(small, dev(w, cuda), denom, c64, col_begin=s0, n_cols=width)
        assert fo.same_bits(host(o64), oracle.c_reduce(kind, x, w, denom)), width
        assert host(o64).tobytes() == host(c64).tobytes()
        assert_clean(far)


H16 = ((na.MODE_H16_NUMPY, "out64"), (na.MODE_H16_W32, "out32"), (na.MODE_H16_NP16, "out16"))  # one per result dtype


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reduce_f16(layout, far, cuda):
    n = 5 if layout == "far_rows" else 3
    rng = np.random.default_rng(16)
    for width in WIDTHS:
        x = rng.standard_normal((n, width)).astype(np.float16)
        stack, c0 = lay_out(far, layout, x)
        small, s0 = compact(x, cuda)
        grid_for(width)
        for mode, _born in H16:
            w = (rng.integers(1, 9, n) / 4).astype(np.float32)  # exact in float16, and so is their sum
            denom = float(w.sum())
            outs = {"out16": far.out(torch.float16, width), "out32": far.out(torch.float32, width),
                    "out64": far.out(torch.float64, width)}
            ops.reduce_stack_f16(stack, dev(w, cuda), mode, denom, col_begin=c0, n_cols=width, **outs)
            launched("reduce_kernel_rows_h16<")
            couts = {k: torch.empty(width, dtype=v.dtype, device=cuda) for k, v in outs.items()}
            ops.reduce_stack_f16(small, dev(w, cuda), mode, denom, col_begin=s0, n_cols=width, **couts)
            want = dict(zip(("out64", "out32", "out16"), half_ref.outputs(half_ref.reduce_rows(mode, x, w, denom))))
            for k in outs:
                assert fo.same_bits(host(outs[k]), want[k]), (width, mode, k)
                assert host(outs[k]).tobytes() == host(couts[k]).tobytes(), (width, mode, k)
        assert_clean(far)


# ---------------------------------------------------------------------------------------------
# fold_stack (opening and carrying chunk) + fold_finish
# ---------------------------------------------------------------------------------------------

FOLDS = {na.ACC_F32: (np.float32, np.float32, na.MODE_W32_DIV64, oracle.MODE_W32_DIV64, "fold_kernel_rows<AccF32,"),
         na.ACC_F32_W64: (np.float32, np.float64, na.MODE_W64, oracle.MODE_W64, "fold_kernel_rows<AccF32W64,"),
         na.ACC_F64: (np.float64, np.float64, 0, "f64", "fold_kernel_elem<AccF64>"),
         na.ACC_I64: (np.int64, np.int64, 0, "i64", "fold_kernel_elem<AccI64>")}


def _fold_round(kind, stack, w_d, n, c0, width, acc_a, acc_b, split):
    """Rows [0, split) open the sum into acc_a, the rest carry it into acc_b; fold_finish divides."""
    _, _, mode, _, family = FOLDS[kind]
    ops.fold_stack(kind, stack, w_d, None, acc_a, col_begin=c0, n_cols=width, n_clients=split)
    launched(family)
    ops.fold_stack(kind, stack[split:], w_d[split:], acc_a, acc_b, col_begin=c0, n_cols=width, n_clients=n - split)
    launched(family)
    return mode


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", sorted(FOLDS))
def test_fold_and_finish(kind, layout, far, cuda):
    n = 5 if layout == "far_rows" else 3
    sdt, wdt, mode, omode, _ = FOLDS[kind]
    rng = np.random.default_rng(100 + kind)
    for width in WIDTHS[:2] + ((40_003,) if kind in (na.ACC_F32, na.ACC_F32_W64) else (10_001,)):
        x = values(rng, n, width, sdt)
        w = rng.integers(-5, 9, n, dtype=np.int64) if kind == na.ACC_I64 else rng.uniform(0.25, 3.0, n).astype(wdt)
        denom = float(np.sum(w.astype(np.float64))) or 1.0
        stack, c0 = lay_out(far, layout, x)
        small, s0 = compact(x, cuda)
        grid_for(width)
        adt = torch.from_numpy(np.empty(0, ACC_NP[kind])).dtype
        acc_a, acc_b, o64 = far.out(adt, width), far.out(adt, width), far.out(torch.float64, width)
        _fold_round(kind, stack, dev(w, cuda), n, c0, width, acc_a, acc_b, 2)
        ops.fold_finish(kind, mode, acc_b, denom, width, out64=o64)
        launched("fold_finish_kernel<")
        ca, cb = torch.empty(width, dtype=adt, device=cuda), torch.empty(width, dtype=adt, device=cuda)
        _fold_round(kind, small, dev(w, cuda), n, s0, width, ca, cb, 2)
        assert fo.same_bits(host(o64), oracle.c_reduce(omode, x, w, denom).astype(np.float64)), width
        assert host(acc_b).tobytes() == host(cb).tobytes() and host(acc_a).tobytes() == host(ca).tobytes(), width
        assert_clean(far)


# ---------------------------------------------------------------------------------------------
# trimmed sums
# ---------------------------------------------------------------------------------------------


def _trim(kind, stack, trim, c0, width, acc, wide=False):
    ops.trim_sum_stack(kind, stack, trim, acc, col_begin=c0, n_cols=width, wide=wide)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind,family", [(na.ACC_F32, "trim_kernel_rows<8,"), (na.ACC_F64, "trim_kernel_elem<double>"),
                                         (na.ACC_I64, "trim_kernel_elem<long>")], ids=["f32", "f64", "i64"])
def test_trim_sum(kind, family, layout, far, cuda):
    n = 5 if layout == "far_rows" else 3
    if layout == "far_window":
        family = family.replace("<8,", "<4,")
    rng = np.random.default_rng(3 + kind)
    for width in (1, 1003, 4099):
        x = values(rng, n, width, ACC_NP[kind])
        stack, c0 = lay_out(far, layout, x)
        small, s0 = compact(x, cuda)
        ops.set_reduce_grid(3 if width > 4000 else 0)  # 17 pieces of 256 columns on 3 blocks
        adt = stack.dtype
        acc, cacc = far.out(adt, width), torch.empty(width, dtype=adt, device=cuda)
        _trim(kind, stack, 1, c0, width, acc)
        launched(family)
        _trim(kind, small, 1, s0, width, cacc)
        assert rr.same_bits(host(acc), rr.trimmed_sum(x, 1)), width
        assert host(acc).tobytes() == host(cacc).tobytes()
        assert_clean(far)


@pytest.mark.parametrize("n,stride,np_", [(130, fo.WIDE_STRIDE_130, 256), (300, fo.WIDE_STRIDE_300, 512)])
def test_trim_sum_wide_far_rows(n, stride, np_, far, cuda):
    """129-1024 clients: the merge-sort kernel's runs of 128 rows begin gigabytes apart (n = 300: a
    wave holding two runs loads under two descriptors that are both far).  A far window of this many
    rows does not fit the arena (130 rows of 4 GiB): far rows only."""
    rng = np.random.default_rng(n)
    for width in (1, 1003):
        x = values(rng, n, width)
        stack, c0 = fo.far_rows(far, x, stride_bytes=stride)
        small, s0 = compact(x, cuda)
        ops.set_reduce_grid(3)  # 1003 columns are several pieces: three blocks sweep them
        for trim in (n // 10, (n - 1) // 2):
            acc, cacc = far.out(torch.float32, width), torch.empty(width, device=cuda)
            _trim(na.ACC_F32, stack, trim, c0, width, acc, wide=True)
            launched(f"merge_trim_kernel<{np_},")
            _trim(na.ACC_F32, small, trim, s0, width, cacc, wide=True)
            assert rr.same_bits(host(acc), rr.trimmed_sum(x, trim)), (width, trim)
            assert host(acc).tobytes() == host(cacc).tobytes()
        assert_clean(far)


# ---------------------------------------------------------------------------------------------
# Gram matrix, update norms: integer rows, the result is the integer answer
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("centred", [False, True], ids=["plain", "centred"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gram_and_rownorm(layout, centred, far, cuda):
    n = 5 if layout == "far_rows" else 3
    rng = np.random.default_rng(8)
    for width in WIDTHS:
        x = rng.integers(-8, 9, (n, width)).astype(np.float32)
        g = rng.integers(-8, 9, width).astype(np.float32) if centred else None
        stack, c0 = lay_out(far, layout, x)
        small, s0 = compact(x, cuda)
        c_far = centre_for(far, layout, g, c0, cuda) if centred else None
        c_small = compact_centre(g, s0, cuda) if centred else None
        grid_for(width)
        gram = ops.gram_stack(stack, center=c_far, col_begin=c0, n_cols=width, out=far.out(torch.float64, n * n))
        launched("gram_kernel_tile<32," + ("true" if centred else "false"))
        cgram = ops.gram_stack(small, center=c_small, col_begin=s0, n_cols=width)
        assert np.array_equal(host(gram), gr.gram(x, g)), width  # integers: exact in any order
        assert host(gram).tobytes() == host(cgram).tobytes()
        norm = ops.rownorm2_stack(stack, center=c_far, col_begin=c0, n_cols=width, out=far.out(torch.float64, n))
        launched("rownorm_kernel<")
        cnorm = ops.rownorm2_stack(small, center=c_small, col_begin=s0, n_cols=width)
        assert np.array_equal(host(norm), cr.norm2(x, g)), width
        assert host(norm).tobytes() == host(cnorm).tobytes()
        assert_clean(far)


# ---------------------------------------------------------------------------------------------
# clipped sums
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("layout", LAYOUTS)
def test_clip_sum_and_clip_fold(layout, far, cuda):
    n = 5 if layout == "far_rows" else 3
    rng = np.random.default_rng(21)
    scale = np.array([1.0, 0.375, 0.0, 2.0, 0.8125][:n], np.float32)  # as it is, shrunk, the centre, ...
    for width in WIDTHS:
        x, g = values(rng, n, width), rng.standard_normal(width).astype(np.float32)
        stack, c0 = lay_out(far, layout, x)
        small, s0 = compact(x, cuda)
        c_far, c_small = centre_for(far, layout, g, c0, cuda), compact_centre(g, s0, cuda)
        s_d = dev(scale, cuda)
        grid_for(width)
        acc, cacc = far.out(torch.float32, width), torch.empty(width, device=cuda)
        ops.clip_sum_stack(stack, c_far, s_d, acc, col_begin=c0, n_cols=width)
        launched("clip_sum_kernel<")
        ops.clip_sum_stack(small, c_small, s_d, cacc, col_begin=s0, n_cols=width)
        assert fo.same_bits(host(acc), cr.clipped_sum(x, g, scale)), width
        assert host(acc).tobytes() == host(cacc).tobytes()
        # opening chunk (rows 0, 1), then the carrying chunk into another accumulator
        a, b = far.out(torch.float32, width), far.out(torch.float32, width)
        ops.clip_fold_stack(stack, c_far, s_d, None, a, col_begin=c0, n_cols=width, n_clients=2)
        ops.clip_fold_stack(stack[2:], c_far, s_d[2:], a, b, col_begin=c0, n_cols=width, n_clients=n - 2)
        launched("clip_fold_kernel<")
        assert fo.same_bits(host(b), cfr.fold_chain(x, g, scale, (2,))), width
        assert fo.same_bits(host(a), cfr.fold_chain(x[:2], g, scale[:2], ())), width
        ca, cb = torch.empty(width, device=cuda), torch.empty(width, device=cuda)
        ops.clip_fold_stack(small, c_small, s_d, None, ca, col_begin=s0, n_cols=width, n_clients=2)
        ops.clip_fold_stack(small[2:], c_small, s_d[2:], ca, cb, col_begin=s0, n_cols=width, n_clients=n - 2)
        assert host(a).tobytes() == host(ca).tobytes() and host(b).tobytes() == host(cb).tobytes(), width
        assert_clean(far)


# ---------------------------------------------------------------------------------------------
# int8 and int4 dequantize-and-sum
# ---------------------------------------------------------------------------------------------


def _far_scales(far, sc, first_block):
    """Per-block scales [n, first_block + blocks] whose rows lie ROW_STRIDE apart, read first_block in."""
    return far.stack(sc, fo.ROW_STRIDE, first_block, fo.MARGIN + fo.GIB)


@pytest.mark.parametrize("centred", [False, True], ids=["plain", "centred"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_deq_fold_q8(layout, centred, far, cuda):
    """Far rows of codes and of scales; far windows on a scale-block boundary (col_begin a multiple of
    1024 is all the entry takes: one off it is refused).  The centre is indexed by absolute column: under
    a window 2^32 codes in it would be 16 GiB long, more than the arena holds between its margins, so the
    centred far window begins 2^30 codes in, where the centre is read 4 GiB from its pointer."""
    n = 5 if layout == "far_rows" else 3
    rng = np.random.default_rng(88)
    for width, extra in ((1, 0), (1003, 3 * 1024), (40_003, 1024)):
        codes = rng.integers(-127, 128, (n, width), dtype=np.int8)
        blocks = -(-width // qr.BLOCK)
        sc = np.exp(rng.uniform(-4, 2, (n, blocks))).astype(np.float32)
        w = rng.uniform(0.25, 3.0, n).astype(np.float32)
        g = rng.standard_normal(width).astype(np.float32) if centred else None
        if layout == "far_rows":
            stack, c0 = fo.far_rows(far, codes)
        else:
            stack, c0 = fo.far_window(far, codes, extra_cols=extra, window_bytes=fo.GIB if centred else fo.WINDOW_BYTES)
        sc_far = _far_scales(far, sc, c0 // qr.BLOCK)
        c_far = centre_for(far, layout, g, c0, cuda) if centred else None
        w_d = dev(w, cuda)
        grid_for(width)
        a, b = far.out(torch.float32, width), far.out(torch.float32, width)
        ops.deq_fold_stack(stack, sc_far, w_d, None, a, center=c_far, col_begin=c0, n_cols=width, n_clients=2)
        launched("deq_fold_kernel<")
        ops.deq_fold_stack(stack[2:], sc_far[2:], w_d[2:], a, b, center=c_far, col_begin=c0, n_cols=width)
        launched("deq_fold_kernel<")
        want_a = qr.deq_fold(None, codes[:2], sc[:2], w[:2], g)
        assert qr.same_bits(host(a), want_a) and qr.same_bits(host(b), qr.deq_fold(want_a, codes[2:], sc[2:], w[2:], g)), width
        small = dev(np.pad(codes, ((0, 0), (0, -width % 16 + 16))), cuda)
        ca, cb = torch.empty(width, device=cuda), torch.empty(width, device=cuda)
        cg = dev(g, cuda) if centred else None
        ops.deq_fold_stack(small, dev(sc, cuda), w_d, None, ca, center=cg, n_cols=width, n_clients=2)
        ops.deq_fold_stack(small[2:], dev(sc[2:], cuda), w_d[2:], ca, cb, center=cg, n_cols=width)
        assert host(a).tobytes() == host(ca).tobytes() and host(b).tobytes() == host(cb).tobytes(), width
        if layout == "far_window" and width == 1003 and not centred:
            with pytest.raises(na.NativeError, match="1024"):
                ops.deq_fold_stack(stack, sc_far, w_d, None, a, col_begin=c0 + 512, n_cols=8)
        assert_clean(far)


@pytest.mark.parametrize("centred", [False, True], ids=["plain", "centred"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_deq_fold_q4(layout, centred, far, cuda):
    """Two codes per byte: the far window begins 2^33 codes in, on a scale block and (extra) off the
    1024-column boundary of the int8 kernel but on this entry's 2048-column chunk; off it is refused.  As
    for int8 the centred far window begins 2^30 codes in: the centre is then read 4 GiB from its pointer."""
    n = 5 if layout == "far_rows" else 3
    rng = np.random.default_rng(44)
    for width, extra in ((1, 0), (1003, 3 * 2048), (40_003, 2048)):
        nbytes = -(-width // 2)
        packed = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
        blocks = -(-width // q4r.BLOCK)
        sc = np.exp(rng.uniform(-4, 2, (n, blocks))).astype(np.float32)
        w = rng.uniform(0.25, 3.0, n).astype(np.float32)
        g = rng.standard_normal(width).astype(np.float32) if centred else None
        if layout == "far_rows":
            stack, c0 = fo.far_rows(far, packed)
        else:
            stack, b0 = fo.far_window(far, packed, extra_cols=extra // 2,
                                      window_bytes=fo.GIB // 2 if centred else fo.WINDOW_BYTES)
            c0 = 2 * b0
            assert c0 >= 1 << (30 if centred else 33)
        sc_far = _far_scales(far, sc, c0 // q4r.BLOCK)
        c_far = centre_for(far, layout, g, c0, cuda) if centred else None
        w_d = dev(w, cuda)
        grid_for(width)
        a, b = far.out(torch.float32, width), far.out(torch.float32, width)
        ops.deq_fold_q4_stack(stack, sc_far, w_d, None, a, center=c_far, col_begin=c0, n_cols=width, n_clients=2)
        launched("deq_fold4_kernel<")
        ops.deq_fold_q4_stack(stack[2:], sc_far[2:], w_d[2:], a, b, center=c_far, col_begin=c0, n_cols=width)
        launched("deq_fold4_kernel<")
        want_a = q4r.deq_fold4(None, packed[:2], sc[:2], w[:2], width, g)
        want_b = q4r.deq_fold4(want_a, packed[2:], sc[2:], w[2:], width, g)
        assert q4r.same_bits(host(a), want_a) and q4r.same_bits(host(b), want_b), width
        small = dev(np.pad(packed, ((0, 0), (0, -nbytes % 16 + 16))), cuda)
        ca, cb = torch.empty(width, device=cuda), torch.empty(width, device=cuda)
        cg = dev(g, cuda) if centred else None
        ops.deq_fold_q4_stack(small, dev(sc, cuda), w_d, None, ca, center=cg, n_cols=width, n_clients=2)
        ops.deq_fold_q4_stack(small[2:], dev(sc[2:], cuda), w_d[2:], ca, cb, center=cg, n_cols=width)
        assert host(a).tobytes() == host(ca).tobytes() and host(b).tobytes() == host(cb).tobytes(), width
        if layout == "far_window" and width == 40_003 and not centred:
            with pytest.raises(na.NativeError, match="2048"):
                ops.deq_fold_q4_stack(stack, sc_far, w_d, None, a, col_begin=c0 + 1024, n_cols=8)
        assert_clean(far)


# ---------------------------------------------------------------------------------------------
# long windows: window-relative offsets pass 4 GiB inside one launch
# ---------------------------------------------------------------------------------------------
# Small integers, power-of-two weights and denominator: every rule is exact in any order, with or
# without fused multiply-add, so a chunked torch expression on the device is the whole-width
# reference; slices at the head, at both sides of byte offsets 2^31 and 2^32 of each operand and at
# the ragged tail are also checked against the numpy restatements on the host.

LONG = fo.LONG_COLS
CHUNK = 1 << 24
# (multiplier, modulus) of the operands' patterns.  The moduli are odd, so column c and column
# c - 2^30 - where a byte offset truncated to 32 bits would read - hold different values in every
# operand and in everything computed from them.
PA, PB, PC = (7, 61), (13, 31), (5, 13)
W2 = np.array([2.0, 4.0], np.float32)  # the two clients' weights; the denominator is 8
MODE32 = na.MODE_W32_DIV32  # fp32 state and results: four 4 GiB operands at the most


def pattern(c0, c1, pat, device=None):
    """The small-integer test pattern of columns [c0, c1): ((c * mul) % mod) - mod // 2, as int64."""
    mul, mod = pat
    if device is None:
        c = np.arange(c0, c1, dtype=np.int64)
    else:
        c = torch.arange(c0, c1, dtype=torch.int64, device=device)
    return (c * mul) % mod - mod // 2


def test_the_patterns_tell_a_column_from_the_one_a_wrapped_offset_reads():
    c = np.arange((1 << 30) - 5000, LONG, dtype=np.int64)
    for pat in (PA, PB, PC):
        mul, mod = pat
        assert ((c * mul) % mod != ((c - (1 << 30)) * mul) % mod).all()
        assert ((c * mul) % mod != ((c - (1 << 29)) * mul) % mod).all()


def fill_long(t, expr):
    """t[c] = expr(c0, c1)[c - c0], written in chunks (t a 1-D arena view of LONG elements)."""
    for c0 in range(0, t.numel(), CHUNK):
        c1 = min(t.numel(), c0 + CHUNK)
        t[c0:c1] = expr(c0, c1).to(t.dtype)


def pat_on(pat, device):
    return lambda c0, c1: pattern(c0, c1, pat, device)


def probe_slices(item):
    """Column ranges at the head, at both sides of byte offsets 2^31 and 2^32, and at the ragged tail."""
    out = [(0, 600), (LONG - 600, LONG)]
    for byte in (1 << 31, 1 << 32):
        c = byte // item
        if c + 300 <= LONG:
            out.append((c - 300, c + 300))
    return out


def long_rows(far, n, dtype=torch.float32, first=fo.MARGIN):
    """n rows of LONG columns, one after the other from arena offset `first`; returns (stack, end offset)."""
    item = torch.empty(0, dtype=dtype).element_size()
    stride = -(-LONG // 16) * 16
    t = far.view(first, dtype, (n, LONG), (stride, 1))
    far.mark(first, n * stride * item)
    return t, first + n * stride * item


def long_vector(far, dtype, first):
    item = torch.empty(0, dtype=dtype).element_size()
    nbytes = -(-LONG * item // 256) * 256
    far.mark(first, nbytes)
    return far.view(first, dtype, (LONG,)), first + nbytes


def assert_long_equals(t, expr, what):
    """t == expr(c0, c1) over the whole width, compared on the device in chunks."""
    bad = torch.zeros((), dtype=torch.int64, device=t.device)
    for c0 in range(0, LONG, CHUNK):
        c1 = min(LONG, c0 + CHUNK)
        bad += (t[c0:c1] != expr(c0, c1).to(t.dtype)).sum()
    assert int(bad) == 0, f"{what}: {int(bad)} columns differ from the device expression"


def long_stack(far, cuda):
    """The two-client stack of patterns PA and PB, and the first free arena offset."""
    x, end = long_rows(far, 2)
    fill_long(x[0], pat_on(PA, cuda))
    fill_long(x[1], pat_on(PB, cuda))
    return x, end


def rows_np(c0, c1):
    return np.stack([pattern(c0, c1, PA), pattern(c0, c1, PB)]).astype(np.float32)


def wsum(c0, c1, device):  # 2 a + 4 b: integers below 2^8
    return (2 * pattern(c0, c1, PA, device) + 4 * pattern(c0, c1, PB, device)).to(torch.float64)


GRIDS = pytest.mark.parametrize("grid", [0, 5], ids=["default", "forced5"])  # forced small: a block's piece loop runs long


@GRIDS
def test_long_window_reduce_mean(grid, far, cuda):
    x, end = long_stack(far, cuda)
    out, end = long_vector(far, torch.float32, end)
    ops.set_reduce_grid(grid)
    ops.reduce_stack(x, dev(W2, cuda), MODE32, 8.0, out32=out)
    launched(LONG_REDUCE)
    assert_long_equals(out, lambda c0, c1: wsum(c0, c1, cuda) / 8, "reduce_stack mean")
    for c0, c1 in probe_slices(4):
        assert fo.same_bits(host(out[c0:c1]), oracle.c_reduce(MODE32, rows_np(c0, c1), W2, 8.0)), (c0, c1)
    assert_clean(far)


@GRIDS
def test_long_window_fold(grid, far, cuda):
    """Row 0 opens the sum, row 1 carries it (acc_out is acc_in, as fold_stack allows)."""
    x, end = long_stack(far, cuda)
    acc, end = long_vector(far, torch.float32, end)
    w_d = dev(W2, cuda)
    ops.set_reduce_grid(grid)
    ops.fold_stack(na.ACC_F32, x, w_d, None, acc, n_clients=1)
    launched("fold_kernel_rows<AccF32,")
    assert_long_equals(acc, lambda c0, c1: 2 * pattern(c0, c1, PA, cuda), "opening fold")
    ops.fold_stack(na.ACC_F32, x[1:], w_d[1:], acc, acc, n_clients=1)
    launched("fold_kernel_rows<AccF32,")
    assert_long_equals(acc, lambda c0, c1: wsum(c0, c1, cuda), "carrying fold")
    for c0, c1 in probe_slices(4):
        want = oracle.c_reduce(oracle.MODE_W32_DIV32, rows_np(c0, c1), W2, 1.0)
        assert fo.same_bits(host(acc[c0:c1]), want), (c0, c1)
    assert_clean(far)


def test_long_window_fold_finish(far, cuda):
    acc, end = long_vector(far, torch.float32, fo.MARGIN)
    out, end = long_vector(far, torch.float32, end)
    fill_long(acc, lambda c0, c1: wsum(c0, c1, cuda))
    ops.fold_finish(na.ACC_F32, MODE32, acc, 8.0, LONG, out32=out)
    launched("fold_finish_kernel<float,float,0>")
    assert_long_equals(out, lambda c0, c1: wsum(c0, c1, cuda) / 8, "fold_finish mean")
    assert_long_equals(acc, lambda c0, c1: wsum(c0, c1, cuda), "the accumulator (read only)")
    for c0, c1 in probe_slices(4):
        assert fo.same_bits(host(out[c0:c1]), oracle.c_reduce(MODE32, rows_np(c0, c1), W2, 8.0)), (c0, c1)
    assert_clean(far)


@GRIDS
def test_long_window_reduce_epilogue(grid, far, cuda):
    """The momentum epilogue, beta = 0.5: v' = (mean - prev) + v / 2, w = prev + v', multiples of 1/4.
    prev is its own operand (pattern PC).  Two rows, prev, v and out32 are five 4 GiB operands; between
    the arena's margins, under its 24 GiB cap, three fit.  So out32 is prev (the in-place form of a fused
    step) and v is row 0 of the stack, updated in place: the launch reads a column of every row before
    it writes that column's state.  A kernel that stops doing so needs this test on a larger arena."""
    x, end = long_stack(far, cuda)
    prev, end = long_vector(far, torch.float32, end)
    fill_long(prev, pat_on(PC, cuda))
    ops.set_reduce_grid(grid)

    def v_new(c0, c1):
        return (wsum(c0, c1, cuda) / 8 - pattern(c0, c1, PC, cuda)) + pattern(c0, c1, PA, cuda).to(torch.float64) / 2

    slices, want = probe_slices(4), []
    for c0, c1 in slices:
        r, v_np, p_np = rows_np(c0, c1), pattern(c0, c1, PA).astype(np.float32), pattern(c0, c1, PC).astype(np.float32)
        want.append((oracle.c_update("avgm", oracle.c_reduce(MODE32, r, W2, 8.0), p_np, v_np, beta=0.5), v_np))
    # out32 = prev: the in-place form of a fused step (reduce_stack's docstring)
    ops.reduce_stack(x, dev(W2, cuda), MODE32, 8.0, out32=prev, op=na.OP_AVGM, prev=prev, v=x[0], beta=0.5)
    launched(LONG_REDUCE)
    assert_long_equals(x[0], v_new, "epilogue v")
    assert_long_equals(prev, lambda c0, c1: pattern(c0, c1, PC, cuda) + v_new(c0, c1), "epilogue w")
    assert_long_equals(x[1], pat_on(PB, cuda), "row 1 (read only)")
    for (c0, c1), (w_want, v_want) in zip(slices, want):
        assert fo.same_bits(host(prev[c0:c1]), w_want) and fo.same_bits(host(x[0][c0:c1]), v_want), (c0, c1)
    assert_clean(far)


def test_long_window_apply_update(far, cuda):
    """The standalone momentum update (apply_kernel records no launch): v' = (glob - local) + v / 2,
    w = local + v' into its own operand."""
    local, end = long_vector(far, torch.float32, fo.MARGIN)
    glob, end = long_vector(far, torch.float32, end)
    v, end = long_vector(far, torch.float32, end)
    fill_long(local, pat_on(PA, cuda))
    fill_long(glob, pat_on(PB, cuda))
    fill_long(v, pat_on(PC, cuda))

    def v_new(c0, c1):
        return (pattern(c0, c1, PB, cuda) - pattern(c0, c1, PA, cuda)) + pattern(c0, c1, PC, cuda).to(torch.float64) / 2

    slices, want = probe_slices(4), []
    for c0, c1 in slices:
        v_np = pattern(c0, c1, PC).astype(np.float32)
        want.append((oracle.c_update("avgm", pattern(c0, c1, PB).astype(np.float32), pattern(c0, c1, PA).astype(np.float32),
                                     v_np, beta=0.5), v_np))
    ops.apply_update(na.OP_AVGM, local, glob, v, out32=glob, beta=0.5)  # w over glob, as apply_dyn documents
    assert_long_equals(v, v_new, "apply_update v")
    assert_long_equals(glob, lambda c0, c1: pattern(c0, c1, PA, cuda) + v_new(c0, c1), "apply_update w")
    assert_long_equals(local, pat_on(PA, cuda), "local (read only)")
    for (c0, c1), (w_want, v_want) in zip(slices, want):
        assert fo.same_bits(host(glob[c0:c1]), w_want) and fo.same_bits(host(v[c0:c1]), v_want), (c0, c1)
    assert_clean(far)


def test_long_window_apply_dyn_and_gauss_add(far, cuda):
    """apply_dyn and gauss_add over 2^30 + 1003 columns.  The noise of a column depends on its absolute
    index only, so a slice equals the same entry run on a small window at that col_begin."""
    glob, end = long_vector(far, torch.float32, fo.MARGIN)
    h, end = long_vector(far, torch.float32, end)
    theta, end = long_vector(far, torch.float32, end)
    for t, pat in ((glob, PA), (h, PB), (theta, PC)):
        fill_long(t, pat_on(pat, cuda))
    slices = probe_slices(4)
    want = []
    for c0, c1 in slices:  # FedDyn with alpha = 0.5, N = 4: the oracle on the slices
        g_np, h_np, t_np = (pattern(c0, c1, pat).astype(np.float32) for pat in (PA, PB, PC))
        want.append((oracle.c_update_dyn(g_np, h_np, t_np, 4, alpha=0.5), h_np, t_np))
    ops.apply_dyn(glob, h, theta, 4, 0.5, out32=glob)  # apply_kernel records no launch
    for (c0, c1), (w_np, h_np, t_np) in zip(slices, want):
        assert fo.same_bits(host(glob[c0:c1]), w_np) and fo.same_bits(host(h[c0:c1]), h_np), (c0, c1)
        assert fo.same_bits(host(theta[c0:c1]), t_np), (c0, c1)
    # the same step on a compact copy of a window that straddles byte 2^32 of every operand
    c0, c1 = (1 << 30) - 4096, LONG
    cg, ch, ct = (pattern(c0, c1, pat, cuda).to(torch.float32) for pat in (PA, PB, PC))
    ops.apply_dyn(cg, ch, ct, 4, 0.5, out32=cg)
    assert torch.equal(glob[c0:c1], cg) and torch.equal(h[c0:c1], ch) and torch.equal(theta[c0:c1], ct)

    for grid in (0, 5):
        fill_long(glob, pat_on(PA, cuda))
        ops.set_reduce_grid(grid)
        ops.gauss_add(glob, 0.5, 11, 3, col_begin=4096)
        assert ops.last_launch()[0] == "gauss_add_kernel"
        for s0, s1 in slices + [(c0, c1)]:
            a0 = s0 & ~3
            small = pattern(a0, s1, PA, cuda).to(torch.float32)
            ops.gauss_add(small, 0.5, 11, 3, col_begin=4096 + a0)
            assert torch.equal(glob[a0:s1], small), (grid, s0, s1)
            assert not torch.equal(small, pattern(a0, s1, PA, cuda).to(torch.float32))  # noise was added
    assert_clean(far)


# ---------------------------------------------------------------------------------------------
# fill_uniform and fa_copy over a range that crosses 4 GiB
# ---------------------------------------------------------------------------------------------


def test_fill_uniform_and_copy_cross_4_gib(far, cuda):
    dst, end = long_vector(far, torch.float32, fo.MARGIN)
    ops.fill_uniform(dst, 77, row_begin=3, col_begin=64)
    for c0, c1 in probe_slices(4):
        assert host(dst[c0:c1]).tobytes() == oracle.fill_uniform(1, c1 - c0, 77, row0=3, col0=64 + c0).tobytes(), (c0, c1)
    copy, end = long_vector(far, torch.float32, end)
    nbytes = LONG * 4 - 4  # ends in a partial 16-byte quad
    L = na.lib()
    na.check(L.fa_copy(copy.data_ptr(), dst.data_ptr(), nbytes, na.stream_handle(cuda)), "fa_copy")
    bad = torch.zeros((), dtype=torch.int64, device=cuda)
    a, b = dst.view(torch.int32), copy.view(torch.int32)
    for c0 in range(0, LONG - 1, CHUNK):
        c1 = min(LONG - 1, c0 + CHUNK)
        bad += (a[c0:c1] != b[c0:c1]).sum()
    assert int(bad) == 0
    assert int(b[LONG - 1]) == fo.SENTINEL  # nothing past the end
    assert_clean(far)


# ---------------------------------------------------------------------------------------------
# device uploads read in place through a row table
# ---------------------------------------------------------------------------------------------


def test_row_table_of_far_unequal_rows(far, cuda):
    """Uploads that are views at far, unequal distances in the arena: the engine reads them through
    reduce_stack on a RowTable (fa_reduce_f32_rows), bit-exact with the oracle."""
    from flearn_amd import AVG

    n, numel = 5, 70_003
    rng = np.random.default_rng(55)
    x = values(rng, n, numel)
    offs = [0, 2 * fo.GIB + 4096, 4 * fo.GIB + 64 * fo.MIB, 7 * fo.GIB + 256, 11 * fo.GIB + 1024]
    clients = []
    for i in range(n):
        for rel in fo.wraps(offs[i]) - {offs[0]}:
            far.decoy(fo.MARGIN + rel, 4096, np.float32)
    for i in range(n):
        far.write(fo.MARGIN + offs[i], x[i])
        clients.append({"w": far.view(fo.MARGIN + offs[i], torch.float32, (numel,))})
    weights = [1.0 + 0.25 * i for i in range(n)]
    s = AVG()
    got = s.server([{"agg_weight": w, "params": c} for w, c in zip(weights, clients)], 0)["w_glob"]
    assert s.engine.packer.last_row_tables.get("f32") == "rows", s.engine.packer.last_row_tables
    launched("reduce_kernel_segrows_rm<")
    want = oracle.server_ensemble(weights, [{"w": x[i]} for i in range(n)])
    g = got["w"]
    g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    assert g.dtype == np.asarray(want["w"]).dtype and g.tobytes() == np.asarray(want["w"]).tobytes()
    assert_clean(far)
