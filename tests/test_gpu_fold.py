"""GPU: fa_fold / fa_fold_finish (a round aggregated in chunks of clients) against the C oracle.

The expected value is always oracle.c_reduce(mode, the WHOLE stack, the WHOLE weight list, denom) —
the reference's arithmetic on the undivided list (strategy.py:123-129) — so chunking must be
invisible: results are bit-identical, NaN exactly where the oracle has NaN.  Epilogues are
oracle.c_update / c_update_dyn on that mean, as tests/test_gpu_epilogue_values.py checks the fused
families.  Every output and accumulator is followed by 96 sentinel elements that must survive.
Every launch's full name comes from the table of tests/instantiation_cases.py, which
tests/test_kernel_inventory.py holds equal to the built library: the fold kernel of the kind, and
the one fold_finish_kernel<A,T,OP> of the (kind, mode, op) — all 19 are reached here (mean and the
five epilogues in the three fp32 modes, the mean of the two 8-byte kinds)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import oracle
from epilogue_table import HYPERS, first_diffs, same_values, stack_for, table
from flearn_amd import _native as na
from flearn_amd import aggregator as agg
from instantiation_cases import FOLD_ELEM, FOLD_ROWS_POLICY, FOLD_TARGETS, FOLD_V, fold_finish_name, fold_rows_name

pytestmark = pytest.mark.gpu

TAIL = 96
SENT = {torch.float32: 0x7FA5A5A5, torch.float64: 0x7FF5A5A5A5A5A5A5, torch.int64: 0x7FF5A5A5A5A5A5A5}
INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64}
NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64}

# acc kind -> (stack dtype, weight dtype, accumulator dtype)
KINDS = {
    na.ACC_F32: (torch.float32, torch.float32, torch.float32),
    na.ACC_F32_W64: (torch.float32, torch.float64, torch.float64),
    na.ACC_F64: (torch.float64, torch.float64, torch.float64),
    na.ACC_I64: (torch.int64, torch.int64, torch.int64),
}
# (acc kind, finish mode, oracle mode)
FP32_MODES = [(na.ACC_F32, na.MODE_W32_DIV64, oracle.MODE_W32_DIV64), (na.ACC_F32, na.MODE_W32_DIV32, oracle.MODE_W32_DIV32),
              (na.ACC_F32_W64, na.MODE_W64, oracle.MODE_W64)]
WIDE_MODES = [(na.ACC_F64, 0, "f64"), (na.ACC_I64, 0, "i64")]
MODE_IDS = {0: "div64", 1: "div32", 2: "w64", "f64": "f64", "i64": "i64"}


class Arr:
    """A device array of n values followed by TAIL sentinel elements; filled with the sentinel when
    no host values are given (an unwritten column would show)."""

    def __init__(self, n, dtype, cuda, host=None):
        self.n, self.dtype = n, dtype
        self.bits = torch.full((n + TAIL,), SENT[dtype], dtype=INT_OF[dtype], device=cuda)
        self.t = self.bits.view(dtype)
        if host is not None:
            self.t[:n] = torch.from_numpy(np.ascontiguousarray(host, NP_OF[dtype])).to(cuda)

    def got(self):
        return self.t[: self.n].cpu().numpy()

    def tail_intact(self):
        return bool((self.bits[self.n :] == SENT[self.dtype]).all())

    def untouched(self):
        return bool((self.bits == SENT[self.dtype]).all())


def _stack(host, col_begin, cuda):
    """[n, stride] device stack; outside the window [col_begin, +ncols): NaN (int64: a large value)."""
    n, ncols = host.shape
    stride = -(-(col_begin + ncols + TAIL) // 64) * 64
    dt = torch.from_numpy(host[:0]).dtype
    fill = float("nan") if dt.is_floating_point else 0x7A5A5A5A5A5A5A5A
    x = torch.full((n, stride), fill, dtype=dt, device=cuda)
    x[:, col_begin : col_begin + ncols] = torch.from_numpy(host).to(cuda)
    return x


def _check(name, got, want):
    assert same_values(got, want), (name,) + first_diffs(got, want)


def _stream(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


def fold_chain(cuda, kind, x, w, splits, col_begin, ncols, *, double=False):
    """Folds the rows of device stack x in chunks of `splits` clients; returns (final accumulator Arr,
    the other Arr or None, kernel names launched)."""
    L = na.lib()
    sdt, wdt, adt = KINDS[kind]
    accs = [Arr(ncols, adt, cuda), Arr(ncols, adt, cuda) if double else None]
    shipped = {fold_rows_name(kind, v) for v in FOLD_V} if kind in FOLD_ROWS_POLICY else {FOLD_ELEM[kind]}
    cur, i0, names = None, 0, []
    for j, k in enumerate(splits):
        out = accs[j % 2] if double else accs[0]
        rc = L.fa_fold(kind, x[i0].data_ptr(), x.stride(0), k, w[i0:].data_ptr(), None if cur is None else cur.t.data_ptr(),
                       out.t.data_ptr(), col_begin, ncols, _stream(cuda))
        na.check(rc, "fa_fold")
        kernel, grid, launches = agg.last_launch()
        assert (kernel is None) == (ncols == 0)
        if kernel is not None:
            assert kernel in shipped and launches == 1 and grid >= 1, kernel
            names.append(kernel)
        cur, i0 = out, i0 + k
    assert i0 == x.shape[0]
    return cur, names


def finish(cuda, kind, mode, acc, denom, ncols, *, epi=None, want32=True, want64=True):
    L = na.lib()
    out32 = Arr(ncols, torch.float32, cuda) if want32 else None
    out64 = Arr(ncols, torch.float64, cuda) if want64 else None
    rc = L.fa_fold_finish(kind, mode, acc.t.data_ptr(), float(denom), ncols, ctypes.byref(epi) if epi is not None else None,
                          out32.t.data_ptr() if out32 else None, out64.t.data_ptr() if out64 else None, _stream(cuda))
    na.check(rc, "fa_fold_finish")
    kernel, _, launches = agg.last_launch()
    if ncols:
        op = epi.op if epi is not None else na.OP_MEAN
        assert kernel == fold_finish_name(kind, mode, op) and launches == 1, kernel
    return out32, out64


def run_round(cuda, kind, mode, omode, xh, wh, denom, splits, *, col_begin=0, double=False):
    """One streamed round through the C ABI, checked against the oracle on the whole list.  Returns
    the final accumulator's bits and the names of the fold kernels."""
    n, ncols = xh.shape
    sdt, wdt, adt = KINDS[kind]
    x = _stack(xh, col_begin, cuda)
    w = torch.from_numpy(np.ascontiguousarray(wh, NP_OF[wdt])).to(cuda)
    acc, names = fold_chain(cuda, kind, x, w, splits, col_begin, ncols, double=double)
    f32res = omode == oracle.MODE_W32_DIV32
    out32, out64 = finish(cuda, kind, mode, acc, denom, ncols)
    torch.cuda.synchronize()
    want = oracle.c_reduce(omode, xh, wh, denom)
    with np.errstate(over="ignore", under="ignore"):
        _check("out32", out32.got(), want.astype(np.float32))
        _check("out64", out64.got(), want.astype(np.float64) if f32res else want)
    assert acc.tail_intact() and out32.tail_intact() and out64.tail_intact(), "written past the end"
    return acc.got().tobytes(), names


def depth_of(name):
    """D of fold_kernel_rows<P,V,D,W,NT>; 1 for the element-wise kernel of the 8-byte kinds."""
    m = re.fullmatch(r"fold_kernel_rows<\w+,(\d+),(\d+),(\d+),true>", name)
    if m is None:
        assert name.startswith("fold_kernel_elem<"), name
        return 1
    v, d, w = map(int, m.groups())
    assert v * d * w == 64
    return d


def chunkings(n, d):
    """All-ones, K in {2, D-1, D, D+1, 2D, 2D+1} (the last chunk takes the remainder), one uneven."""
    out = [(1,) * n]
    for k in (2, d - 1, d, d + 1, 2 * d, 2 * d + 1):
        if k >= 1:
            out.append(tuple([k] * (n // k) + ([n % k] if n % k else [])))
    if n >= 3:
        out.append((1, n - 2, 1))
    out.append((n,))
    return sorted(set(out))


def _values(kind, rng, n, ncols):
    if kind == na.ACC_I64:
        x = rng.integers(-2 ** 62, 2 ** 62, (n, ncols), dtype=np.int64)  # the products and the sum wrap
        w = rng.integers(-5, 9, n, dtype=np.int64)
        return x, w, float(np.sum(w)) or 1.0
    x = (rng.standard_normal((n, ncols)) * np.exp(rng.uniform(-6, 6, (n, ncols))))
    x = x.astype(np.float64 if kind == na.ACC_F64 else np.float32)
    w = rng.uniform(0.25, 3.0, n)
    if kind == na.ACC_F32:
        w = w.astype(np.float32)
        return x, w, float(np.sum(w.astype(np.float64)))
    return x, w, float(np.sum(w))


@pytest.fixture
def grid():
    prev = []

    def set_grid(g):
        prev.append(agg.set_reduce_grid(g))

    yield set_grid
    if prev:
        agg.set_reduce_grid(prev[0])


def _probe_depth(cuda, kind, ncols):
    """The pipeline depth of the kernel this width selects, from the launch record."""
    x = torch.zeros((1, -(-ncols // 64) * 64 + 64), dtype=KINDS[kind][0], device=cuda)
    w = torch.ones(1, dtype=KINDS[kind][1], device=cuda)
    _, names = fold_chain(cuda, kind, x, w, (1,), 0, ncols)
    torch.cuda.synchronize()
    return depth_of(names[0])


# ---------------------------------------------------------------------------------------------
# chunkings of N
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind,mode,omode", FP32_MODES + WIDE_MODES, ids=lambda v: MODE_IDS.get(v, ""))
@pytest.mark.parametrize("n", [1, 2, 3, 17, 100])
def test_every_chunking_of_n_gives_the_single_sum(n, kind, mode, omode, cuda):
    """N in {1, 2, 3, 17, 100} at a narrow width (D = 16 for the fp32 kinds: K < D, K == D,
    D < K < 2D, 2D and 2D + 1 all occur); every chunking leaves the same accumulator bits."""
    ncols = 1025
    rng = np.random.default_rng(100 * n + kind)
    xh, wh, denom = _values(kind, rng, n, ncols)
    if omode == oracle.MODE_W32_DIV32:
        denom = float(np.float32(denom))
    d = _probe_depth(cuda, kind, ncols)
    assert d == (16 if kind in (na.ACC_F32, na.ACC_F32_W64) else 1)
    bits = {run_round(cuda, kind, mode, omode, xh, wh, denom, s, col_begin=64)[0] for s in chunkings(n, d)}
    assert len(bits) == 1


# chunks per block on a forced grid of 3 -> the (V, D) the plan picks, W = 4
DEPTH_SHARES = {5: (2, 8), 9: (4, 4), 17: (8, 2), 33: (16, 1), 130: (16, 1)}


@pytest.mark.parametrize("kind,mode,omode", [FP32_MODES[0], FP32_MODES[2]], ids=["f32", "w64"])
@pytest.mark.parametrize("share", sorted(DEPTH_SHARES))
def test_chunkings_at_every_pipeline_depth(share, kind, mode, omode, cuda, grid):
    """Every shipped (V, D) of fold_kernel_rows on a forced grid of 3 blocks: K around D and 2D;
    share 130: several rounds of 64-KiB pieces per block."""
    grid(3)
    ncols = 3 * share * 256 - 256 + 5
    n = 17
    xh, wh, denom = _values(kind, np.random.default_rng(share), n, ncols)
    d = _probe_depth(cuda, kind, ncols)
    bits = set()
    for s in chunkings(n, d):
        b, names = run_round(cuda, kind, mode, omode, xh, wh, denom, s)
        v, dd = DEPTH_SHARES[share]
        assert dd == 64 // (4 * v) and set(names) == {fold_rows_name(kind, v)}
        bits.add(b)
    assert len(bits) == 1


# ---------------------------------------------------------------------------------------------
# widths
# ---------------------------------------------------------------------------------------------

WIDTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, "grid", 208 * 16384 + 5]


@pytest.mark.parametrize("kind,mode,omode", [FP32_MODES[0], FP32_MODES[2], WIDE_MODES[0], WIDE_MODES[1]],
                         ids=["f32", "w64", "f64", "i64"])
@pytest.mark.parametrize("width", WIDTHS)
def test_widths_in_place_and_double_buffered(width, kind, mode, omode, cuda):
    """3 clients as (1, 1, 1) and (2, 1): the ragged last quad, one piece +-1, more 1-KiB chunks
    than blocks, more pieces than one round of the grid; a window inside wider rows (col_begin 64);
    the accumulator in place and double-buffered holds the same bits."""
    if width == "grid":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        width = int(cus * 0.75 + 0.5) * 256 + 1
    if width > 1 << 20 and kind in (na.ACC_F64, na.ACC_I64):
        width = 100_003  # the 8-byte kinds are small buckets: past the grid-stride cap of the kernel is enough
    xh, wh, denom = _values(kind, np.random.default_rng(width % 9973), 3, width)
    bits = set()
    for splits, double in (((1, 1, 1), False), ((1, 1, 1), True), ((2, 1), True), ((3,), False)):
        bits.add(run_round(cuda, kind, mode, omode, xh, wh, denom, splits, col_begin=64, double=double)[0])
    assert len(bits) == 1


def test_empty_window_is_a_no_op(cuda):
    L = na.lib()
    x = torch.zeros((2, 64), device=cuda)
    w = torch.ones(2, device=cuda)
    acc = Arr(4, torch.float32, cuda)
    out = Arr(4, torch.float32, cuda)
    assert L.fa_fold(na.ACC_F32, x.data_ptr(), 64, 2, w.data_ptr(), None, acc.t.data_ptr(), 0, 0, _stream(cuda)) == 0
    assert agg.last_launch()[0] is None
    assert L.fa_fold_finish(na.ACC_F32, na.MODE_W32_DIV64, acc.t.data_ptr(), 1.0, 0, None, out.t.data_ptr(), None,
                            _stream(cuda)) == 0
    assert agg.last_launch()[0] is None
    torch.cuda.synchronize()
    assert acc.untouched() and out.untouched()


# ---------------------------------------------------------------------------------------------
# IEEE corners
# ---------------------------------------------------------------------------------------------


def _corner_stack(n=6, reps=40):
    """Columns of special values, each placed in the first chunk (row 0) and, in another column, in
    a later chunk (row 3): +-0, a column that is -0.0 in every client, +-inf, inf - inf, NaN,
    denormals, and sums that overflow float32 in the running sum (first and later chunk)."""
    big, sub = np.float32(3e38), np.float32(1e-45)
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, np.float32(1.1754942e-38), big, -big]
    cols = []
    for r in (0, 3):
        for s in specials:
            c = np.ones(n, np.float32)
            c[r] = s
            cols.append(c)
        c = np.zeros(n, np.float32)  # zeros but one -0.0
        c[r] = -0.0
        cols.append(c)
        c = np.full(n, big, np.float32)  # overflow in the running sum, from row r on
        c[:r] = 1.0
        cols.append(c)
        c = np.ones(n, np.float32)  # inf - inf
        c[r], c[(r + 1) % n] = np.inf, -np.inf
        cols.append(c)
        c = np.full(n, sub, np.float32)  # a sum of denormals
        cols.append(c)
    cols.append(np.full(n, -0.0, np.float32))  # -0.0 in every client: the sum stays -0.0
    cols.append(np.zeros(n, np.float32))
    x = np.stack(cols, axis=1)
    return np.ascontiguousarray(np.tile(x, (1, reps))[:, : x.shape[1] * reps - 1])


@pytest.mark.parametrize("kind,mode,omode", FP32_MODES, ids=["div64", "div32", "w64"])
@pytest.mark.parametrize("splits", [(1, 1, 1, 1, 1, 1), (2, 2, 2), (3, 3), (1, 4, 1), (6,)])
def test_ieee_corners_in_first_and_later_chunks(splits, kind, mode, omode, cuda):
    xh = _corner_stack()
    wh = np.ones(6, np.float64 if kind == na.ACC_F32_W64 else np.float32)
    want = oracle.c_reduce(omode, xh, wh, 6.0)
    j = np.flatnonzero((xh == 0).all(axis=0) & np.signbit(xh).all(axis=0))  # -0.0 in every client
    assert len(j) and np.signbit(want[j]).all() and (want[j] == 0).all()
    assert np.isnan(want).any() and np.isinf(want).any()
    run_round(cuda, kind, mode, omode, xh, wh, 6.0, splits, col_begin=64, double=len(splits) == 3)


def test_f64_corners(cuda):
    x = np.array([[0.0, -0.0, np.inf, np.nan, 5e-324, 1.7e308, -0.0, 1.0],
                  [1.0, -0.0, -np.inf, 1.0, 5e-324, 1.7e308, -0.0, -1.0],
                  [-1.0, -0.0, 1.0, 1.0, -5e-324, 1.0, 0.0, 1e-300]])
    for splits in ((1, 1, 1), (2, 1), (1, 2), (3,)):
        run_round(cuda, na.ACC_F64, 0, "f64", x, np.array([1.0, 1.0, 1.0]), 3.0, splits)


# ---------------------------------------------------------------------------------------------
# epilogues: tests/epilogue_table.py through fold + fold_finish
# ---------------------------------------------------------------------------------------------

T_OF = {oracle.MODE_W32_DIV64: np.float64, oracle.MODE_W32_DIV32: np.float32, oracle.MODE_W64: np.float64}
TORCH_OF = {np.float32: torch.float32, np.float64: torch.float64}
OPS = ("mean", "avgm", "adagrad", "yogi", "adam", "dyn")
_TABLES = {}


def _table(T, kind):
    key = (np.dtype(T).name, kind)
    if key not in _TABLES:
        _TABLES[key] = table(T, kind, 4, 3)  # a ragged last quad
    return _TABLES[key]


@pytest.mark.parametrize("state", ["inplace", "v_out"])
@pytest.mark.parametrize("kind,mode,omode", FP32_MODES, ids=["div64", "div32", "w64"])
@pytest.mark.parametrize("op", range(1, 6), ids=OPS[1:])
def test_epilogue_table_through_fold_and_finish(op, kind, mode, omode, state, cuda):
    T = T_OF[omode]
    tdt = TORCH_OF[T]
    tab = _table(T, "dyn" if op == na.OP_DYN else "opt")
    ncols = len(tab.g)
    assert ncols % 4 == 3
    n = 3
    xh, _, _ = stack_for(tab.g, n)
    wh = np.ones(n, np.float64 if kind == na.ACC_F32_W64 else np.float32)
    x = _stack(xh, 0, cuda)
    w = torch.from_numpy(wh).to(cuda)
    acc, _ = fold_chain(cuda, kind, x, w, (1, 2), 0, ncols, double=True)
    l32 = Arr(ncols, torch.float32, cuda, tab.l32)
    v = Arr(ncols, tdt, cuda, tab.v)
    v_out = Arr(ncols, tdt, cuda) if state == "v_out" else None
    hyper = HYPERS["nondefault"] if op != na.OP_DYN else {}
    if op == na.OP_DYN:
        epi = na.Epilogue(op, 0, None, v.t.data_ptr(), 0, 0, 0, 0, l32.t.data_ptr(), 0.01, float(n),
                          v_out.t.data_ptr() if v_out else None)
    else:
        epi = na.Epilogue(op, 0, l32.t.data_ptr(), v.t.data_ptr(), hyper["beta"], hyper["eta"], hyper["tau"],
                          hyper["beta2"], None, 0.0, 0.0, v_out.t.data_ptr() if v_out else None)
    out32, out64 = finish(cuda, kind, mode, acc, 1.0, ncols, epi=epi, want64=T is np.float64)
    torch.cuda.synchronize()
    g = oracle.c_reduce(omode, xh, wh, 1.0)
    if op == na.OP_DYN:
        l_want, v_want = tab.l32.copy(), tab.v.copy()
        want = oracle.c_update_dyn(g, l_want, v_want, n)
    else:
        l_want, v_want = tab.l32, tab.v.copy()
        want = oracle.c_update(OPS[op], g, tab.l32, v_want, **hyper)
    with np.errstate(over="ignore", under="ignore"):
        _check("out32", out32.got(), want.astype(np.float32))
    if out64 is not None:
        _check("out64", out64.got(), want)
    _check("prev / h", l32.got(), l_want)
    if v_out is not None:
        _check("v_out", v_out.got(), v_want)
        _check("v (read only)", v.got(), tab.v)
    else:
        _check("v", v.got(), v_want)
    for name, a in (("out32", out32), ("out64", out64), ("l32", l32), ("v", v), ("v_out", v_out), ("acc", acc)):
        assert a is None or a.tail_intact(), f"{name}: written past the end"
    assert np.isnan(want).any() and not np.isnan(want).all()


def test_the_parametrisations_reach_every_finish_instantiation():
    """finish() holds every launch to fold_finish_name(kind, mode, op); the (kind, mode, op) of
    test_every_chunking_of_n_gives_the_single_sum (plain mean) and of
    test_epilogue_table_through_fold_and_finish (ops 1-5) are all 19 shipped instantiations."""
    means = {fold_finish_name(kind, mode, na.OP_MEAN) for kind, mode, _ in FP32_MODES + WIDE_MODES}
    fused = {fold_finish_name(kind, mode, op) for kind, mode, _ in FP32_MODES for op in range(1, 6)}
    assert means | fused == {t for t in FOLD_TARGETS if t.startswith("fold_finish_kernel<")}
    assert len(means | fused) == 19


# ---------------------------------------------------------------------------------------------
# validation: refused calls launch nothing and leave every output on its fill pattern
# ---------------------------------------------------------------------------------------------


def test_refused_calls_leave_the_outputs_untouched(cuda):
    L = na.lib()
    s = _stream(cuda)
    x = torch.zeros((2, 128), device=cuda)
    x8 = torch.zeros((2, 128), dtype=torch.float64, device=cuda)
    w = torch.ones(2, device=cuda)
    w8 = torch.ones(2, dtype=torch.float64, device=cuda)
    acc, acc8 = Arr(64, torch.float32, cuda), Arr(64, torch.float64, cuda)
    out32, out64 = Arr(64, torch.float32, cuda), Arr(64, torch.float64, cuda)
    v = Arr(64, torch.float64, cuda)
    a, o32, o64 = acc.t.data_ptr(), out32.t.data_ptr(), out64.t.data_ptr()

    def refused(rc, code):
        assert rc == code, (rc, L.fa_last_error())
        assert agg.last_launch()[0] is None

    # fa_fold
    refused(L.fa_fold(7, x.data_ptr(), 128, 2, w.data_ptr(), None, a, 0, 64, s), na.FA_ERR_ARG)  # unknown kind
    refused(L.fa_fold(-1, x.data_ptr(), 128, 2, w.data_ptr(), None, a, 0, 64, s), na.FA_ERR_ARG)
    refused(L.fa_fold(na.ACC_F32, x.data_ptr(), 128, 0, w.data_ptr(), None, a, 0, 64, s), na.FA_ERR_ARG)  # n_clients 0
    refused(L.fa_fold(na.ACC_F32, x.data_ptr(), 128, 2, w.data_ptr(), None, a, 1, 60, s), na.FA_ERR_ALIGN)  # window
    refused(L.fa_fold(na.ACC_F32, x.data_ptr(), 126, 2, w.data_ptr(), None, a, 0, 60, s), na.FA_ERR_ALIGN)  # stride
    refused(L.fa_fold(na.ACC_F64, x8.data_ptr(), 128, 2, w8.data_ptr(), None, acc8.t.data_ptr(), 1, 60, s),
            na.FA_ERR_ALIGN)
    refused(L.fa_fold(na.ACC_F32, x.data_ptr(), 128, 2, w.data_ptr(), None, a + 4, 0, 60, s), na.FA_ERR_ALIGN)  # acc
    refused(L.fa_fold(na.ACC_F32, x.data_ptr(), 128, 2, w.data_ptr(), a, a + 16, 0, 60, s), na.FA_ERR_ARG)  # overlap
    refused(L.fa_fold(na.ACC_F32, x.data_ptr(), 128, 2, w.data_ptr(), None, a, 100, 64, s), na.FA_ERR_ARG)  # > stride
    # fa_fold_finish
    refused(L.fa_fold_finish(9, 0, a, 1.0, 64, None, o32, o64, s), na.FA_ERR_ARG)
    refused(L.fa_fold_finish(na.ACC_F32, na.MODE_W32_DIV64, a, 1.0, 64, None, None, None, s), na.FA_ERR_ARG)  # no output
    refused(L.fa_fold_finish(na.ACC_F32, na.MODE_W32_DIV64, a + 4, 1.0, 60, None, o32, o64, s), na.FA_ERR_ALIGN)
    refused(L.fa_fold_finish(na.ACC_F32, na.MODE_W32_DIV64, a, 1.0, 60, None, o32 + 4, o64, s), na.FA_ERR_ALIGN)
    avgm = na.Epilogue(na.OP_AVGM, 0, o32, v.t.data_ptr(), 0.9, 0.1, 1e-9, 0.99)
    for k in (na.ACC_F64, na.ACC_I64):  # an epilogue on an 8-byte kind
        refused(L.fa_fold_finish(k, 0, acc8.t.data_ptr(), 1.0, 64, ctypes.byref(avgm), None, o64, s), na.FA_ERR_ARG)
    dyn = na.Epilogue(na.OP_DYN, 0, None, v.t.data_ptr(), 0, 0, 0, 0, o32, 0.01, 0.0)  # no N to take
    refused(L.fa_fold_finish(na.ACC_F32, na.MODE_W32_DIV64, a, 1.0, 64, ctypes.byref(dyn), None, o64, s), na.FA_ERR_ARG)
    over = na.Epilogue(na.OP_AVGM, 0, o32, v.t.data_ptr(), 0.9, 0.1, 1e-9, 0.99, None, 0, 0, v.t.data_ptr() + 32)
    refused(L.fa_fold_finish(na.ACC_F32, na.MODE_W32_DIV64, a, 1.0, 32, ctypes.byref(over), None, o64, s), na.FA_ERR_ARG)
    torch.cuda.synchronize()
    for name, arr in (("acc", acc), ("acc8", acc8), ("out32", out32), ("out64", out64), ("v", v)):
        assert arr.untouched(), name
