"""GPU: every reduce kernel instantiation the library ships, launched against the C oracle.

The host picks one of several hundred instantiations from the mode, the op, the window, the client
count, the CU count and fa_set_reduce_grid.  Each case of tests/instantiation_cases.py names the
one it means to reach; here the library's launch record (fa_last_launch) must name exactly that
kernel, and the outputs and every state array must equal the oracle's bit for bit.
tests/test_kernel_inventory.py closes the loop on a CPU box: the cases' targets are exactly the
kernels in the built library.

Every case: ncols % 4 != 0, col_begin = 4 x an odd number, NaN in the stack outside the window,
n = 2 * D + 3 for the target's pipeline depth (steady loop and both drains) unless the case says
otherwise, full-mantissa weights, v with zeros in it, every output and state array 64 elements
longer than the window with a sentinel tail that must survive."""
import numpy as np
import pytest
import torch

import oracle
from flearn_amd import AVG, AVGM, OPT, Dyn
from flearn_amd import _native as na
from flearn_amd import aggregator as agg
from golden_io import bitwise_equal
from instantiation_cases import (BALANCED, CASES, NONDEFAULT, OPS, SEGROWS_TARGETS, SEGROWS_WEIGHTS, Case,
                                 chunk_cols, resolve_ncols)

pytestmark = pytest.mark.gpu

TAIL = 64
SENT = {torch.float32: 0x7FA5A5A5, torch.float64: 0x7FF5A5A5A5A5A5A5}  # NaN payloads no kernel produces
INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64}
NP_OF = {torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture
def grid():
    """Sets fa_set_reduce_grid for one test and puts the previous value back."""
    prev = []

    def set_grid(g):
        prev.append(agg.set_reduce_grid(g))

    yield set_grid
    if prev:
        agg.set_reduce_grid(prev[0])


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Arr:
    """A device array of `ncols` values (host copy kept) followed by TAIL sentinel elements."""

    def __init__(self, host, dtype, cuda):
        self.n, self.dtype = len(host), dtype
        bits = torch.full((self.n + TAIL,), SENT[dtype], dtype=INT_OF[dtype], device=cuda)
        self.t = bits.view(dtype)
        self.host = np.ascontiguousarray(host, NP_OF[dtype])
        self.t[: self.n] = torch.from_numpy(self.host).to(cuda)

    @classmethod
    def out(cls, ncols, dtype, cuda):
        a = cls(np.zeros(ncols), dtype, cuda)
        a.t.view(INT_OF[dtype])[:ncols] = SENT[dtype]  # unwritten columns would show
        return a

    def got(self):
        return self.t[: self.n].cpu().numpy()

    def tail_intact(self):
        return bool((self.t.view(INT_OF[self.dtype])[self.n :] == SENT[self.dtype]).all())


def _stack(host, col_begin, cuda):
    """[n, stride] device stack, NaN everywhere but the window [col_begin, +ncols)."""
    n, ncols = host.shape
    stride = -(-(col_begin + ncols + TAIL) // 64) * 64
    x = torch.full((n, stride), float("nan"), dtype=torch.from_numpy(host[:0]).dtype, device=cuda)
    x[:, col_begin : col_begin + ncols] = torch.from_numpy(host).to(cuda)
    return x


def _weights(rng, n, mode):
    w = rng.uniform(0.25, 3.0, n)
    if mode == na.MODE_W64:
        return w, float(np.sum(w))
    w = w.astype(np.float32)
    return w, float(np.sum(w)) if mode == na.MODE_W32_DIV32 else float(np.sum(w.astype(np.float64)))


def _run_case(c, ncols, cuda, seed):
    """Runs one case; returns (launch record, list of (name, got, want), list of Arr)."""
    rng = np.random.default_rng(seed)
    tdt = torch.float32 if c.mode == na.MODE_W32_DIV32 else torch.float64
    xh = oracle.fill_uniform(c.n, ncols, seed)
    if c.reorder:  # same-sign terms, so the split order stands; every 5th column stays zero-mean
        keep = xh[:, ::5].copy()  # and is re-summed in list order by the kernel's cancellation guard
        xh = np.float32(0.5) * xh + np.float32(1.0)
        xh[:, ::5] = keep
    wh, denom = _weights(rng, c.n, c.mode)
    x = _stack(xh, c.col_begin, cuda)
    w = torch.from_numpy(wh).to(cuda)
    arrs, kw, checks = {}, {}, []
    arrs["out32"] = Arr.out(ncols, torch.float32, cuda)
    if tdt == torch.float64:
        arrs["out64"] = Arr.out(ncols, torch.float64, cuda)
    hyper = NONDEFAULT if (c.hyper and 1 <= c.op <= 4) else {}
    split_out = seed % 2 == 1  # the updated state into v_out, or in place
    if c.op:
        vh = rng.uniform(0.0, 0.5, ncols)
        vh[::7] = 0.0
        arrs["v"] = Arr(vh, tdt, cuda)
        if split_out:
            arrs["v_out"] = Arr.out(ncols, tdt, cuda)
            kw["v_out"] = arrs["v_out"].t
        lh = rng.uniform(-1.0, 1.0, ncols)
        if c.op == na.OP_DYN:
            arrs["h"] = Arr(0.5 * lh, torch.float32, cuda)
            kw.update(h=arrs["h"].t)
        else:
            arrs["prev"] = Arr(lh, torch.float32, cuda)
            kw.update(prev=arrs["prev"].t, **hyper)
        kw.update(op=c.op, v=arrs["v"].t)
    agg.reduce_stack(x, w, c.mode, denom, col_begin=c.col_begin, n_cols=ncols, out32=arrs["out32"].t,
                     out64=arrs["out64"].t if "out64" in arrs else None, reorder=c.reorder, **kw)
    rec = agg.last_launch()
    torch.cuda.synchronize()
    # the oracle
    g = (oracle.c_reduce_splitn if c.reorder else oracle.c_reduce)(c.mode, xh, wh, denom)
    want = g
    if c.reorder:  # the data tells the two orders apart, and the guard swaps some columns back
        assert (g != oracle.c_reduce(c.mode, xh, wh, denom)).any()
        assert (g != oracle.c_reduce_splitn(c.mode, xh, wh, denom, guard=False)).any()
    if c.op:
        v_new = arrs["v"].host.copy()
        if c.op == na.OP_DYN:
            h_new = arrs["h"].host.copy()
            want = oracle.c_update_dyn(g, h_new, v_new, c.n)
            checks.append(("h", arrs["h"].got(), h_new))
        else:
            want = oracle.c_update(OPS[c.op], g, arrs["prev"].host, v_new, **hyper)
            checks.append(("prev", arrs["prev"].got(), arrs["prev"].host))
        if split_out:
            checks += [("v_out", arrs["v_out"].got(), v_new), ("v (read only)", arrs["v"].got(), arrs["v"].host)]
        else:
            checks.append(("v", arrs["v"].got(), v_new))
    checks.append(("out32", arrs["out32"].got(), want.astype(np.float32)))
    if "out64" in arrs:
        checks.append(("out64", arrs["out64"].got(), want))
    return rec, checks, arrs


def _case_id(i):
    c = CASES[i]
    return f"{i}-{c.target.split('<')[0][14:]}-m{c.mode}-{OPS[c.op]}-g{c.grid}-n{c.n}"


@pytest.mark.parametrize("i", range(len(CASES)), ids=_case_id)
def test_instantiation_against_oracle(i, cuda, grid):
    c = CASES[i]
    ncols = resolve_ncols(c, _cus())
    assert ncols % 4 != 0 and c.col_begin % 8 == 4
    grid(c.grid)
    (kernel, _, launches), checks, arrs = _run_case(c, ncols, cuda, seed=1000 + i)
    assert kernel == c.target, f"the shape no longer reaches its kernel: launched {kernel}"
    assert launches == 1
    for name, got, want in checks:
        assert bitwise_equal(got, want), (name, int((got.view(np.uint8) != want.view(np.uint8)).sum()))
    for name, a in arrs.items():
        assert a.tail_intact(), f"{name}: written past the window"


# ---------------------------------------------------------------------------------------------
# "Results never depend on it" (fa_set_reduce_grid)
# ---------------------------------------------------------------------------------------------

GRIDS = (0, 1, 2, 3, 5, 7, 160)


@pytest.mark.parametrize("mode,op", [(na.MODE_W32_DIV32, na.OP_AVGM), (na.MODE_W64, na.OP_MEAN)])
def test_results_do_not_depend_on_the_grid(mode, op, cuda, grid):
    c = Case("", 0, mode, op, 7, 300_003, 12, False, False)
    results, kernels = [], set()
    for g in GRIDS:
        grid(g)
        (kernel, gr, launches), checks, arrs = _run_case(c, c.ncols, cuda, seed=77)  # same data every time
        assert launches == 1 and (g == 0 or gr == g), (g, gr)
        kernels.add(kernel)
        results.append(checks)
        assert all(a.tail_intact() for a in arrs.values())
    for name, got, want in results[0]:
        assert bitwise_equal(got, want), name  # the natural grid against the oracle
    for g, checks in zip(GRIDS[1:], results[1:]):
        for (name, got, _), (_, got0, _) in zip(checks, results[0]):
            assert bitwise_equal(got, got0), (g, name)
    assert len(kernels) >= 2, kernels  # the grids did take different kernels


# ---------------------------------------------------------------------------------------------
# column-window splits of wide fp32-sum windows, float32 state (epi_at's offsets with T = float)
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("op,ncols,launches", [(na.OP_MEAN, (8 << 20) + 5, 2), (na.OP_AVGM, (16 << 20) + 5, 3)])
def test_window_splits_div32(op, ncols, launches, cuda):
    c = Case("", 0, na.MODE_W32_DIV32, op, 2, ncols, 4, False, False)
    assert na.load().fa_reduce_windows(op, ncols) == launches
    (_, _, got_launches), checks, arrs = _run_case(c, ncols, cuda, seed=5)
    assert got_launches == launches
    for name, got, want in checks:
        assert bitwise_equal(got, want), name
    assert all(a.tail_intact() for a in arrs.values())


# ---------------------------------------------------------------------------------------------
# the row-pointer kernel (fa_reduce_f32_rows), all 18 instantiations, through the Strategy API
# ---------------------------------------------------------------------------------------------

ROWS_LAYOUT = [("t70001", 70001), ("t6000", 6000), ("t2049", 2049), ("t2048", 2048), ("t300", 300), ("t7", 7),
               ("t1", 1)]  # an odd number of wide pieces (one group of 2 lacks a piece), 4 narrow ones
STRATEGIES = ("mean", "avgm", "adagrad", "yogi", "adam", "dyn")


@pytest.fixture(scope="module")
def rows_data():
    """Host clients (19 of them), the previous model and the FedDyn state, shared and never changed."""
    total = sum(m for _, m in ROWS_LAYOUT)
    flat = oracle.fill_uniform(21, total, seed=31)
    dicts = []
    for r in range(21):
        d, off = {}, 0
        for k, m in ROWS_LAYOUT:
            d[k] = flat[r, off : off + m].copy()
            off += m
        dicts.append(d)
    return dicts[:19], dicts[19], dicts[20]


def test_row_pointer_layout_leaves_a_group_short(cuda):
    """What the comment on ROWS_LAYOUT claims, from the library's own plan on this device: an odd
    number of wide pieces (the last group of 2 has one) and several narrow ones."""
    import ctypes

    L = na.load()
    lens = [m for _, m in ROWS_LAYOUT]
    cols = [sum(-(-x // 64) * 64 for x in lens[:i]) for i in range(len(lens))]
    c, n = (ctypes.c_int64 * len(lens))(*cols), (ctypes.c_int64 * len(lens))(*lens)
    cnt, g = ctypes.c_int64(), ctypes.c_int32()
    for op in range(6):
        assert L.fa_rows_plan(len(lens), c, n, op, 0, None, 0, ctypes.byref(cnt), ctypes.byref(g)) == 0
        arr = (na.Piece * cnt.value)()
        assert L.fa_rows_plan(len(lens), c, n, op, 0, arr, cnt.value, ctypes.byref(cnt), ctypes.byref(g)) == 0
        nwide = arr[0].aux
        assert nwide % 2 == 1 and nwide >= 3 and cnt.value - nwide >= 3, (op, nwide, cnt.value)


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.mark.parametrize("n", [1, 2, 19])
@pytest.mark.parametrize("wkind", sorted(SEGROWS_WEIGHTS))
@pytest.mark.parametrize("strat", STRATEGIES)
def test_row_pointer_kernel_instantiations(strat, wkind, n, cuda, rows_data):
    clients, prev, h0 = rows_data
    clients = clients[:n]
    rng = np.random.default_rng(n)
    wt = {"pyfloat": float, "np32": np.float32, "np64": np.float64}[wkind]
    weights = [wt(x) for x in rng.uniform(0.25, 3.0, n)]
    g = oracle.server_ensemble(weights, [{k: v.copy() for k, v in c.items()} for c in clients])
    h_want = None
    if strat == "mean":
        s, want = AVG(), g
    elif strat == "dyn":
        s = Dyn({k: v.copy() for k, v in h0.items()})
        h_want = {k: v.copy() for k, v in h0.items()}
        want, _ = oracle.dyn_f(dict(g), h_want, {k: v.copy() for k, v in h0.items()}, n)
    else:
        s = AVGM(server_side=True) if strat == "avgm" else OPT(server_side=True, method=strat)
        s.server_opt.init_global({k: v.copy() for k, v in prev.items()})
        if strat == "avgm":
            want, _ = oracle.mean_momentum(dict(prev), g, None, 0.9)
        else:
            want, _ = oracle.adaptive_opt(dict(prev), g, None, strat)
    dev = [{k: torch.from_numpy(v).to(cuda) for k, v in c.items()} for c in clients]
    got = s.server([{"agg_weight": a, "params": c} for a, c in zip(weights, dev)], 0)["w_glob"]
    kernel, _, launches = agg.last_launch()
    assert s.engine.packer.last_row_tables["f32"] == "rows"
    assert kernel == SEGROWS_TARGETS[(wkind, STRATEGIES.index(strat))] and launches == 1
    assert set(got) == set(want)
    for k in want:
        assert bitwise_equal(_host(got[k]), np.asarray(want[k])), (k, _host(got[k]).dtype, np.asarray(want[k]).dtype)
    if h_want is not None:
        for k in h_want:
            assert bitwise_equal(_host(s.h[k]), h_want[k]), k


# ---------------------------------------------------------------------------------------------
# the 8-byte kernel (reduce_kernel_balanced): float64 models, int64 counters
# ---------------------------------------------------------------------------------------------

REDUCE8 = {"f64": (agg.reduce_stack_f64, torch.float64, np.float64),
           "i64": (agg.reduce_stack_i64, torch.int64, np.int64)}


def _values8(kind, rng, n, ncols):
    if kind == "f64":
        return rng.standard_normal((n, ncols)), rng.uniform(0.25, 3.0, n)
    return rng.integers(-1000, 1000, (n, ncols), dtype=np.int64), rng.integers(1, 601, n, dtype=np.int64)


def _run8(kind, xh, wh, col_begin, cuda):
    """One fa_reduce_f64 / _i64 over the window, checked against the oracle; returns the record."""
    fn, tdt, _ = REDUCE8[kind]
    n, ncols = xh.shape
    stride = -(-(col_begin + ncols + TAIL) // 64) * 64
    # outside the window: NaN (f64) / a huge value (i64)
    x = torch.full((n, stride), float("nan") if kind == "f64" else 2**62 + 12345, dtype=tdt, device=cuda)
    x[:, col_begin : col_begin + ncols] = torch.from_numpy(xh).to(cuda)
    out = Arr.out(ncols, torch.float64, cuda)
    denom = float(np.sum(wh))
    fn(x, torch.from_numpy(wh).to(cuda), denom, out.t, col_begin=col_begin, n_cols=ncols)
    rec = agg.last_launch()
    torch.cuda.synchronize()
    want = oracle.c_reduce(kind, xh, wh, denom)
    got = out.got()
    assert rec[0] == BALANCED[kind] and rec[2] == 1
    assert bitwise_equal(got, want), np.flatnonzero(got.view(np.int64) != want.view(np.int64))[:8]
    assert out.tail_intact()
    return rec


@pytest.fixture(scope="module")
def slots8(cuda):
    """Resident blocks of the 8-byte kernel on this device (CUs x occupancy), per kind: the grid of
    a launch with more chunks than that."""
    out = {}
    for kind in REDUCE8:
        xh, wh = _values8(kind, np.random.default_rng(1), 1, chunk_cols(16384))
        grid = _run8(kind, xh, wh, 4, cuda)[1]
        assert grid < 16384
        out[kind] = grid
    return out


@pytest.mark.parametrize("kind", sorted(REDUCE8))
@pytest.mark.parametrize("col_begin", [4, 260])
def test_balanced_one_chunk_per_block(kind, col_begin, cuda):
    xh, wh = _values8(kind, np.random.default_rng(col_begin), 9, chunk_cols(5))
    assert _run8(kind, xh, wh, col_begin, cuda)[1] == 5  # five blocks, the last chunk ragged


@pytest.mark.parametrize("kind", sorted(REDUCE8))
@pytest.mark.parametrize("per,n", [(2, 3), (3, 1), (6, 2), (11, 1)])
def test_balanced_masked_subtiles_with_remainder(kind, per, n, cuda, slots8):
    """Several chunks a block with a non-zero `extra`, less than one 16-chunk sub-tile: kMasked.  A
    slot is 4 chunks (256 quads), so per = 2..3 leaves each wave at most its first slot (nv <= 1)
    and per = 6 / 11 give nv = 2 / 3 (blocks with the extra chunk: one wave more)."""
    slots = slots8[kind]
    chunks = per * slots + slots // 2 + 1
    xh, wh = _values8(kind, np.random.default_rng(per), n, chunk_cols(chunks))
    grid = _run8(kind, xh, wh, 260, cuda)[1]
    assert grid == slots and chunks // grid == per and chunks % grid != 0


@pytest.mark.parametrize("kind", sorted(REDUCE8))
def test_balanced_full_then_masked_then_ragged(kind, cuda, slots8):
    """per >= 17: a kFull sub-tile (16 chunks), then a masked one, and the ragged window end."""
    slots = slots8[kind]
    chunks = 17 * slots + 3
    xh, wh = _values8(kind, np.random.default_rng(17), 2, chunk_cols(chunks))
    grid = _run8(kind, xh, wh, 4, cuda)[1]
    assert grid == slots and chunks // grid >= 17 and xh.shape[1] % 4 != 0


EDGE_COLS = (0, 255, 256, 4095, 4096, -1)


def test_balanced_f64_special_values(cuda):
    """NaN, +-inf, -0.0 and subnormals at the chunk and sub-tile edges (columns 0, 255, 256, 4095,
    4096 and the last).  Every NaN result is a propagated input NaN (no inf - inf, no 0 * inf), so
    its bits are defined."""
    rng = np.random.default_rng(3)
    n, ncols = 5, chunk_cols(33)
    xh, wh = _values8("f64", rng, n, ncols)
    tiny, quarter_min = np.float64(5e-324), np.float64(2.2250738585072014e-308) / 4
    xh[2, 0] = np.nan
    xh[0, 255] = np.inf
    xh[1, 256] = -np.inf
    xh[:, 4095] = -0.0  # every client -0.0: the mean is -0.0
    xh[:, 4096] = [tiny * k for k in (1, 3, 5, 2, 7)]  # subnormal products and sums
    xh[:, -1] = [quarter_min, -quarter_min, tiny, -0.0, quarter_min]
    xh[4, 1] = np.nan  # and inside a chunk: NaN after an infinity
    xh[0, 1] = -np.inf
    _run8("f64", xh, wh, 4, cuda)


def test_balanced_i64_wraps_and_rounds(cuda):
    """Products and sums that wrap (values near +-2**62, weights up to 600), and exact sums beyond
    2**53 (the int64 -> float64 rounding before the divide)."""
    rng = np.random.default_rng(4)
    n, ncols = 7, chunk_cols(33)
    xh, wh = _values8("i64", rng, n, ncols)
    wh[:3] = [600, 599, 1]
    big = (2**62 - rng.integers(0, 1000, (n, len(EDGE_COLS)))) * rng.choice([-1, 1], (n, len(EDGE_COLS)))
    xh[:, list(EDGE_COLS)] = big
    past53 = 2**53 // 600 + rng.integers(1, 2**20, (n, 64)) * 2 + 1  # odd: sums past 2**53 are inexact
    xh[:, 1000:1064] = past53
    exact = (xh[:, 1000:1064].astype(object) * wh[:, None].astype(object)).sum(axis=0)
    assert all(2**53 < int(e) < 2**63 for e in exact)
    assert sum(int(float(int(e))) != int(e) for e in exact) >= 8  # not representable: the cast rounds
    _run8("i64", xh, wh, 260, cuda)
