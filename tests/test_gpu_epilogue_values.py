"""GPU: the fused epilogues' arithmetic over the whole float range and the IEEE special values.

tests/epilogue_table.py drives the divide by sum(a), d*d, the square root, the second divide and
the stores' casts of update / epi_compute / finish_quad / finish_piece / apply_kernel
(flearn_amd/csrc/fa_device.hpp) with subnormal, near-overflow, zero, infinite and NaN operands, with
exact ties and with cancellation.  Everything is compared with oracle.c_reduce + c_update /
c_update_dyn, which tests/test_epilogue_table.py ties to numpy on the same table: NaN exactly where
the oracle has NaN, every other column bit-identical (-0.0 is not +0.0), in out32, out64, the
updated v_t / theta and h; prev and the v_t a step reads stay unchanged; sentinels behind every
array, and between the windows, survive.

(a) the standalone update (apply_update / apply_dyn) runs the whole table, every op x precision x
    hyper-parameter set, at a length with % 4 == 3;
(b) every fused-epilogue kernel family runs it at the smallest shape that reaches the family
    (tests/instantiation_cases.py), n = 1 (8 for split-N), the launch record naming the kernel.
    Families narrower than the table walk it in non-overlapping windows over one uploaded stack;
(c) the plain mean's divide and out32 cast run the mean columns through a narrow and a row-major
    shape."""
import numpy as np
import pytest
import torch

import oracle
from epilogue_table import (DYN_HYPERS, HYPERS, OPT_OPS, W64_WEIGHTS, first_diffs, mean_columns,
                            same_values, stack_for, table)
from flearn_amd import AVG, AVGM, OPT, Dyn
from flearn_amd import _native as na
from flearn_amd import aggregator as agg
from instantiation_cases import (OPS, SEGROWS_TARGETS, chunk_cols, narrow_name, rowmajor_name, rows_name,
                                 splitn_name)
from test_gpu_instantiations import INT_OF, NP_OF, SENT, TAIL, Arr

pytestmark = pytest.mark.gpu

T_OF_MODE = {na.MODE_W32_DIV64: np.float64, na.MODE_W32_DIV32: np.float32, na.MODE_W64: np.float64}
TORCH_OF = {np.float32: torch.float32, np.float64: torch.float64}
MODES = (na.MODE_W32_DIV64, na.MODE_W32_DIV32, na.MODE_W64)

_TABLES = {}


def _table(T, kind, pad_to=1, rem=0):
    """Tables are built once and never changed (the oracle's in-place updates get copies)."""
    key = (np.dtype(T).name, kind, pad_to, rem)
    if key not in _TABLES:
        _TABLES[key] = table(T, kind, pad_to, rem)
    return _TABLES[key]


def _check(name, got, want):
    assert same_values(got, want), (name,) + first_diffs(got, want)


# ---------------------------------------------------------------------------------------------
# (a) the standalone update: apply_kernel -> finish_quad (guarded loads, the ragged last quad)
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hyper", sorted(HYPERS))
@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("op", OPT_OPS)
def test_standalone_update_over_the_table(op, t, hyper, cuda):
    T = {"f32": np.float32, "f64": np.float64}[t]
    tab = _table(T, "opt", 4, 3)
    n = len(tab.g)
    assert n % 4 == 3
    tdt = TORCH_OF[T]
    g, prev, v = Arr(tab.g, tdt, cuda), Arr(tab.l32, torch.float32, cuda), Arr(tab.v, tdt, cuda)
    out32 = Arr.out(n, torch.float32, cuda)
    out64 = Arr.out(n, torch.float64, cuda) if T is np.float64 else None
    agg.apply_update(na.OP_BY_NAME[op], prev.t[:n], g.t[:n], v.t[:n], out32=out32.t[:n],
                     out64=out64.t[:n] if out64 else None, **HYPERS[hyper])
    torch.cuda.synchronize()
    v_want = tab.v.copy()
    want = oracle.c_update(op, tab.g, tab.l32, v_want, **HYPERS[hyper])
    with np.errstate(over="ignore", under="ignore"):
        _check("out32", out32.got(), want.astype(np.float32))
    if out64:
        _check("out64", out64.got(), want)
    _check("v", v.got(), v_want)
    _check("prev", prev.got(), tab.l32)
    _check("glob", g.got(), tab.g)
    for name, a in (("glob", g), ("prev", prev), ("v", v), ("out32", out32), ("out64", out64)):
        assert a is None or a.tail_intact(), f"{name}: written past the end"


@pytest.mark.parametrize("alpha,n_clients", DYN_HYPERS)
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_standalone_dyn_over_the_table(t, alpha, n_clients, cuda):
    T = {"f32": np.float32, "f64": np.float64}[t]
    tab = _table(T, "dyn", 4, 3)
    n = len(tab.g)
    assert n % 4 == 3
    tdt = TORCH_OF[T]
    g, h, th = Arr(tab.g, tdt, cuda), Arr(tab.l32, torch.float32, cuda), Arr(tab.v, tdt, cuda)
    out32 = Arr.out(n, torch.float32, cuda)
    out64 = Arr.out(n, torch.float64, cuda) if T is np.float64 else None
    agg.apply_dyn(g.t[:n], h.t[:n], th.t[:n], n_clients, alpha, out32=out32.t[:n], out64=out64.t[:n] if out64 else None)
    torch.cuda.synchronize()
    h_want, th_want = tab.l32.copy(), tab.v.copy()
    want = oracle.c_update_dyn(tab.g, h_want, th_want, n_clients, alpha=alpha)
    with np.errstate(over="ignore", under="ignore"):
        _check("out32", out32.got(), want.astype(np.float32))
    if out64:
        _check("out64", out64.got(), want)
    _check("theta", th.got(), th_want)
    _check("h", h.got(), h_want)
    _check("glob", g.got(), tab.g)
    for name, a in (("glob", g), ("h", h), ("theta", th), ("out32", out32), ("out64", out64)):
        assert a is None or a.tail_intact(), f"{name}: written past the end"


# ---------------------------------------------------------------------------------------------
# (b) the fused kernels
# ---------------------------------------------------------------------------------------------


class Windows:
    """A device array of nwin windows of `width` columns, `pitch` (a multiple of 4) apart, with
    sentinels in the gaps between the windows and in a tail of TAIL elements."""

    def __init__(self, nwin, width, dtype, cuda, host=None):
        self.nwin, self.width, self.dtype = nwin, width, dtype
        self.pitch = -(-width // 4) * 4
        bits = torch.full((nwin * self.pitch + TAIL,), SENT[dtype], dtype=INT_OF[dtype], device=cuda)
        self.t = bits.view(dtype)
        if host is not None:
            self.host = np.ascontiguousarray(host, NP_OF[dtype])
            self._cells(self.t)[:] = torch.from_numpy(self.host.reshape(nwin, width)).to(cuda)

    def _cells(self, t):
        return t[: self.nwin * self.pitch].unflatten(0, (self.nwin, self.pitch))[:, : self.width]

    def at(self, k):
        return self.t[k * self.pitch :]

    def got(self):
        return self._cells(self.t).cpu().numpy().reshape(-1)

    def intact(self):
        bits = self.t.view(INT_OF[self.dtype])
        gaps = bits[: self.nwin * self.pitch].unflatten(0, (self.nwin, self.pitch))[:, self.width :]
        return bool((gaps == SENT[self.dtype]).all()) and bool((bits[self.nwin * self.pitch :] == SENT[self.dtype]).all())


def _window_stack(x, nwin, width, cuda):
    """[n, nwin * width] host values as a device stack of windows `pitch` apart, NaN elsewhere."""
    n = x.shape[0]
    pitch = -(-width // 4) * 4
    stride = -(-(nwin * pitch + TAIL) // 64) * 64
    xs = torch.full((n, stride), float("nan"), dtype=torch.float32, device=cuda)
    cells = xs[:, : nwin * pitch].unflatten(1, (nwin, pitch))[:, :, :width]
    cells[:] = torch.from_numpy(np.ascontiguousarray(x).reshape(n, nwin, width)).to(cuda)
    return xs


def _variants(mode, denoms=(1.0,)):
    """(weight of row 0, denom) per window, in turn: the given denoms, and under MODE_W64 the
    float64 weights that carry the sum beyond the float32 range."""
    if mode == na.MODE_W64 and len(denoms) == 1:
        return [(w, denoms[0]) for w in W64_WEIGHTS]
    if mode == na.MODE_W32_DIV32:
        return [(1.0, float(np.float32(d))) for d in denoms]
    return [(1.0, float(d)) for d in denoms]


def _run_windows(cuda, mode, op, x, l32, v, width, target, *, reorder=False, hyper=None, variants=None,
                 variant_of=None):
    """Runs op over x (host [n, ncols], ncols a multiple of width) window by window, the state
    from l32 / v, and checks everything against the oracle.  Window k takes variants[variant_of(k)]."""
    n, ncols = x.shape
    nwin = ncols // width
    assert nwin * width == ncols
    T = T_OF_MODE[mode]
    tdt = TORCH_OF[T]
    wdt = np.float64 if mode == na.MODE_W64 else np.float32
    variants = variants or _variants(mode)
    variant_of = variant_of or (lambda k: k % len(variants))
    hyper = hyper or {}
    xs = _window_stack(x, nwin, width, cuda)
    ws = []
    for w0, _ in variants:
        wh = np.ones(n, wdt)
        wh[0] = w0
        ws.append((wh, torch.from_numpy(wh).to(cuda)))
    arrs = {"out32": Windows(nwin, width, torch.float32, cuda)}
    if T is np.float64:
        arrs["out64"] = Windows(nwin, width, torch.float64, cuda)
    if op != na.OP_MEAN:
        arrs["v"] = Windows(nwin, width, tdt, cuda, v)
        arrs["v_out"] = Windows(nwin, width, tdt, cuda)
        arrs["h" if op == na.OP_DYN else "prev"] = Windows(nwin, width, torch.float32, cuda, l32)
    for k in range(nwin):
        i = variant_of(k)
        kw = {}
        if op != na.OP_MEAN:
            kw = dict(op=op, v=arrs["v"].at(k), v_out=arrs["v_out"].at(k), **hyper)
            if op == na.OP_DYN:
                kw["h"] = arrs["h"].at(k)
            else:
                kw["prev"] = arrs["prev"].at(k)
        agg.reduce_stack(xs, ws[i][1], mode, variants[i][1], col_begin=k * arrs["out32"].pitch, n_cols=width,
                         out32=arrs["out32"].at(k), out64=arrs["out64"].at(k) if "out64" in arrs else None,
                         reorder=reorder, **kw)
        kernel, _, launches = agg.last_launch()
        assert kernel == target and launches == 1, f"window {k}: the shape no longer reaches its kernel: {kernel}"
    torch.cuda.synchronize()
    # the oracle: the mean per variant, each column taking its window's
    red = oracle.c_reduce_splitn if reorder else oracle.c_reduce
    col_variant = np.repeat([variant_of(k) for k in range(nwin)], width)
    g = np.empty(ncols, T)
    for i, (_, denom) in enumerate(variants):
        if (col_variant == i).any():
            g[col_variant == i] = red(mode, x, ws[i][0], denom)[col_variant == i]
    want = g
    if op == na.OP_DYN:
        h_want, th_want = l32.copy(), v.copy()
        want = oracle.c_update_dyn(g, h_want, th_want, n, **hyper)
        _check("h", arrs["h"].got(), h_want)
        _check("theta (v_out)", arrs["v_out"].got(), th_want)
    elif op != na.OP_MEAN:
        v_want = v.copy()
        want = oracle.c_update(OPS[op], g, l32, v_want, **hyper)
        _check("v_out", arrs["v_out"].got(), v_want)
        _check("prev", arrs["prev"].got(), l32)
    if op != na.OP_MEAN:
        _check("v (read only)", arrs["v"].got(), v)
    with np.errstate(over="ignore", under="ignore"):
        _check("out32", arrs["out32"].got(), want.astype(np.float32))
    if "out64" in arrs:
        _check("out64", arrs["out64"].got(), want)
    for name, a in arrs.items():
        assert a.intact(), f"{name}: written outside a window"
    return g, want


@pytest.fixture
def grid():
    """Sets fa_set_reduce_grid for one test and puts the previous value back."""
    prev = []

    def set_grid(g):
        prev.append(agg.set_reduce_grid(g))

    yield set_grid
    if prev:
        agg.set_reduce_grid(prev[0])


# family -> (forced grid, window width, rows, reorder, kernel name of (mode, op), modes)
ROWMAJOR_XL, ROWMAJOR_K4 = chunk_cols(64 * 3 * 2 + 7), chunk_cols(64 * 3 * 3 + 7)
FAMILIES = {
    "narrow": (0, 517, 1, False, lambda m, o: narrow_name(m, o, 16), MODES),
    "rows": (1, chunk_cols(3), 1, False, lambda m, o: rows_name(m, o, 1, 4), MODES),
    # three pieces a block (KG = 3): the float64 epilogues store whole lines through LDS (XL)
    "rowmajor_xl": (3, ROWMAJOR_XL, 1, False, lambda m, o: rowmajor_name(m, o, False, 3), MODES[:2]),
    # four pieces a block (KG = 4): the plain stores (row-major groups sum in float32 only)
    "rowmajor": (3, ROWMAJOR_K4, 1, False, lambda m, o: rowmajor_name(m, o, False, 4), MODES[:2]),
    "splitn": (0, 517, 8, True, lambda m, o: splitn_name(m, o), MODES),
}
FUSED_CASES = [(f, m, o) for f, spec in FAMILIES.items() for m in spec[5] for o in range(6)]


def _fused(cuda, grid, family, mode, op, hyper=None):
    g_, width, n, reorder, name, _ = FAMILIES[family]
    grid(g_)
    T = T_OF_MODE[mode]
    if op == na.OP_MEAN:
        tab = _table(T, "opt", width)
    else:
        tab = _table(T, "dyn" if op == na.OP_DYN else "opt", width)
    x, _, _ = stack_for(tab.g, n)
    assert len(tab.g) % width == 0 and len(tab.g) >= tab.n_cross + 8192
    return _run_windows(cuda, mode, op, x, tab.l32, tab.v, width, name(mode, op), reorder=reorder, hyper=hyper)


@pytest.mark.parametrize("family,mode,op", FUSED_CASES, ids=[f"{f}-m{m}-{OPS[o]}" for f, m, o in FUSED_CASES])
def test_fused_epilogue_over_the_table(family, mode, op, cuda, grid):
    """Every column of the table through every fused family, at the reference's hyper-parameters
    (FedDyn: alpha = 0.01, N = the launch's rows)."""
    _, want = _fused(cuda, grid, family, mode, op)
    # the launch did see the value classes (the oracle's results on what the kernel was given;
    # tests/test_epilogue_table.py counts them class by class)
    assert np.isnan(want).any() and (want == 0).any() and not np.isnan(want).all()
    with np.errstate(over="ignore", under="ignore"):
        w32 = want.astype(np.float32)
    assert ((w32 != 0) & (np.abs(w32) < np.finfo(np.float32).tiny)).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", [na.OP_AVGM, na.OP_ADAGRAD, na.OP_YOGI, na.OP_ADAM])
def test_fused_epilogue_degenerate_hypers(op, mode, cuda, grid):
    """beta = 0, eta = 1, tau = 0, beta2 = 0 (x / 0 and 0 / 0 in the step), through the narrow family."""
    _fused(cuda, grid, "narrow", mode, op, hyper=HYPERS["degenerate"])


def test_xl_flag_of_the_rowmajor_shapes():
    """What FAMILIES claims (the launch records above then check the names): the first row-major
    shape is the XL = true kernel for float64 fused epilogues, the second XL = false."""
    for op in range(1, 6):
        assert FAMILIES["rowmajor_xl"][4](0, op).endswith(",true>")
        assert FAMILIES["rowmajor"][4](0, op).endswith(",false>")
        assert FAMILIES["rowmajor_xl"][4](1, op).endswith(",false>")  # float32 epilogues have no XL form


# ---- the row-pointer kernel (reduce_kernel_segrows_rm) through AVG / AVGM / OPT / Dyn ----------

SEG_SIZES = (7, 300, 2049, 6000)  # narrow and wide pieces; the rest of the table is the last tensor
SEG_WEIGHTS = {"pyfloat": 1.0, "np32": np.float32(1), "np64": np.float64(1), "np64big": np.float64(W64_WEIGHTS[1])}
SEG_KIND = {"pyfloat": "pyfloat", "np32": "np32", "np64": "np64", "np64big": "np64"}
SEG_MODE = {"pyfloat": na.MODE_W32_DIV64, "np32": na.MODE_W32_DIV32, "np64": na.MODE_W64, "np64big": na.MODE_W64}


def _split(a):
    out, off = {}, 0
    for i, m in enumerate(SEG_SIZES + (len(a) - sum(SEG_SIZES),)):
        out[f"t{i}"] = np.array(a[off : off + m])
        off += m
    return out


def _join(d):
    host = [v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in
            (d[f"t{i}"] for i in range(len(SEG_SIZES) + 1))]
    return np.concatenate([h.reshape(-1) for h in host])


@pytest.mark.parametrize("wkind", sorted(SEG_WEIGHTS))
@pytest.mark.parametrize("strat", OPS)
def test_row_pointer_epilogue_over_the_table(strat, wkind, cuda):
    """Device uploads read in place, server_side=True, the state restored by load_state (a foreign
    v_t goes straight to the kernel) or given to Dyn.  np64big: a float64 weight of 2^900, so the
    product leaves the float32 range (and overflows) before the divide by sum(a) = 2^900."""
    mode, weight = SEG_MODE[wkind], SEG_WEIGHTS[wkind]
    T = T_OF_MODE[mode]
    op = OPS.index(strat)
    tab = _table(T, "dyn" if strat == "dyn" else "opt")
    x, _, _ = stack_for(tab.g)
    wh = np.array([weight], np.float64 if mode == na.MODE_W64 else np.float32)
    g = oracle.c_reduce(mode, x, wh, float(np.sum([weight])))
    ups = [{"agg_weight": weight, "params": {k: torch.from_numpy(a).to(cuda) for k, a in _split(x[0]).items()}}]
    checks = []
    if strat == "mean":
        s = AVG()
        got = s.server(ups, 0)["w_glob"]
        want = g
    elif strat == "dyn":
        s = Dyn(_split(tab.l32))
        s.theta = _split(tab.v)
        got = s.server(ups, 0)["w_glob"]
        h_want, th_want = tab.l32.copy(), tab.v.copy()
        want = oracle.c_update_dyn(g, h_want, th_want, 1)
        checks.append(("h", _join(s.h), h_want))
    else:
        s = AVGM(server_side=True) if strat == "avgm" else OPT(server_side=True, method=strat)
        s.server_opt.load_state({"w_glob": _split(tab.l32), "v_t": _split(tab.v)})
        got = s.server(ups, 0)["w_glob"]
        v_want = tab.v.copy()
        want = oracle.c_update(strat, g, tab.l32, v_want)
        state = s.server_opt.state_dict()
        checks.append(("v_t", _join(state["v_t"]), v_want))
        with np.errstate(over="ignore", under="ignore"):
            checks.append(("out32 (the next round's w_glob)", _join(state["w_glob"]), want.astype(np.float32)))
    kernel, _, launches = agg.last_launch()
    assert s.engine.packer.last_row_tables["f32"] == "rows"
    assert kernel == SEGROWS_TARGETS[(SEG_KIND[wkind], op)] and launches == 1, kernel
    checks.append(("w_glob", _join(got), want))
    for name, a, b in checks:
        _check(name, a, b)


# ---------------------------------------------------------------------------------------------
# (c) the plain mean: the divide by denom and the out32 cast next to out64
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", MODES)
def test_mean_divide_and_cast_narrow(mode, cuda, grid):
    per = 4  # windows per denom
    x, denoms = mean_columns(per * 517)
    grid(0)
    _run_windows(cuda, mode, na.OP_MEAN, x.reshape(1, -1), None, None, 517, narrow_name(mode, 0, 16),
                 variants=_variants(mode, denoms), variant_of=lambda k: k // per)


@pytest.mark.parametrize("mode", MODES[:2])
def test_mean_divide_and_cast_rowmajor(mode, cuda, grid):
    x, denoms = mean_columns(ROWMAJOR_XL)
    grid(3)
    _run_windows(cuda, mode, na.OP_MEAN, x.reshape(1, -1), None, None, ROWMAJOR_XL, rowmajor_name(mode, 0, False, 3),
                 variants=_variants(mode, denoms), variant_of=lambda k: k)
