"""CPU: tests/epilogue_table.py is a fair instrument before any GPU sees it.

On the table, for every op, both epilogue precisions and every hyper-parameter set, the C oracle
(oracle.c_update / c_update_dyn, what the GPU test compares against) agrees bit for bit with a
vectorised numpy restatement of the reference's update; not too many columns are NaN; and every
class of result the table is built to reach — subnormal results and state, overflow from finite
operands, square roots of subnormal and of negative v_t, a zero denominator, Yogi's sign 0 and
NaN — holds at least 32 columns.  The thresholds are fixed conditions on the table's design, not
measurements: if one fails, the table is adjusted, not the threshold."""
import numpy as np
import pytest

import oracle
from epilogue_table import (DYN_HYPERS, HYPERS, OPT_OPS, W64_WEIGHTS, edges, g_edges, mean_columns, same_values,
                            first_diffs, stack_for, table)

TYPES = {"f32": np.float32, "f64": np.float64}
MAX_NAN_SHARE = 0.25
MIN_CLASS = 32


@pytest.fixture(scope="module")
def tables():
    return {(t, kind): table(T, kind) for t, T in TYPES.items() for kind in ("opt", "dyn")}


# ---------------------------------------------------------------------------------------------
# the reference's update, vectorised: flearn avgm.py:19-36, opt.py:23-65, dyn.py:17-36 — the same
# ufuncs in the same order on arrays of the dtypes the reference has (w_glob in T, w_local / h
# float32, the hyper-parameters Python floats)
# ---------------------------------------------------------------------------------------------


def np_update(op, g, l32, v, beta, eta, tau, beta2):
    """Returns (new w_local, new v_t)."""
    with np.errstate(all="ignore"):
        delta = g - l32
        if op == "avgm":
            v = delta + beta * v
            return l32 + v, v
        sq = np.multiply(delta, delta)
        c = 1 - beta2  # a Python float: evaluated in double
        if op == "adagrad":
            v = v + sq
        elif op == "yogi":
            v = v - c * sq * np.sign(v - sq)
        else:
            v = beta2 * v + c * sq
        return l32 + eta * delta / (np.sqrt(v) + tau), v


def np_update_dyn(g, h32, theta, n_clients, alpha):
    """Returns (new w_glob = new theta, new h)."""
    with np.errstate(all="ignore"):
        delta = g * n_clients - theta
        h = h32.copy()
        h -= alpha / n_clients * delta  # in place on the float32 h: computed in T, stored as float32
        return g - alpha * h, h


def _assert_same(name, got, want):
    assert same_values(got, want), (name, first_diffs(got, want))


def _is_sub(a):
    return (a != 0) & (np.abs(a) < np.finfo(a.dtype).tiny)


# Classes the degenerate set (beta = 0, eta = 1, tau = 0, beta2 = 0) cannot reach whatever the table
# holds; there the count must be 0, everywhere else at least MIN_CLASS.
UNREACHABLE = {
    # v_t = d and w = l + d with d = fl(g - l): |l| < 2^128 is below half an ulp of the float64
    # maximum, so no finite g, l overflows either
    ("avgm", "f64", "degenerate", "inf from finite inputs"),
    # v_t = 0 * v_t + 1 * d*d is NaN or >= +0 (-0 + +0 = +0)
    ("adam", "f32", "degenerate", "sqrt of a negative v_t"),
    ("adam", "f64", "degenerate", "sqrt of a negative v_t"),
    # the step d / sqrt(fl(d*d)) is 0, NaN, inf or of magnitude about 1, and the float32 l widened
    # to float64 is 0 or at least 2^-149: l + step is 0 or normal
    ("adam", "f64", "degenerate", "out subnormal"),
}


def _count(name, mask, where=None):
    n = int(mask.sum())
    if where is not None and where + (name,) in UNREACHABLE:
        assert n == 0, f"{name}: listed as unreachable, yet {n} columns"
        return
    assert n >= MIN_CLASS, f"{name}: only {n} columns"


# ---------------------------------------------------------------------------------------------
# the table's shape
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("t", sorted(TYPES))
def test_edge_list(t):
    T = TYPES[t]
    fi, e = np.finfo(T), edges(T)
    assert e[0] == 0 and e[1] == fi.smallest_subnormal and e[3] < fi.tiny == e[4] and e[-2] == fi.max and np.isinf(e[-1])
    with np.errstate(all="ignore"):
        assert 0 < e[6] * e[6] < fi.tiny == e[7] * e[7] and np.isfinite(e[12] * e[12]) and np.isinf(e[13] * e[13])
    g = g_edges(T)
    assert np.isnan(g).sum() == 1 and np.signbit(g[g == 0]).sum() == 1
    assert set(np.abs(edges(T))) <= set(np.abs(g[~np.isnan(g)]))


@pytest.mark.parametrize("kind", ["opt", "dyn"])
@pytest.mark.parametrize("t", sorted(TYPES))
def test_table_parts(t, kind, tables):
    T = TYPES[t]
    tab = tables[t, kind]
    assert tab.g.dtype == T and tab.l32.dtype == np.float32 and tab.v.dtype == T
    ne = len(edges(T))
    nv = 2 * ne + 1 if kind == "dyn" else ne + 3
    assert tab.n_cross == len(g_edges(T)) * (2 * ne + 1) * nv
    assert len(tab.g) == len(tab.l32) == len(tab.v) >= tab.n_cross + 8192 + 128
    # every combination of the three edge lists is a column (NaN and the sign of zero included)
    bits = np.stack([tab.g[: tab.n_cross].astype(np.float64).view(np.int64),
                     tab.l32[: tab.n_cross].astype(np.float64).view(np.int64),
                     tab.v[: tab.n_cross].astype(np.float64).view(np.int64)])
    assert len(np.unique(bits, axis=1).T) == tab.n_cross
    ties = slice(tab.n_cross, tab.n_cross + 256)
    d = tab.g[ties] - tab.l32[ties].astype(T)
    assert (d[:128] == 0).all() and (d[128:] != 0).all() and (d[128:] * d[128:] == tab.v[ties][128:]).all()
    rnd = slice(tab.n_cross + 256, None)
    for a in (tab.g[rnd], tab.l32[rnd], tab.v[rnd]):
        ex = np.frexp(a)[1]
        fi = np.finfo(a.dtype)
        assert np.isfinite(a).all() and ex.min() < fi.minexp - fi.nmant + 8 and ex.max() > fi.maxexp - 4
        assert _is_sub(a).sum() >= 100  # subnormal binades are drawn like any other
    if kind == "opt":
        assert (tab.v[rnd] >= 0).all() and (tab.g[rnd] < 0).any() and (tab.l32[rnd] < 0).any()
    # a longer table has the shorter one as its prefix
    longer = table(T, kind, pad_to=517)
    assert len(longer.g) % 517 == 0
    for a, b in zip(tab[:3], longer[:3]):
        assert same_values(a[: tab.n_cross + 256], b[: tab.n_cross + 256])


def test_stack_mapping():
    g = g_edges(np.float64)
    x, w, denom = stack_for(g, n=8)
    assert x.shape == (8, len(g)) and x.dtype == np.float32 and denom == 1.0 and (w == 1).all()
    assert (x[1:] == 0).all() and not np.signbit(x[1:]).any()
    g32 = g_edges(np.float32)
    assert same_values(stack_for(g32)[0][0], g32)  # float32 values pass unchanged
    # a float64 weight carries the sum past both ends of the float32 range
    x1 = np.float64(x[0])
    with np.errstate(all="ignore"):
        assert (np.isfinite(x1 * W64_WEIGHTS[1]) & (np.abs(x1 * W64_WEIGHTS[1]) > np.finfo(np.float32).max)).any()
        small = np.abs(x1 * W64_WEIGHTS[2])
        assert ((small > 0) & (small < np.finfo(np.float64).tiny)).any()


# ---------------------------------------------------------------------------------------------
# oracle agreement and the fixed conditions
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hyper", sorted(HYPERS))
@pytest.mark.parametrize("t", sorted(TYPES))
@pytest.mark.parametrize("op", OPT_OPS)
def test_oracle_agrees_with_numpy_and_classes_are_reached(op, t, hyper, tables):
    tab = tables[t, "opt"]
    hy = HYPERS[hyper]
    where = (op, t, hyper)
    v_c = tab.v.copy()
    out_c = oracle.c_update(op, tab.g, tab.l32, v_c, **hy)
    out_n, v_n = np_update(op, tab.g, tab.l32, tab.v, **hy)
    assert out_n.dtype == tab.g.dtype and v_n.dtype == tab.g.dtype
    _assert_same("out", out_c, out_n)
    _assert_same("v_t", v_c, v_n)

    assert np.isnan(out_c).mean() <= MAX_NAN_SHARE, np.isnan(out_c).mean()
    finite_in = np.isfinite(tab.g) & np.isfinite(tab.l32) & np.isfinite(tab.v)
    _count("out subnormal", _is_sub(out_c), where)
    _count("state subnormal", _is_sub(v_c), where)
    _count("inf from finite inputs", finite_in & (np.isinf(out_c) | np.isinf(v_c)), where)
    if op != "avgm":
        _count("sqrt of a subnormal v_t", _is_sub(v_c), where)
        _count("sqrt of a negative v_t", v_c < 0, where)
        if hyper == "degenerate":
            with np.errstate(all="ignore"):
                _count("denominator exactly 0", np.sqrt(v_c) + tab.g.dtype.type(hy["tau"]) == 0, where)
    if op == "yogi":
        with np.errstate(all="ignore"):
            d = tab.g - tab.l32
            s = tab.v - d * d
        _count("yogi sign 0", s == 0, where)
        _count("yogi sign NaN", np.isnan(s), where)


@pytest.mark.parametrize("alpha,n_clients", DYN_HYPERS)
@pytest.mark.parametrize("t", sorted(TYPES))
def test_dyn_oracle_agrees_with_numpy_and_classes_are_reached(t, alpha, n_clients, tables):
    tab = tables[t, "dyn"]
    h_c, th_c = tab.l32.copy(), tab.v.copy()
    out_c = oracle.c_update_dyn(tab.g, h_c, th_c, n_clients, alpha=alpha)
    out_n, h_n = np_update_dyn(tab.g, tab.l32, tab.v, n_clients, alpha)
    assert out_n.dtype == tab.g.dtype and h_n.dtype == np.float32
    _assert_same("out", out_c, out_n)
    _assert_same("theta", th_c, out_n)
    _assert_same("h", h_c, h_n)

    assert np.isnan(out_c).mean() <= MAX_NAN_SHARE, np.isnan(out_c).mean()
    finite_in = np.isfinite(tab.g) & np.isfinite(tab.l32) & np.isfinite(tab.v)
    _count("out subnormal", _is_sub(out_c))
    _count("state subnormal", _is_sub(h_c))
    _count("inf from finite inputs", finite_in & (np.isinf(out_c) | np.isinf(h_c)))


def test_mean_columns_reach_the_cast_edges():
    """The plain mean under MODE_W32_DIV64: the float64 quotient, and its float32 cast next to it."""
    x, denoms = mean_columns(2068)
    assert x.shape == (len(denoms), 2068) and x.dtype == np.float32
    out64 = np.concatenate([oracle.c_reduce(oracle.MODE_W32_DIV64, x[i : i + 1], np.ones(1, np.float32), d)
                            for i, d in enumerate(denoms)])
    with np.errstate(all="ignore"):
        want = np.concatenate([x[i].astype(np.float64) / d for i, d in enumerate(denoms)])
        out32 = out64.astype(np.float32)
    assert same_values(out64, want)
    assert _is_sub(out32).sum() >= 100
    assert (np.isinf(out32) & np.isfinite(out64)).sum() >= 100
    assert (np.isfinite(out32) & (out32.astype(np.float64) != out64)).sum() >= 100
    for mode, T in ((oracle.MODE_W32_DIV32, np.float32), (oracle.MODE_W64, np.float64)):
        for i, d in enumerate(denoms):
            with np.errstate(all="ignore"):
                want = x[i].astype(T) / T(d)
            assert same_values(oracle.c_reduce(mode, x[i : i + 1], np.ones(1, T), float(T(d))), want), (mode, d)


# ---------------------------------------------------------------------------------------------
# the oracle itself does not flush
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("t", sorted(TYPES))
def test_oracle_keeps_subnormals(t):
    """Results known in closed form: 3 x the smallest subnormal over 1, through the reduce, the
    momentum update (beta = 0: v_t = d, w = 0 + d) and FedDyn (h = 0, theta = 0: w = g - 0)."""
    T = TYPES[t]
    sub3 = T(3) * T(np.finfo(T).smallest_subnormal)
    x = np.full((1, 8), np.float32(3) * np.float32(np.finfo(np.float32).smallest_subnormal), np.float32)
    for mode in (oracle.MODE_W32_DIV64, oracle.MODE_W32_DIV32, oracle.MODE_W64):
        w = np.ones(1, np.float64 if mode == oracle.MODE_W64 else np.float32)
        out = oracle.c_reduce(mode, x, w, 1.0)
        assert (out == x[0]).all() and (out != 0).all()
    g = np.full(8, sub3, T)
    v = np.zeros(8, T)
    out = oracle.c_update("avgm", g, np.zeros(8, np.float32), v, beta=0.0)
    assert same_values(out, g) and same_values(v, g)
    v = np.zeros(8, T)
    out = oracle.c_update("adagrad", np.full(8, edges(T)[6], T), np.zeros(8, np.float32), v)
    assert (v != 0).all() and _is_sub(v).all()  # the square of 0.75 sqrt(tiny) is subnormal
    h, th = np.zeros(8, np.float32), np.zeros(8, T)
    out = oracle.c_update_dyn(g, h, th, 1, alpha=0.01)
    assert same_values(out, g) and same_values(th, g)
