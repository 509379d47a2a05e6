"""The value table of tests/test_gpu_epilogue_values.py: operands that drive the fused epilogues
(the divide by sum(a), d*d, the square root, the second divide, the stores' casts) over the whole
exponent range of the epilogue precision T and through the IEEE special values.

A plain numpy module (no torch, no GPU).  tests/test_epilogue_table.py shows on a CPU box that the
table is a fair instrument: the C oracle agrees with a numpy restatement of the reference on it,
not too many columns are NaN, and every class of result the table is meant to reach is reached.

A table is aligned column arrays: g (the mean, in T), l32 (float32: the previous global model, or
FedDyn's h) and v (T: v_t, or FedDyn's theta).  Its parts, in order:
  cross    the cross product of the edge lists below (n_cross columns);
  d = 0    g == l32 exactly;
  sign 0   v == d*d exactly, d = g - l32 with four mantissa bits (Yogi's sign is 0);
  random   full-width mantissas, binades uniform over the whole range of the type (subnormal
           binades included), random signs for g and l32, v >= 0.  Last, so that a longer table
           (pad_to: a launch shape) has the shorter one as its prefix.

The standalone update takes g as it is (`glob`).  A fused kernel forms g from a float32 stack:
stack_for() maps the wanted g to (x, w, denom) with n = 1, w = [1], denom = 1, so the mean is
fl32(g) widened to T — exactly g where T is float32, and where T is float64 the float32 edges of
G(T) plus what the float64 ones round to.  Under MODE_W64 the weight is float64, and W64_WEIGHTS
lists weights that carry w*x past the float32 range in both directions (denom stays 1).
"""
from collections import namedtuple

import numpy as np

from instantiation_cases import NONDEFAULT

DEFAULT = dict(beta=0.9, eta=1e-1, tau=1e-9, beta2=0.99)  # avgm.py:19, opt.py:24-27
DEGENERATE = dict(beta=0.0, eta=1.0, tau=0.0, beta2=0.0)
HYPERS = {"default": DEFAULT, "nondefault": dict(NONDEFAULT), "degenerate": DEGENERATE}
DYN_HYPERS = tuple((alpha, n) for alpha in (0.01, 0.5) for n in (1, 7))  # (alpha, n_clients)
OPT_OPS = ("avgm", "adagrad", "yogi", "adam")

# MODE_W64 (float64 weight, float64 sum): 1, and two that carry w*x beyond the float32 range
W64_WEIGHTS = (1.0, 2.0 ** 900, 2.0 ** -960)
MEAN_DENOMS = (1.0, 3.0, 2.0 ** 20, 2.0 ** -20, 1e-30, 1e30)

N_RANDOM = 8192
N_TIES = 128

Table = namedtuple("Table", "g l32 v n_cross")


def edges(T):
    """E(T): 17 magnitudes from 0 to inf — the subnormals, around tiny, where the square
    underflows (0.75 sqrt(tiny): a subnormal square; sqrt(tiny): exactly tiny), around 1, where the
    square overflows, around max."""
    fi = np.finfo(T)
    t = fi.dtype.type
    sub, tiny, big = t(fi.smallest_subnormal), t(fi.tiny), t(fi.max)
    with np.errstate(all="ignore"):
        e = [t(0), sub, t(3) * sub, np.nextafter(tiny, t(0)), tiny, t(1.5) * tiny, t(0.75) * np.sqrt(tiny), np.sqrt(tiny),
             t(fi.eps),
             t(1) - t(fi.epsneg), t(1), t(1.5), t(0.99) * np.sqrt(big), t(1.01) * np.sqrt(big), big / t(2), big,
             t(np.inf)]
    e = np.array(e, dtype=t)
    assert len(e) == 17 and (np.diff(e) > 0).all()
    return e


def signed(mags):
    """+-mags plus NaN (-0.0 included)."""
    return np.concatenate([mags, -mags, np.array([np.nan], mags.dtype)])


def g_edges(T):
    """G(T): +-E(T) plus NaN; for float64 the float32 edges too (what a float32 stack can hold,
    and where g meets the float32 operand)."""
    mags = edges(T)
    if np.dtype(T) == np.float64:
        mags = np.unique(np.concatenate([mags, edges(np.float32).astype(np.float64)]))
    return signed(mags)


def v_edges(T, kind):
    """v_t: E(T) plus -0.0, -1 and NaN (a restored foreign state); theta: +-E(T) plus NaN."""
    if kind == "dyn":
        return signed(edges(T))
    return np.concatenate([edges(T), np.array([-0.0, -1.0, np.nan], np.dtype(T))])


def log_uniform(rng, T, n, signs=True):
    """n values of T: the binade uniform over [smallest subnormal, max], the mantissa full width
    (cut to the subnormal grid below tiny), the sign random or +."""
    fi = np.finfo(T)
    t = fi.dtype.type
    k = rng.integers(fi.minexp - fi.nmant, fi.maxexp, n)
    m = rng.integers(0, 1 << fi.nmant, n, dtype=np.int64)
    frac = (t(1) + m.astype(t) / t(1 << fi.nmant)).astype(t)  # exact: nmant bits
    x = np.ldexp(frac, k.astype(np.int32)).astype(t)
    if signs:
        x = np.where(rng.integers(0, 2, n) == 1, -x, x).astype(t)
    assert np.isfinite(x).all()
    return x


def _ties(rng, T, n):
    """(d = 0 columns, sign-0 columns), each (g, l32, v)."""
    t = np.dtype(T).type
    l0 = log_uniform(rng, np.float32, n)
    zero = (l0.astype(t), l0, log_uniform(rng, T, n, signs=False))
    # d = r * 2^e, r odd below 16; l = q * 2^e, |q| <= 8: g = (q + r) * 2^e and d*d = r*r * 2^(2e)
    # are exact in float32 (and so in float64) for |e| <= 60
    e = rng.integers(-60, 61, n).astype(np.int32)
    r = (2 * rng.integers(0, 8, n) + 1) * rng.choice([-1, 1], n)
    q = rng.integers(-8, 9, n)
    l1 = np.ldexp(q.astype(np.float32), e)
    g1 = np.ldexp((q + r).astype(t), e)
    v1 = np.ldexp((r * r).astype(t), 2 * e)
    assert ((g1 - l1.astype(t)) ** 2 == v1).all()
    return zero, (g1, l1, v1)


def table(T, kind="opt", pad_to=1, rem=0, seed=2024):
    """The table for epilogue precision T; kind "opt" (AVGM / Adagrad / Yogi / Adam: l32 = prev,
    v = v_t) or "dyn" (l32 = h, v = theta).  pad_to, rem: the random part is lengthened until the
    length is rem modulo pad_to."""
    t = np.dtype(T).type
    G, L, V = g_edges(T), signed(edges(np.float32)), v_edges(T, kind)
    gi, li, vi = np.meshgrid(np.arange(len(G)), np.arange(len(L)), np.arange(len(V)), indexing="ij")
    cross = (G[gi.ravel()], L[li.ravel()], V[vi.ravel()])
    rng = np.random.default_rng(seed)
    zero, sq = _ties(rng, T, N_TIES)
    fixed = len(cross[0]) + 2 * N_TIES
    nrand = N_RANDOM + (rem - fixed - N_RANDOM) % pad_to
    rand = (log_uniform(rng, T, nrand), log_uniform(rng, np.float32, nrand),
            log_uniform(rng, T, nrand, signs=kind == "dyn"))
    g, l32, v = (np.ascontiguousarray(np.concatenate([p[i] for p in (cross, zero, sq, rand)])) for i in range(3))
    assert g.dtype == t and l32.dtype == np.float32 and v.dtype == t and len(g) % pad_to == rem % pad_to
    return Table(g, l32, v, len(cross[0]))


def stack_for(g, n=1):
    """The wanted g as a float32 client stack [n, len(g)]: row 0 = fl32(g), rows 1.. = +0.0 (the
    sum is exact in any order, up to the sign of a zero), with w = ones(n) and denom = 1."""
    with np.errstate(over="ignore", under="ignore"):
        x = np.zeros((n, len(g)), np.float32)
        x[0] = g.astype(np.float32)
    return x, np.ones(n), 1.0


def mean_columns(m, seed=7):
    """The plain mean's divide and out32 cast: for each denom of MEAN_DENOMS, m log-uniform float32
    values (n = 1, w = [1]).  Returns (x [len(MEAN_DENOMS), m], MEAN_DENOMS)."""
    rng = np.random.default_rng(seed)
    return np.stack([log_uniform(rng, np.float32, m) for _ in MEAN_DENOMS]), MEAN_DENOMS


def same_values(got, want):
    """The comparison rule: NaN exactly where `want` has NaN, every other element bit-identical
    (-0.0 is not +0.0).  Created NaNs differ in sign between SSE and the GPU, so NaN bits are free."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn)) and got[~gn].tobytes() == want[~wn].tobytes()


def first_diffs(got, want, k=6):
    """Indices of the first k columns that break same_values (for assertion messages)."""
    got, want = np.asarray(got), np.asarray(want)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(u) != want.view(u)))
    return np.flatnonzero(bad)[:k].tolist(), int(bad.sum())
