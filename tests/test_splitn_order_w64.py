"""The split-N order for FA_MODE_W64 (oracle.c_reduce_splitn -> ora_sum_w64_splitn), on the CPU:
tests/test_gpu_instantiations.py pins reduce_kernel_splitn<AccF32W64, ...> to it bit for bit, so the
restatement itself is pinned here to a plain numpy float64 statement of the same splits, tree and
guard, and to the sequential f64 sum (oracle.c_reduce, itself pinned to the reference's fixtures)."""
import numpy as np

import oracle


def _numpy_split(x, w, splits, guard):
    n = x.shape[0]
    prod = w[:, None] * x.astype(np.float64)  # one rounding per product, as the kernel's f64 multiply
    parts, aparts = [], []
    for v in range(splits):
        r0, r1 = v * n // splits, (v + 1) * n // splits
        acc, aacc = prod[r0].copy(), np.abs(prod[r0])
        for i in range(r0 + 1, r1):
            acc = acc + prod[i]
            aacc = aacc + np.abs(prod[i])
        parts.append(acc)
        aparts.append(aacc)
    h = 1
    while h < splits:
        for v in range(0, splits - h, 2 * h):
            parts[v] = parts[v] + parts[v + h]
            aparts[v] = aparts[v] + aparts[v + h]
        h *= 2
    seq = prod[0].copy()
    for i in range(1, n):
        seq = seq + prod[i]
    s, a = parts[0], aparts[0]
    flag = ~(a <= 2.0 * np.abs(s)) | ~(np.abs(s) <= 3.0e38)
    return np.where(flag & guard, seq, s), flag


def test_w64_split_order_restatement():
    n, p = 77, 1500
    x = oracle.fill_uniform(n, p, 9)
    x[:, 300:] = np.float32(0.5) * x[:, 300:] + np.float32(1.0)  # same-sign terms: the split order stands
    x[1::2, :300] = -x[0:-1:2, :300] + np.float32(1e-4) * x[1::2, :300]  # columns that nearly cancel
    x[3, 700] = np.inf  # a non-finite sum takes the sequential order too
    w = np.random.default_rng(2).uniform(0.25, 3.0, n)
    denom = float(np.sum(w))
    seq = oracle.c_reduce(oracle.MODE_W64, x, w, denom)
    assert np.array_equal(oracle.c_reduce_splitn(oracle.MODE_W64, x, w, denom, splits=1, guard=False), seq)
    for guard in (True, False):
        want, flag = _numpy_split(x, w, 4, guard)
        got = oracle.c_reduce_splitn(oracle.MODE_W64, x, w, denom, guard=guard)
        assert got.dtype == np.float64 and (got.tobytes() == (want / denom).tobytes())
    assert flag[:300].all() and flag[700] and not flag[300:700].any() and not flag[701:].any()
    assert (oracle.c_reduce_splitn(oracle.MODE_W64, x, w, denom)[701:] != seq[701:]).any()  # a different order
    guarded = oracle.c_reduce_splitn(oracle.MODE_W64, x, w, denom)
    assert np.array_equal(guarded[flag], seq[flag])
