"""The numpy restatement of the robust aggregation rules (include/flearn_amd.h fa_trim_sum,
DESIGN.md section 12): what tests/test_robust_host.py pins and the GPU tests compare with, bit for bit.

For a column with client values x_0 .. x_{N-1} and a trim count t per side, 0 <= 2t < N:
  1. order by IEEE totalOrder (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN): the signed-integer
     order of k = b ^ ((b >> 31) & 0x7fffffff) on the bit pattern b (64-bit form for float64;
     int64 buffers sort as integers);
  2. drop the t smallest and the t largest;
  3. sum the kept N - 2t values in ascending order in the sum type (fp32 for fp32, float64 for
     float64, wrapping int64 for int64), the first kept value initialising the sum;
  4. divide by N - 2t: fl64(acc) / d for fp32 sums (a float64 result), acc / d for float64,
     (double)acc / d for int64.
"""
import numpy as np

_INT = {4: np.int32, 8: np.int64}
_MASK = {4: np.int32(0x7FFFFFFF), 8: np.int64(0x7FFFFFFFFFFFFFFF)}


def total_order_keys(x):
    """Signed integers whose order is the totalOrder of the float array x (an involution on bits)."""
    x = np.ascontiguousarray(x)
    it = _INT[x.dtype.itemsize]
    b = x.view(it)
    return b ^ ((b >> (8 * x.dtype.itemsize - 1)) & _MASK[x.dtype.itemsize])


def keys_to_values(k, dtype):
    it = _INT[np.dtype(dtype).itemsize]
    k = np.ascontiguousarray(k, dtype=it)
    return (k ^ ((k >> (8 * k.dtype.itemsize - 1)) & _MASK[k.dtype.itemsize])).view(dtype)


def sorted_columns(stack):
    """stack [N, ...] sorted along axis 0 by totalOrder (floats) or as integers (int64)."""
    stack = np.asarray(stack)
    if stack.dtype.kind == "f":
        return keys_to_values(np.sort(total_order_keys(stack), axis=0), stack.dtype)
    return np.sort(stack, axis=0)


def median_trim(n):
    return (n - 1) // 2


def trimmed_sum(stack, trim):
    """The accumulator fa_trim_sum makes: ranks trim .. N - trim - 1 summed in ascending order in
    the stack's own dtype (fp32 / float64 sequential sums, int64 wrapping)."""
    stack = np.asarray(stack)
    n = stack.shape[0]
    if not (isinstance(trim, (int, np.integer)) and 0 <= 2 * trim < n):
        raise ValueError(f"trim {trim!r} out of range for {n} clients")
    s = sorted_columns(stack)
    with np.errstate(all="ignore"):
        acc = s[trim].copy()
        for r in range(trim + 1, n - trim):
            acc = acc + s[r]  # numpy adds elementwise in the dtype: one rounding per step, no fma
    assert acc.dtype == stack.dtype
    return acc


def trimmed_mean(stack, trim):
    """The float64 result under output="reference": fl64(acc) / (N - 2 trim)."""
    stack = np.asarray(stack)
    acc = trimmed_sum(stack, trim)
    with np.errstate(all="ignore"):
        return acc.astype(np.float64) / np.float64(stack.shape[0] - 2 * trim)


def trimmed_mean_f32(stack, trim):
    """What output="float32" / "device" hold for an fp32 key: fl32 of the float64 quotient."""
    with np.errstate(all="ignore"):
        return trimmed_mean(stack, trim).astype(np.float32)


def median(stack):
    return trimmed_mean(stack, median_trim(np.asarray(stack).shape[0]))


def ensemble(w_local_lst, trim, keys=None):
    """The reference-typed global model of a robust round over numpy state dicts: float64 arrays
    (numpy float64 scalars for 0-d values), key order of the first upload."""
    keys = list(w_local_lst[0].keys()) if keys is None else list(keys)
    out = {}
    for k in keys:
        st = np.stack([np.asarray(w[k]) for w in w_local_lst])
        q = trimmed_mean(st, trim)
        out[k] = np.float64(q) if q.ndim == 0 else q
    return out


def same_bits(a, b):
    """Bit equality with only NaN payload / sign bits free: NaN exactly where the other has NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na_, nb = np.isnan(a), np.isnan(b)
    it = _INT[a.dtype.itemsize]
    return bool((na_ == nb).all() and (a.view(it)[~na_] == b.view(it)[~nb]).all())
