"""The sparse round's arithmetic in plain numpy fp32, row by row: per column
acc = init, then for the rows in list order that hold an entry (c, v): acc = fl32(acc + fl32(a_i * v)).
Rows are (columns uint32 ascending, values float32); columns are the bucket's."""
import numpy as np

F32 = np.float32


def fold(rows, weights, n_cols, col_begin=0, center=None, wsum=0.0, acc_in=None):
    """acc[c] for the window [col_begin, +n_cols): init is acc_in, else fl32(wsum * center[col_begin + c]),
    else +0.0; entries outside the window are dropped."""
    if acc_in is not None:
        acc = np.array(acc_in[:n_cols], dtype=F32)
    elif center is not None:
        acc = F32(wsum) * np.asarray(center, dtype=F32)[col_begin : col_begin + n_cols]
    else:
        acc = np.zeros(n_cols, F32)
    with np.errstate(all="ignore"):
        for (cols, vals), a in zip(rows, weights):
            rel = np.asarray(cols).astype(np.int64) - col_begin
            m = (rel >= 0) & (rel < n_cols)
            acc[rel[m]] = acc[rel[m]] + F32(a) * np.asarray(vals, dtype=F32)[m]  # a row's columns are distinct
    return acc


def pairs(rows, kstride=None):
    """The device layout: uint32 [N][kstride][2] of (column, bit pattern), rows padded with (0xFFFFFFFF, 0);
    kstride the largest count made even (at least 2)."""
    k = max(2, (max(len(c) for c, _ in rows) + 1) & ~1) if kstride is None else kstride
    out = np.zeros((len(rows), k, 2), np.uint32)
    out[:, :, 0] = 0xFFFFFFFF
    for r, (cols, vals) in enumerate(rows):
        out[r, : len(cols), 0] = cols
        out[r, : len(cols), 1] = np.asarray(vals, dtype=F32).view(np.uint32)
    return out


def same_bits(a, b):
    """Equal bit for bit; a NaN matches any NaN (only a NaN's bits are free)."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and (a.view(np.uint32)[~nan] == b.view(np.uint32)[~nan]).all()
