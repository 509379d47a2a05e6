"""Operands carved out of one device arena so that the addresses a kernel forms lie gigabytes from
the pointer it is given (tests/test_gpu_far_addresses.py).

The arena is filled once with a NaN-pattern sentinel word.  Every operand under test starts at least
MARGIN (4 GiB) into it and ends at least MARGIN before its end, so an offset truncated to 32 bits, or
sign-extended from 32 bits, still lands inside the allocation: a narrowed address computation shows
as a mismatch, not as a fault.  Before a launch the places such a wrapped address would hit are
given finite decoy data (`Arena.stack` does it for every row window), so a wrapped read gives a wrong
finite answer and never a lucky NaN.  After the launch `Arena.settle()` puts the sentinel back over
everything the test wrote or asked a kernel to write, then scans the whole arena on the device, in
chunks: any word that is not the sentinel was written by a kernel where it had no business.

Three layouts (`far_rows`, `far_window`, `long_window`), each the smallest that makes its offset real:

  far rows     a large row stride: row i begins i * stride bytes from the stack's pointer
  far window   col_begin at least 4 GiB of bytes into each row
  long window  n_cols just over 2^30: window-relative offsets pass 4 GiB inside one launch
"""
from __future__ import annotations

import numpy as np
import torch

GIB = 1 << 30
MIB = 1 << 20
WRAP = 1 << 32
MARGIN = 4 * GIB
ARENA_BYTES = 23 * GIB
LIVE_CAP = 24 * GIB  # the arena, compact copies, outputs off the arena and torch's scan temporaries
SENTINEL = 0x7FA5A5A5  # an fp32 NaN; as a float64 pair and in its high half also a NaN
OUT_ZONE = ARENA_BYTES - MARGIN - GIB // 2  # small operands (outputs, accumulators, centres) live here
SCAN_WORDS = 64 * MIB  # words per chunk of the sentinel scan (256 MiB)

ROW_STRIDE = 2 * GIB + 64  # far rows, n = 5: row 1 starts past 2^31, row 2 past 2^32
ROW9_STRIDE = GIB + 64  # far rows, n = 9 (the split-N reduce takes 8 clients or more)
WIDE_STRIDE_130 = 112 * MIB + 64  # n = 130: row 128 (run 1's first) lies 14 GiB from row 0, 18 GiB into the arena
WIDE_STRIDE_300 = 48 * MIB + 64  # n = 300: runs 1 and 2 begin 6 GiB and 12 GiB from row 0
WINDOW_STRIDE = 4 * GIB + 16 * MIB  # far window, n = 3: every row holds a window 4 GiB into it
WINDOW_BYTES = 4 * GIB  # col_begin of a far window, in bytes
LONG_COLS = (1 << 30) + 1003  # a long window: ragged, and its last 16-B quad is partial


def skip_reason(device):
    """None when the device has room for the module, else the reason to skip it."""
    free, _total = torch.cuda.mem_get_info(device)
    need = LIVE_CAP + 4 * GIB
    return None if free >= need else f"far-address tests need {need >> 30} GiB free device memory, {free >> 30} GiB are"


def wraps(x):
    """Where a 32-bit slip could take the byte offset x: truncated, sign-extended, one wrap short."""
    lo = x % WRAP
    return {lo, lo - WRAP, x - WRAP} - {x}


def wrapped_offsets(row_part, col_part):
    """The byte offsets (from the operand's pointer) a narrowed computation of row_part + col_part
    could form instead: either term wrapped, or their sum."""
    out = {row_part + c for c in wraps(col_part)} | {r + col_part for r in wraps(row_part)} | wraps(row_part + col_part)
    return out - {row_part + col_part}


class Arena:
    def __init__(self, device):
        self.device = device
        self.words = torch.empty(ARENA_BYTES // 4, dtype=torch.int32, device=device)
        self.words.fill_(SENTINEL)
        self._typed = {torch.int32: self.words}
        self._dirty = []  # (byte offset, bytes) written since the last settle()
        self._out = OUT_ZONE
        self._rng = np.random.default_rng(2024)
        torch.cuda.synchronize(device)

    def typed(self, dtype):
        if dtype not in self._typed:
            self._typed[dtype] = self.words.view(dtype)
        return self._typed[dtype]

    # -- carving -----------------------------------------------------------------------------------
    def view(self, off, dtype, shape, strides=None):
        """A tensor of `dtype` at byte offset `off` of the arena; all of it lies between the margins."""
        item = torch.empty(0, dtype=dtype).element_size()
        shape = tuple(int(s) for s in shape)
        strides = tuple(int(s) for s in strides) if strides is not None else tuple(
            int(np.prod(shape[i + 1:], dtype=np.int64)) for i in range(len(shape)))
        last = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
        assert off % item == 0 and off % 16 == 0
        assert MARGIN <= off and off + last * item <= ARENA_BYTES - MARGIN, "operand inside a margin"
        return torch.as_strided(self.typed(dtype), shape, strides, off // item)

    def mark(self, off, nbytes):
        """[off, off + nbytes) is about to be written (by the test or, as an output, by a kernel)."""
        assert 0 <= off and off + nbytes <= ARENA_BYTES
        self._dirty.append((off, nbytes))

    def write(self, off, host):
        host = np.ascontiguousarray(host)
        raw = torch.from_numpy(host.reshape(-1).view(np.uint8))
        self.mark(off, raw.numel())
        self.typed(torch.uint8)[off : off + raw.numel()].copy_(raw)

    def decoy(self, off, nbytes, np_dtype):
        """Finite data of np_dtype, unlike any operand's, over [off, off + nbytes)."""
        if off < 0 or off + nbytes > ARENA_BYTES:
            return
        dt = np.dtype(np_dtype)
        n = -(-nbytes // dt.itemsize)
        junk = self._rng.integers(-7, 8, n) * 3 + 64  # finite, away from the tests' small values
        self.write(off, junk.astype(dt).view(np.uint8)[:nbytes])

    def stack(self, host, stride_bytes, col_begin=0, base=MARGIN):
        """host [n, width] laid out as rows stride_bytes apart with the window at column col_begin:
        decoys where a wrapped row or window address would land, then the rows themselves.  Returns the
        [n, col_begin + width] tensor to hand to an entry."""
        host = np.ascontiguousarray(host)
        n, width = host.shape
        item = host.dtype.itemsize
        assert stride_bytes % item == 0 and stride_bytes >= (col_begin + width) * item
        t = self.view(base, torch.from_numpy(host[:0]).dtype, (n, col_begin + width), (stride_bytes // item, 1))
        for i in range(n):
            for rel in wrapped_offsets(i * stride_bytes, col_begin * item):
                self.decoy(base + rel, width * item, host.dtype)
        for i in range(n):
            self.write(base + i * stride_bytes + col_begin * item, host[i])
        return t

    def far_row_vector(self, host, col_begin, base):
        """A 1-D operand indexed by absolute column (a centre row): col_begin + len(host) elements
        from arena offset `base`, of which only the window is filled, decoys behind it."""
        host = np.ascontiguousarray(host)
        return self.stack(host[None, :], (col_begin + host.size) * host.dtype.itemsize, col_begin, base)[0]

    def place(self, host):
        """A small contiguous input (centre, accumulator, prev, v ...) in the output zone."""
        host = np.ascontiguousarray(host)
        t = self.out(torch.from_numpy(host.reshape(-1)[:0]).dtype, host.size)
        self.write(self._last_off, host)
        return t

    def out(self, dtype, n):
        """A 1-D output of n elements in the output zone, left on the sentinel, 4 KiB from its
        neighbours; settle() restores it and so finds any write around it."""
        item = torch.empty(0, dtype=dtype).element_size()
        off = self._out
        self._out = -(-(off + n * item + 4096) // 256) * 256
        assert self._out <= ARENA_BYTES - MARGIN, "output zone full"
        self._last_off = off
        self.mark(off, n * item)
        return self.view(off, dtype, (n,))

    # -- after the launch --------------------------------------------------------------------------
    def restore(self):
        """Put the sentinel back over everything marked."""
        for off, nbytes in self._dirty:
            self.words[off // 4 : -(-(off + nbytes) // 4)].fill_(SENTINEL)
        self._dirty = []
        self._out = OUT_ZONE

    def settle(self):
        """restore(), then the number of arena words that are not the sentinel: writes no test asked for."""
        torch.cuda.synchronize(self.device)
        self.restore()
        bad = torch.zeros((), dtype=torch.int64, device=self.device)
        for w0 in range(0, self.words.numel(), SCAN_WORDS):
            bad += (self.words[w0 : w0 + SCAN_WORDS] != SENTINEL).sum()
        return int(bad)


def far_rows(arena, host, stride_bytes=ROW_STRIDE, base=MARGIN):
    """(stack tensor, col_begin = 0)."""
    return arena.stack(host, stride_bytes, 0, base), 0


def far_window(arena, host, extra_cols=0, base=MARGIN, window_bytes=WINDOW_BYTES):
    """(stack tensor, col_begin): the window window_bytes (+ extra_cols elements) into each of the rows.
    For nibble-packed rows the caller scales col_begin by its columns per byte."""
    item = np.asarray(host).dtype.itemsize
    col_begin = window_bytes // item + extra_cols
    return arena.stack(host, WINDOW_STRIDE, col_begin, base), col_begin


def same_bits(got, want):
    """Bit equality, NaN exactly where the reference has NaN (payloads free)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return got.tobytes() == want.tobytes()
    nan = np.isnan(want)
    iv = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.isnan(got[nan]).all() and (got[~nan].view(iv) == want[~nan].view(iv)).all())
