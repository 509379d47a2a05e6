"""Host-only: fa_last_error is one object per thread for the whole library.

The C ABI is compiled as several units (flearn_amd/_build.py SOURCES) that share their error state
through fa_host.hpp.  One entry of each group is called with arguments it refuses before touching a
device — the stack reduce, the row-pointer plan, the trimmed sum (the streamed group) and the plain
copy — and fa_last_error, which lives in one unit, must hold that entry's own message each time.  A
copy of the state per unit would leave every entry outside fa_last_error's unit reporting a stale
or empty text.  The same from a second thread, which must not disturb the first thread's message."""
import ctypes
import threading

import pytest

from flearn_amd import _native as na
from test_cabi import FAKE, header_define


@pytest.fixture(scope="module")
def L():
    return na.load()


def refused_calls(L):
    """(entry, call, expected return code, the entry's message), one per entry group."""
    cnt, grid = ctypes.c_int64(), ctypes.c_int32()
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")
    return [
        ("fa_reduce_f32", lambda: L.fa_reduce_f32(FAKE, 64, 0, 0, FAKE, 1.0, 0, 64, None, FAKE, None, None),
         arg, b"n_clients must be >= 1"),
        ("fa_rows_plan", lambda: L.fa_rows_plan(0, None, None, 99, 0, None, 0, ctypes.byref(cnt), ctypes.byref(grid)),
         arg, b"unknown epilogue op"),
        ("fa_trim_sum", lambda: L.fa_trim_sum(na.ACC_F32, FAKE, 64, 2, 1, FAKE, 0, 64, None),
         arg, b"trim must satisfy 0 <= 2 * trim < n_clients"),
        ("fa_copy", lambda: L.fa_copy(FAKE + 8, FAKE, 16, None),
         align, b"copy pointers must be 16-byte aligned"),
    ]


def check_every_entry(L):
    for name, call, code, message in refused_calls(L):
        assert call() == code, name
        assert L.fa_last_error() == message, name


def test_every_unit_writes_the_error_fa_last_error_reads(L):
    check_every_entry(L)


def test_the_error_is_per_thread_across_units(L):
    name, call, code, message = refused_calls(L)[1]  # an entry outside fa_last_error's own unit
    assert call() == code and L.fa_last_error() == message
    failures = []

    def other_thread():
        try:
            assert L.fa_last_error() == b""  # a fresh thread has no error yet
            check_every_entry(L)
        except BaseException as e:  # reported by the test's own thread
            failures.append(e)

    t = threading.Thread(target=other_thread)
    t.start()
    t.join()
    assert not failures, failures
    assert L.fa_last_error() == message, "another thread's errors replaced this thread's message"
