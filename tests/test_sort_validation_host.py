"""The rt_sort family validates its arguments on the host before any HIP
call; runs without a GPU: every call here fails validation, has a zero
extent or is host arithmetic."""

import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.skip("libramba_rt.so not built")
    return hip_backend._load_lib()


P = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)  # never read
ODD = ctypes.c_void_p(P.value + 4)


def sort(lib, in_=P, out=P, n=4, dtype=2, scratch=P, nbytes=1 << 30):
    return lib.rt_sort(0, in_, out, None, 0, None, n, dtype, scratch, nbytes,
                       None)


def lines(lib, in_=P, nlines=4, length=4, dtype=2, keys=P, pos=None):
    return lib.rt_sort_lines(0, in_, 0, nlines, length, length, 1, dtype,
                             keys, pos)


def bounds(lib, run=P, n=4, dtype=2, spl=P, m=2, out=P):
    return lib.rt_sort_bounds(0, run, n, dtype, spl, m, out)


REJECTED = [
    (sort, dict(dtype=-1), "bad dtype"), (sort, dict(dtype=7), "bad dtype"),
    (sort, dict(n=-1), "negative n"), (sort, dict(n=1 << 40), "out of range"),
    (sort, dict(in_=None), "NULL in"), (sort, dict(out=None), "NULL out"),
    (sort, dict(scratch=None), "NULL scratch"),
    (sort, dict(scratch=ODD), "not 16-byte aligned"),
    (sort, dict(nbytes=100), "scratch_bytes too small"),
    (lines, dict(dtype=9), "bad dtype"),
    (lines, dict(nlines=-1), "negative nlines"),
    (lines, dict(length=-1), "negative len"),
    (lines, dict(nlines=1 << 40), "nlines out of range"),
    (lines, dict(length=1 << 20), "len exceeds line_max"),
    (lines, dict(nlines=1 << 39, length=1 << 10), "too large"),
    (lines, dict(in_=None), "NULL in"),
    (lines, dict(keys=None), "NULL out_keys and out_pos"),
    (bounds, dict(dtype=7), "bad dtype"), (bounds, dict(n=-1), "n out of"),
    (bounds, dict(m=-1), "m out of"), (bounds, dict(run=None), "NULL run"),
    (bounds, dict(spl=None), "NULL splitters"),
    (bounds, dict(out=None), "NULL bounds"),
]


@pytest.mark.parametrize("fn,kw,what", REJECTED)
def test_rejected_argument_is_named(lib, fn, kw, what):
    rc = fn(lib, **kw)
    msg = lib.rt_last_error().decode()
    who = {sort: "rt_sort:", lines: "rt_sort_lines:",
           bounds: "rt_sort_bounds:"}[fn]
    assert rc != 0, f"{who} accepted a call that should fail on {what!r}"
    assert msg.startswith(who) and what in msg, msg


def test_zero_extent_returns_without_launching(lib):
    assert sort(lib, n=0, in_=None, out=None, scratch=None, nbytes=0) == 0
    assert lines(lib, nlines=0, in_=None, keys=None) == 0
    assert lines(lib, length=0, in_=None, keys=None) == 0
    assert bounds(lib, m=0, spl=None, out=None) == 0


def test_scratch_is_monotone_sufficient_and_small(lib):
    need = lib.rt_sort_scratch
    assert [need(-1, 2, 0), need(1 << 40, 2, 0), need(4, 7, 0)] == [-1] * 3
    for dtype, size in ((0, 8), (1, 4), (4, 2), (6, 1)):
        last = 0
        for n in (0, 1, 2047, 2048, 2049, 10 ** 6, 1 << 26, 1 << 32):
            keys, pay = need(n, dtype, 0), need(n, dtype, 1)
            assert keys >= last and pay >= keys + 8 * n
            last = keys
            # one copy of the keys, and counters that stay a small fraction
            assert n * size <= keys <= n * size + (8 << 20)
            assert sort(lib, n=max(n, 1), dtype=dtype,
                        nbytes=need(max(n, 1), dtype, 0) - 1) != 0


def test_geometry_is_sane(lib):
    from ramba_amd.hip_backend import sort_geometry
    g = sort_geometry(lib)
    assert g["block"] == 256 and g["wave_max"] == 64
    assert g["tile"] == g["block"] * g["keys_per_lane"] >= g["block"]
    assert g["grid_cap"] >= 1 and g["lines_per_launch"] >= 1
    assert sorted(g["line_max"]) == [1, 2, 4, 8]
    assert all(2048 <= v < 65536 for v in g["line_max"].values())
