"""rt_unique_count, rt_unique_write and rt_searchsorted validate their
arguments on the host before any HIP call; runs without a GPU: every call
here fails validation, has a zero extent or is host arithmetic."""

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
I4 = (ctypes.c_int64 * 4)


def count(lib, keys=P, n=4, dtype=2, scratch=P, nbytes=1 << 30, nu=True):
    return lib.rt_unique_count(0, keys, n, dtype, scratch, nbytes,
                               ctypes.byref(ctypes.c_int64()) if nu else None)


def write(lib, keys=P, n=4, dtype=2, scratch=P, out=P):
    return lib.rt_unique_write(0, keys, None, n, dtype, scratch, out, None,
                               None)


def search(lib, v=P, m=4, x=P, nd=1, shape=(4,), strides=(1,), dtype=2,
           side=0, out=P):
    return lib.rt_searchsorted(0, v, m, x, 0, nd,
                               I4(*shape) if shape is not None else None,
                               I4(*strides) if strides is not None else None,
                               dtype, side, out)


REJECTED = [
    (count, dict(dtype=-1), "bad dtype"), (count, dict(dtype=7), "bad dtype"),
    (count, dict(n=-1), "negative n"), (count, dict(n=1 << 40), "out of range"),
    (count, dict(keys=None), "NULL keys"),
    (count, dict(scratch=None), "NULL scratch"),
    (count, dict(scratch=ODD), "not 16-byte aligned"),
    (count, dict(nbytes=8), "scratch_bytes too small"),
    (count, dict(nu=False), "NULL n_unique"),
    (write, dict(dtype=7), "bad dtype"), (write, dict(n=-1), "negative n"),
    (write, dict(n=1 << 40), "out of range"),
    (write, dict(keys=None), "NULL keys"),
    (write, dict(scratch=None), "NULL scratch"),
    (write, dict(scratch=ODD), "not 16-byte aligned"),
    (write, dict(out=None), "NULL out_keys, out_first and out_counts"),
    (search, dict(nd=0), "nd out of range"), (search, dict(nd=5), "nd out of"),
    (search, dict(shape=None), "NULL shape"),
    (search, dict(strides=None), "NULL strides"),
    (search, dict(shape=(-1,)), "negative extent"),
    (search, dict(shape=(1 << 40,)), "out of range"),
    (search, dict(dtype=7), "bad dtype"), (search, dict(side=2), "bad side"),
    (search, dict(m=-1), "negative m"), (search, dict(m=1 << 40), "m out of"),
    (search, dict(v=None), "NULL v"), (search, dict(x=None), "NULL x"),
    (search, dict(out=None), "NULL out"),
]


@pytest.mark.parametrize("fn,kw,what", REJECTED)
def test_rejected_argument_is_named(lib, fn, kw, what):
    rc = fn(lib, **kw)
    msg = lib.rt_last_error().decode()
    who = {count: "rt_unique_count:", write: "rt_unique_write:",
           search: "rt_searchsorted:"}[fn]
    assert rc != 0, f"{who} accepted a call that should fail on {what!r}"
    assert msg.startswith(who) and what in msg, msg


def test_zero_extent_returns_without_launching(lib):
    nu = ctypes.c_int64(-1)
    assert lib.rt_unique_count(0, None, 0, 2, None, 0, ctypes.byref(nu)) == 0
    assert nu.value == 0
    assert write(lib, n=0, keys=None, scratch=None, out=None) == 0
    assert search(lib, shape=(0,), x=None, out=None) == 0
    assert search(lib, nd=2, shape=(3, 0), strides=(0, 1), x=None) == 0


def test_scratch_and_geometry_are_host_arithmetic(lib):
    from ramba_amd.hip_backend import searchsorted_geometry, unique_geometry
    need = lib.rt_unique_scratch
    assert [need(-1), need(1 << 40)] == [-1, -1]
    sizes = [need(n) for n in (0, 1, 4097, 10 ** 6, 1 << 30, (1 << 40) - 1)]
    assert sizes == sorted(sizes) and sizes[-1] <= 1 << 16
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert count(lib, n=10 ** 6, nbytes=need(10 ** 6) - 1) != 0
    u = unique_geometry(lib)
    assert u["block"] == 256 and u["tile"] == 256 * u["keys_per_lane"]
    assert u["keys_per_lane"] % 16 == 0 and u["grid_cap"] >= 1
    s = searchsorted_geometry(lib)
    assert s["block"] == 256 and s["grid_cap"] >= 1
    assert s["fence"] & (s["fence"] - 1) == 0 and s["fence"] >= 64
    # all of v for two blocks a CU: at most 80 KB of LDS each
    assert all(s["fence"] < n and n * w <= 80 * 1024
               for w, n in s["lds_max"].items())
