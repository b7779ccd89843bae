"""rt_partition validates its arguments on the host before any HIP call; runs
without a GPU: every call here fails validation, has a zero extent or is host
arithmetic."""

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


def part(lib, in_=P, out=P, vals_out=None, n=4, dtype=3, pivots=(5,),
         npiv=None, scratch=P, nbytes=1 << 30, counts=None):
    piv = None if pivots is None else \
        (ctypes.c_uint64 * max(len(pivots), 1))(*pivots)
    return lib.rt_partition(0, in_, out, None, 0, vals_out, n, dtype,
                            len(pivots) if npiv is None else npiv, piv,
                            scratch, nbytes, counts)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=-1), "bad dtype"), (dict(dtype=7), "bad dtype"),
    (dict(n=-1), "negative n"), (dict(n=1 << 40), "n out of range"),
    (dict(npiv=0), "npiv out of range"), (dict(npiv=9), "npiv out of range"),
    (dict(pivots=None, npiv=1), "NULL pivots"),
    (dict(pivots=(7, 3)), "not distinct and ascending"),
    (dict(pivots=(3, 3)), "not distinct and ascending"),
    (dict(pivots=(1 << 32,)), "bits above the key width"),
    (dict(pivots=(256,), dtype=6), "bits above the key width"),
    (dict(in_=None), "NULL in"), (dict(out=None), "NULL out and vals_out"),
    (dict(scratch=None), "NULL scratch"),
    (dict(scratch=ODD), "not 16-byte aligned"),
    (dict(nbytes=47), "scratch_bytes too small"),
])
def test_rejected_argument_is_named(lib, kw, what):
    rc = part(lib, **kw)
    msg = lib.rt_last_error().decode()
    assert rc != 0, f"rt_partition accepted a call that should fail on {what!r}"
    assert msg.startswith("rt_partition:") and what in msg, msg


def test_zero_extent_scratch_and_geometry(lib):
    counts = (ctypes.c_int64 * 5)(*[9] * 5)
    assert part(lib, n=0, in_=None, out=None, scratch=None, nbytes=0,
                pivots=(1, 2), counts=counts) == 0
    assert list(counts) == [0] * 5
    assert part(lib, n=0, pivots=(2, 1)) != 0       # still validated
    from ramba_amd.hip_backend import partition_geometry
    g = partition_geometry(lib)
    assert g["block"] == 256 and g["npiv_max"] == 8 and g["grid_cap"] >= 1
    assert g["tile"] == g["block"] * g["keys_per_lane"] < 1 << 16
    need = lib.rt_partition_scratch
    assert [need(-1, 1), need(1 << 40, 1), need(4, 0), need(4, 9)] == [-1] * 4
    for npiv in (1, 4, 8):
        last = 0
        for n in (1, g["tile"], g["tile"] + 1, 10 ** 6, 1 << 32):
            got = need(n, npiv)
            # two int64 per bucket and block, and the totals
            assert last <= got <= 16 * (2 * npiv + 1) * (g["grid_cap"] + 1)
            assert got % 16 == 0 and part(
                lib, n=n, pivots=tuple(range(npiv)), nbytes=got - 1) != 0
            last = got
