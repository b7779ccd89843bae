"""rt_hist validates its arguments on the host before any HIP call; runs
without a GPU: every call here fails validation or has a zero extent."""

import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.skip("libramba_rt.so not built")
    return hip_backend._load_lib()


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


P = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)  # never read
ONES = i64(1, 1, 1, 1)

NULL64 = ctypes.POINTER(ctypes.c_int64)()
REJECTED = [
    (dict(nd=0), "nd out of range"), (dict(nd=5), "nd out of range"),
    (dict(shp=NULL64), "NULL shape"), (dict(strides=None), "NULL strides"),
    (dict(shape=(-1,)), "negative extent"),
    (dict(shape=(1 << 40,)), "out of range"),
    (dict(nd=2, shape=(1 << 39, 1 << 39)), "shape too large"),
    (dict(dtype=-1), "bad dtype"), (dict(dtype=7), "bad dtype"),
    (dict(mode=-1), "bad mode"), (dict(mode=3), "bad mode"),
    (dict(mode=0, dtype=0), "INDEX mode needs an integer dtype"),
    (dict(mode=0, dtype=1), "INDEX mode needs an integer dtype"),
    (dict(nbins=0), "nbins < 1"), (dict(nbins=-5), "nbins < 1"),
    (dict(nbins=1 << 40), "nbins out of range"),
    (dict(mode=1, edges=None), "NULL edges"),
    (dict(mode=2, edges=None), "NULL edges"),
    (dict(mode=1, edt=2), "bad edges dtype"),
    (dict(mode=2, edt=1), "bad edges dtype"),
    (dict(in_=None), "NULL in"), (dict(counts=None), "NULL counts"),
]


def call(lib, nd=1, shape=(4,), shp=None, strides=ONES, dtype=2, mode=0,
         edges=P, edt=0, nbins=4, in_=P, counts=P):
    return lib.rt_hist(0, in_, 0, nd, i64(*shape) if shp is None else shp,
                       strides, dtype, mode, edges, edt, nbins, counts, None)


@pytest.mark.parametrize("kw,what", REJECTED)
def test_rejected_argument_is_named(lib, kw, what):
    rc = call(lib, **kw)
    msg = lib.rt_last_error().decode()
    assert rc != 0, f"rt_hist accepted a call that should fail on {what!r}"
    assert msg.startswith("rt_hist:") and what in msg, msg


def test_zero_extent_returns_without_launching(lib):
    assert call(lib, shape=(0,), in_=None, counts=None) == 0
    assert call(lib, nd=3, shape=(3, 0, 1 << 39), mode=2, in_=None) == 0


def test_regime_and_geometry_agree_at_the_thresholds(lib):
    from ramba_amd.hip_backend import hist_geometry
    g = hist_geometry(lib)
    assert g["block"] == 256 and g["grid_cap"] >= 1
    assert 1 <= g["wave_max_bins"] < g["block_max_bins"]
    regime = lib.rt_hist_regime
    assert [regime(n) for n in (1, g["wave_max_bins"])] == [0, 0]
    assert [regime(n) for n in (g["wave_max_bins"] + 1,
                                g["block_max_bins"])] == [1, 1]
    assert [regime(n) for n in (g["block_max_bins"] + 1, 10 ** 7)] == [2, 2]
    assert [regime(n) for n in (0, -1, 1 << 40)] == [-1, -1, -1]
