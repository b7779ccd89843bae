"""sort / argsort on the HIP backend: every regime of rt_sort and
rt_sort_lines against numpy.sort / numpy.argsort with kind="stable", through
the public functions, with the host fallback taken away.  Sorted values are
compared by their bits, so zero signs and NaN payloads count."""

import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "bool"]
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):      # reaching HostSort is a TypeError
    mod = importlib.import_module("ramba_amd.sorting")
    for hook in ("sort_lines", "sort_run", "local_run", "sort_bounds"):
        monkeypatch.setattr(mod.HostSort, hook, None)


@pytest.fixture(scope="module")
def geo():
    from ramba_amd import hip_backend as hb
    return hb.sort_geometry(hb._load_lib())


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(UINT[x.dtype.itemsize])


def check(ra, host, view=lambda x: x, axis=-1):
    a, h = view(ra.fromarray(host)), view(host)
    got, ref = ra.sort(a, axis=axis).asarray(), np.sort(h, axis=axis,
                                                        kind="stable")
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert np.array_equal(bits(got), bits(ref)), (host.dtype, h.shape, axis)
    got = ra.argsort(a, axis=axis).asarray()
    ref = np.argsort(h, axis=axis, kind="stable")
    assert got.dtype == np.int64 and got.shape == ref.shape
    assert np.array_equal(got, ref), (host.dtype, h.shape, axis)


def ties(shape, dtype):     # five distinct values with negatives; bool 0 / 1
    k = np.arange(int(np.prod(shape))) * 7 // 3
    return (k % 2 if dtype == "bool" else k % 5 - 2).astype(dtype) \
        .reshape(shape)


def hostile(dtype, n):
    """Hostile values of `dtype`, cycled with a period that is odd, so they
    fall on both sides of every wave and tile boundary."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        quiet = {4: 0x7fc00000, 8: 0x7ff8000000000000}[dt.itemsize]
        sign = 1 << (8 * dt.itemsize - 1)
        nans = np.array([quiet, quiet | sign, quiet | 0x123,
                         quiet | sign | 0x456],
                        dtype=UINT[dt.itemsize]).view(dt)
        fi = np.finfo(dt)
        vals = np.concatenate([nans, np.array(
            [np.inf, -np.inf, 0.0, -0.0, fi.smallest_subnormal,
             -fi.smallest_subnormal, 1.0, fi.max, -fi.max], dtype=dt)])
    else:
        info = np.iinfo(dt)
        vals = np.array([info.min, info.max, -1, 0, 0, info.max, info.min],
                        dtype=dt)
    return np.resize(vals, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ["1", "2", "63", "64", "65", "lm-1", "lm",
                               "lm+1", "tile-1", "tile", "tile+1",
                               "2*tile+3", "3*tile"])
def test_sizes_and_dtypes_1d(ra_gpu, geo, n, dtype):
    n = eval(n, {"lm": geo["line_max"][np.dtype(dtype).itemsize],
                 "tile": geo["tile"]})
    check(ra_gpu, ties(n, dtype))


@pytest.mark.parametrize("case", ["int64-all-bytes", "float64-all-bytes",
                                  "constant", "byte0", "byte3", "three-bytes",
                                  "int16-high-byte"])
def test_every_pass_and_pass_skipping(ra_gpu, geo, case):
    n = 2 * geo["tile"] + 3
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + (
        rng.integers(0, 2, n, dtype=np.uint64))
    small = rng.integers(0, 256, n)
    host = {"int64-all-bytes": raw.view(np.int64),
            "float64-all-bytes": raw.view(np.float64),
            "constant": np.full(n, -7, dtype=np.int32),   # no pass: a copy
            "byte0": small.astype(np.int32),              # one pass
            "byte3": (small << 24).astype(np.int64),      # one pass, not first
            "three-bytes": rng.integers(0, 1 << 24, n),   # odd: ping-pong
            "int16-high-byte": ((small - 128) << 8).astype(np.int16)}[case]
    check(ra_gpu, host)


@pytest.mark.parametrize("dtype", DTYPES[:6])
@pytest.mark.parametrize("n", ["64", "100", "2*tile+3"])
def test_hostile_values(ra_gpu, geo, n, dtype):
    check(ra_gpu, hostile(dtype, eval(n, {"tile": geo["tile"]})))


def test_two_tiles_per_block_and_a_ragged_tail(ra_gpu, geo):
    # the capped grid of rt_sort: every block walks two tiles, the last one a
    # full tile and five keys
    n = (2 * geo["grid_cap"] - 1) * geo["tile"] + 5
    check(ra_gpu, ties(n, "int16"))


def test_more_lines_than_one_launch_takes(ra_gpu, geo):
    check(ra_gpu, ties((geo["lines_per_launch"] + 5, 2), "int8"))


@pytest.mark.parametrize("dtype", ["float64", "float32", "int16", "bool"])
@pytest.mark.parametrize("length", ["1", "2", "3", "63", "64", "65", "100",
                                    "lm-1", "lm", "lm+1"])
def test_lines(ra_gpu, geo, length, dtype):
    length = eval(length, {"lm": geo["line_max"][np.dtype(dtype).itemsize]})
    rng = np.random.default_rng(length)
    for nlines in (1, 4, 5, 257) if length <= geo["wave_max"] else (1, 3):
        host = rng.integers(-3, 4, (nlines, length)).astype(dtype)
        if host.dtype.kind == "f":
            host[rng.random(host.shape) < 0.1] = np.nan
        check(ra_gpu, host)


@pytest.mark.parametrize("dtype", ["float64", "float32", "int16", "bool"])
def test_axes_and_views(ra_gpu, dtype):
    host = ties((3, 5, 70), dtype)
    for axis in (0, 1, 2, -2, None):
        check(ra_gpu, host, axis=axis)
    flat, mat = ties(301, dtype), ties((41, 67), dtype)
    check(ra_gpu, flat, lambda x: x[::-1])
    check(ra_gpu, flat, lambda x: x[1::3])
    for axis in (0, 1):
        check(ra_gpu, mat, lambda x: x.T, axis=axis)
        check(ra_gpu, mat, lambda x: x[3:30, 5:66], axis=axis)


def test_argsort_take_and_in_place_agree_with_sort(ra_gpu):
    host = ties(5000, "float32")
    host[::7] = np.nan
    a = ra_gpu.fromarray(host)
    ref = bits(np.sort(host, kind="stable"))
    assert np.array_equal(bits(a[ra_gpu.argsort(a)].asarray()), ref)
    a.sort()
    assert np.array_equal(bits(a.asarray()), ref)
