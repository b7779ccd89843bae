"""median / percentile / quantile on the HIP backend: every dtype, load path,
digit structure and launch schedule of rt_select_pass against NumPy with
array_equal, through the public functions, with the host fallback taken
away."""

import importlib

import numpy as np
import pytest

from hist_util import both, same

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "uint8"]
METHODS = ["linear", "lower", "higher", "nearest", "midpoint"]


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):      # reaching HostSelect is a TypeError
    mod = importlib.import_module("ramba_amd.selection")
    monkeypatch.setattr(mod.HostSelect, "select_pass", None)


@pytest.fixture(scope="module")
def geo():
    from ramba_amd import hip_backend as hb
    return hb.select_geometry(hb._load_lib())


def values(n, dtype):       # both signs, ties, every byte of the key in use
    k = np.arange(n, dtype=np.uint64) // np.uint64(2) * np.uint64(
        0x9E3779B97F4A7C15)
    if np.dtype(dtype).kind == "f":
        return ((k >> np.uint64(44)).astype(np.int64) - (1 << 19)) \
            .astype(dtype) * np.dtype(dtype).type(1.25)
    bits = 8 * np.dtype(dtype).itemsize
    return (k >> np.uint64(64 - bits)).astype(f"u{bits // 8}").view(dtype)


def check(ra, h, view=lambda np_, x: x, q=(0, 37.5, 100)):
    both(ra, "median", h, view)
    for method in METHODS:
        both(ra, "percentile", h, view, q=list(q), method=method)
    both(ra, "percentile", h, view, q=q[1])
    both(ra, "quantile", h, view, q=q[1] / 100)
    return ra.deferred.get_runtime().last_select


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, "unit-1", "unit", "unit+1", 63, 64, 65,
                               255, 256, 257])
def test_sizes_and_dtypes(ra_gpu, n, dtype):
    unit = 16 // np.dtype(dtype).itemsize       # elements per 16-byte load
    check(ra_gpu, values({"unit-1": max(1, unit - 1), "unit": unit,
                          "unit+1": unit + 1}.get(n, n), dtype))


@pytest.mark.parametrize("dtype", ["float64", "int32"])
def test_two_grid_stride_trips_both_load_paths(ra_gpu, geo, dtype):
    # every block of the capped grid gets two full grid-stride trips, half of
    # them a third, plus a ragged tail; the [1:] view is not 16-byte aligned
    per = 16 // np.dtype(dtype).itemsize
    lanes = geo["grid_cap"] * geo["block"] * 5 // 2
    h = values(lanes * per + per + 1, dtype)
    both(ra_gpu, "median", h)
    both(ra_gpu, "percentile", h, q=[1, 99])
    both(ra_gpu, "median", h[:lanes + 3], lambda np_, x: x[1:])


def keys_to(dtype, k):      # int64 patterns as values of dtype, order kept
    k = np.asarray(k, dtype=np.int64)
    return k if dtype == "int64" else \
        (k + np.float64(1.0).view(np.int64)).view(np.float64)


@pytest.mark.parametrize("dtype", ["int64", "float64"])
def test_digit_structure(ra_gpu, dtype):
    i = np.arange(1000)
    st = check(ra_gpu, keys_to(dtype, np.full(1000, 77)))
    assert not st["collected"] and st["full_passes"] == 8   # never narrows
    check(ra_gpu, keys_to(dtype, i % 2))            # the last pass decides
    check(ra_gpu, keys_to(dtype, (i % 256) << 24))  # one middle byte
    h = keys_to(dtype, i % 7 << 40)                 # ranks part at the top
    check(ra_gpu, np.concatenate([h, -h]))


@pytest.mark.parametrize("dtype", ["int64", "float64"])
@pytest.mark.parametrize("extra", [0, 1])
def test_collect_rule_at_an_eighth(ra_gpu, dtype, extra):
    # n = 4096; the median's top byte is shared by 512 (+ extra) keys that
    # differ only in their lowest byte, so the candidates entering the second
    # pass, and every later one, are n / 8 (+ 1)
    mid = keys_to(dtype, np.arange(512 + extra) % 256)
    lo, hi = (-2 ** 60, 2 ** 60) if dtype == "int64" else (-2.0, 1e300)
    h = np.concatenate([np.full(1792, lo, dtype), mid,
                        np.full(1792 - extra, hi, dtype)])
    assert h.size == 4096
    st = check(ra_gpu, np.random.default_rng(0).permutation(h), q=(49, 50, 51))
    assert st["collect_pass"] == (None if extra else 1), st


def test_more_prefixes_than_one_launch_holds(ra_gpu, geo):
    q = list(np.linspace(1, 99, 20))
    spread = np.random.default_rng(1).permutation(5000).astype(np.int16)
    both(ra_gpu, "percentile", spread - 2500, q=q)
    st = ra_gpu.deferred.get_runtime().last_select
    # top pass: one prefix; second: 20 top bytes, three launches, no collect
    assert st["launches"] > 2 + 20 // geo["nq_max"] - 1 and not st["collected"]
    both(ra_gpu, "percentile", spread % 200, q=q)   # one top byte: merged
    assert ra_gpu.deferred.get_runtime().last_select["launches"] == 2


HOSTILE = {
    "float64": [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.0, -1.0,
                2.2250738585072014e-308, 1.7976931348623157e308],
    "float32": [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0,
                1.1754944e-38, 3.4028235e38],
    "int64": [-2 ** 63, 2 ** 63 - 1, 2 ** 53 + 1, 2 ** 53 + 3, -2 ** 53 - 1,
              0, 2 ** 62 + 1, 2 ** 62 + 3],
    "int8": [-128, 127, 0, -1, 1],
}


@pytest.mark.parametrize("dtype", sorted(HOSTILE))
def test_hostile_values(ra_gpu, dtype):
    h = np.array(HOSTILE[dtype] * 3, dtype=dtype)[:-1]
    check(ra_gpu, h)
    check(ra_gpu, h[:-1])
    both(ra_gpu, "nanmedian", h)
    both(ra_gpu, "nanpercentile", h, q=[10, 50], method="lower")
    if h.dtype.kind != "f":
        return
    h[[2, 11]] = np.nan
    check(ra_gpu, h)                            # NaN from the plain functions
    both(ra_gpu, "nanmedian", h)
    both(ra_gpu, "nanpercentile", h, q=[0, 37.5, 100])
    both(ra_gpu, "nanquantile", h, q=0.5, method="midpoint")
    for fn, kw in (("nanmedian", {}), ("nanpercentile", dict(q=[5, 50]))):
        with pytest.warns(RuntimeWarning, match="All-NaN slice"):
            both(ra_gpu, fn, np.full(70, np.nan, dtype), **kw)


VIEWS = {
    "contiguous": lambda np_, x: x,
    "offset": lambda np_, x: x[1:],
    "step2": lambda np_, x: x[::2],
    "reversed": lambda np_, x: x[::-1],
    "transposed": lambda np_, x: x[:1024].reshape(32, 32).T,
    "broadcast": lambda np_, x: np_.broadcast_to(x[:300], (5, 300)),
}


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("dtype", ["float64", "float32", "int8"])
def test_views(ra_gpu, view, dtype):
    check(ra_gpu, values(1031, dtype), VIEWS[view])


@pytest.mark.parametrize("dtype", ["float64", "float32", "int32"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("shape", [(7, 65), (65, 7)])
def test_axis_composition(ra_gpu, shape, axis, dtype):
    # sort along the axis, slices and fused arithmetic; one line holds a NaN
    h = values(455, dtype).reshape(shape)
    if h.dtype.kind == "f":
        h[3, 5] = np.nan
    both(ra_gpu, "median", h, axis=axis)
    both(ra_gpu, "median", h, lambda np_, x: x[:-1, :-1], axis=axis)  # even
    for method in METHODS:
        both(ra_gpu, "percentile", h, q=[0, 37.5, 100], method=method,
             axis=axis)
    both(ra_gpu, "quantile", h, q=0.375, axis=axis)
