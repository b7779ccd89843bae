"""searchsorted on the HIP backend: both regimes of rt_searchsorted against
numpy.searchsorted, exactly, through the public function, with the host
fallback taken away.  The key counts come from rt_searchsorted_geometry."""

import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32", "int64", "int8", "bool"]


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):      # reaching HostUnique is a TypeError
    mod = importlib.import_module("ramba_amd.setops")
    for hook in ("unique_run", "search_core"):
        monkeypatch.setattr(mod.HostUnique, hook, None)


@pytest.fixture(scope="module")
def geo():
    from ramba_amd import hip_backend as hb
    return hb.searchsorted_geometry(hb._load_lib())


def keys(m, dtype, fence):
    """m sorted keys with duplicates; from 3 * seg keys on, a run of
    duplicates that is longer than two fence segments."""
    seg = -(-m // fence)
    k = np.arange(m) // 3 * 2               # even values, each three times
    if m > 3 * seg:
        k[seg // 2:seg // 2 + 2 * seg + 1] = k[seg // 2]
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return k > k[m // 2] if m else k.astype(bool)
    if dt.kind == "i" and dt.itemsize == 1:
        return np.sort((k % 251 - 125).astype(dt))
    return (k - k[m // 2] if m else k).astype(dt)


def needles(v, fence):
    """The specials of the dtype, below and above, the value of the planted
    run of duplicates, then EVERY value of v and the midpoints."""
    dt = v.dtype
    if dt == np.bool_:
        return np.array([False, True])
    u = np.unique(v) if v.size else np.zeros(1, dtype=dt)
    if dt.kind == "f":
        extra = [np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, u[0] - 1,
                 u[-1] + 1]
    else:
        info = np.iinfo(dt)
        extra = [info.min, info.max, 0, -1]
    seg = -(-v.size // fence)
    dup = v[min(v.size - 1, 3 * seg // 2)] if v.size else 0
    return np.concatenate([np.array(extra + [dup], dt), u, u + 1]).astype(dt)


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", ["0", "1", "2", "F-1", "F", "F+1", "lm-1", "lm",
                               "lm+1", "3*lm+7"])
def test_key_counts_dtypes_and_sides(ra_gpu, geo, m, dtype, side):
    lm = geo["lds_max"][np.dtype(dtype).itemsize]
    v = keys(eval(m, {"F": geo["fence"], "lm": lm}), dtype, geo["fence"])
    a = ra_gpu.fromarray(v)
    every = needles(v, geo["fence"])
    # all needles once; then 1, 65 and one tile plus one of them, cycled
    for n in (every.size, 1, 65, geo["block"] * 16 // v.itemsize + 1):
        x = np.resize(every, n)
        got = ra_gpu.searchsorted(a, ra_gpu.fromarray(x), side=side)
        ref = np.searchsorted(v, x, side=side)
        assert got.dtype == np.int64 and got.shape == ref.shape
        assert np.array_equal(got.asarray(), ref), (m, dtype, side, n)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_keys_writes_zeros(ra_gpu, dtype, side):
    # the public function answers m == 0 itself; the kernel's own m == 0
    # path (nothing staged, no LDS) is reached through the backend's library
    import ctypes
    import torch
    from ramba_amd import deferred, hip_backend as hb
    be = deferred.get_runtime().backend
    x = torch.ones(65, dtype=be._tdt(np.dtype(dtype)), device="cuda")
    out = torch.full((65,), -1, dtype=torch.int64, device="cuda")
    be._check(be.lib.rt_searchsorted(
        be._stream(), None, 0, ctypes.c_void_p(x.data_ptr()), 0, 1,
        hb._i64arr((65,)), hb._i64arr((1,)), hb.RT_DTYPE[dtype], side,
        ctypes.c_void_p(out.data_ptr())), "rt_searchsorted")
    assert not out.cpu().numpy().any()


@pytest.mark.parametrize("m", ["lm", "3*lm+7"])
def test_needle_views_and_scalar(ra_gpu, geo, m):
    v = keys(eval(m, {"lm": geo["lds_max"][4]}), "float32", geo["fence"])
    a = ra_gpu.fromarray(v)
    x = np.resize(needles(v, geo["fence"]), 41 * 67).reshape(41, 67)
    rx = ra_gpu.fromarray(x)
    for view in (lambda t: t[::3, 1::2], lambda t: t[::-1, ::-1],
                 lambda t: t.T):
        got = a.searchsorted(view(rx), side="right").asarray()
        assert np.array_equal(got, np.searchsorted(v, view(x), side="right"))
    got = np.searchsorted(a, np.float32(0.0))
    assert isinstance(got, np.int64) and got == np.searchsorted(v, 0.0)
