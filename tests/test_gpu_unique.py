"""unique on the HIP backend: the rt_unique_* run compaction (and, for the
inverse, rt_searchsorted) against numpy.unique, through the public function,
with the host fallback taken away.  return_index=True makes NumPy's sort
stable, so all four results are compared exactly, the values by their bits."""

import importlib

import numpy as np
import pytest

from test_gpu_sort import DTYPES, bits, hostile, ties

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):      # reaching HostUnique is a TypeError
    mod = importlib.import_module("ramba_amd.setops")
    for hook in ("unique_run", "search_core"):
        monkeypatch.setattr(mod.HostUnique, hook, None)


@pytest.fixture(scope="module")
def geo():
    from ramba_amd import hip_backend as hb
    return hb.unique_geometry(hb._load_lib())


def check(ra, host, view=lambda x: x):
    a, h = view(ra.fromarray(host)), view(host)
    ref = np.unique(h, return_index=True, return_inverse=True,
                    return_counts=True)
    got = [g.asarray() for g in ra.unique(a, True, True, True)]
    assert got[0].dtype == h.dtype and got[0].shape == ref[0].shape
    assert np.array_equal(bits(got[0]), bits(ref[0])), (h.dtype, h.shape)
    for g, r, what in zip(got[1:], ref[1:], ("index", "inverse", "counts")):
        assert g.dtype == np.int64 and g.shape == r.shape, what
        assert np.array_equal(g, r), (what, h.dtype, h.shape)


def data(kind, n, dtype, tile):
    if kind == "ties":              # five distinct values with negatives
        return ties(n, dtype)
    if kind == "constant":
        return np.full(n, 1, dtype=dtype)
    k = np.arange(n)
    if kind == "distinct":          # a permutation, as far as the dtype goes
        k = (k * 7919) % n
    else:                           # runs of tile + 1 and a last run of one:
        k = k // (tile + 1)         # heads on every lane, wave, tile boundary
        k[-1] += 1
    if dtype == "bool":
        return (k % 2).astype(bool)
    info = np.iinfo(dtype) if np.dtype(dtype).kind == "i" else None
    span = 200 if info and info.max < n else n
    return (k % span - span // 2).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ["1", "2", "63", "64", "65", "tile-1", "tile",
                               "tile+1", "2*tile+3"])
def test_sizes_and_dtypes(ra_gpu, geo, n, dtype):
    n = eval(n, {"tile": geo["tile"]})
    for kind in ("ties", "distinct", "constant", "runs"):
        check(ra_gpu, data(kind, n, dtype, geo["tile"]))


def test_three_tiles_per_block_and_a_ragged_tail(ra_gpu, geo):
    # one key past twice the capped grid: every block walks three tiles, so
    # the running slot count and both reuses of the wave-sum buffer decide
    # where heads land.  Runs of 7 keys, the two sorted halves swapped: about
    # 585 heads in every tile of the sorted run, on every lane position (7
    # and 16 are coprime), and a last tile of one key.  int32, 64 MB; most of
    # the second or two it takes is NumPy's reference
    n = 2 * geo["grid_cap"] * geo["tile"] + 1
    k = np.arange(n, dtype=np.int32) // 7 - n // 14
    check(ra_gpu, np.concatenate([k[n // 2:], k[:n // 2]]))


@pytest.mark.parametrize("dtype", DTYPES[:6])
@pytest.mark.parametrize("n", ["65", "2*tile+3"])
def test_hostile_values(ra_gpu, geo, n, dtype):
    # +-0.0, four NaN bit patterns, +-inf, subnormals; the kept bits are
    # those of the first occurrence
    check(ra_gpu, hostile(dtype, eval(n, {"tile": geo["tile"]})))


@pytest.mark.parametrize("dtype", ["float64", "int16", "bool"])
def test_views(ra_gpu, dtype):
    check(ra_gpu, ties((41, 67), dtype), lambda x: x.T)
    check(ra_gpu, ties(301, dtype), lambda x: x[::-1])
    check(ra_gpu, ties((3, 5, 70), dtype))


@pytest.mark.parametrize("opt", ["none", "return_index", "return_inverse",
                                 "return_counts"])
def test_single_options(ra_gpu, geo, opt):
    host = data("runs", 2 * geo["tile"] + 3, "float32", geo["tile"])
    kw = {} if opt == "none" else {opt: True}
    got, ref = ra_gpu.unique(ra_gpu.fromarray(host), **kw), \
        np.unique(host, **kw)
    for g, r in zip(got if kw else [got], ref if kw else [ref]):
        g = g.asarray()
        assert g.dtype == r.dtype and np.array_equal(g, r), opt
