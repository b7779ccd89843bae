"""histogram / bincount on the HIP backend: every mode, counter regime and
load path of rt_hist against NumPy with array_equal, through the public
functions, with the host fallback taken away."""

import importlib

import numpy as np
import pytest

from hist_util import both, same

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:Converting input from bool")]

DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "bool"]
INTS = DTYPES[2:]
PATCH = ('import importlib\nimportlib.import_module("ramba_amd.histogram")'
         '.HostHist.hist_partial = None\n')


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):      # reaching HostHist is a TypeError
    mod = importlib.import_module("ramba_amd.histogram")
    monkeypatch.setattr(mod.HostHist, "hist_partial", None)


@pytest.fixture(scope="module")
def geo():
    from ramba_amd import hip_backend as hb
    return hb.hist_geometry(hb._load_lib())


def values(n, dtype, hi=7):      # 0 .. hi-1 (bool: 0 / 1), runs and ties
    return (np.arange(n) * 7 // 3 % (2 if dtype == "bool" else hi)) \
        .astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ["1", "unit-1", "unit", "unit+1", "63", "64",
                               "65", "255", "256", "257"])
def test_sizes_and_dtypes(ra_gpu, n, dtype):
    n = max(1, eval(n, {"unit": 16 // np.dtype(dtype).itemsize}))
    h = values(n, dtype)
    both(ra_gpu, "histogram", h, bins=5)
    both(ra_gpu, "histogram", h, bins=[0, 1, 1, 2.5, 6])
    same(ra_gpu.histogram(ra_gpu.fromarray(h[:1].repeat(n)), bins=3)[0],
         np.array([0, n, 0]))                     # all equal: exactly n
    if dtype in INTS:
        both(ra_gpu, "bincount", h, minlength=n % 9)


@pytest.mark.parametrize("dtype", ["float64", "float32", "int32"])
def test_two_grid_stride_trips_both_load_paths(ra_gpu, geo, dtype):
    # every block of the capped grid gets two full grid-stride trips, half of
    # them a third, plus a ragged tail
    per = 16 // np.dtype(dtype).itemsize
    lanes = geo["grid_cap"] * geo["block"] * 5 // 2
    h = values(lanes * per + per + 1, dtype, hi=100)
    both(ra_gpu, "histogram", h, bins=64)
    if dtype in INTS:
        both(ra_gpu, "bincount", h)
    # an offset view is not 16-byte aligned: one element per lane and trip
    both(ra_gpu, "histogram", h[:lanes + 3], lambda np_, x: x[1:], bins=3)


@pytest.mark.parametrize("which", ["1", "2", "wave", "wave+1", "block",
                                   "block+1"])
def test_nbins_at_the_regime_thresholds(ra_gpu, geo, which):
    nbins = eval(which, {"wave": geo["wave_max_bins"],
                         "block": geo["block_max_bins"]})
    rng = np.random.default_rng(nbins)
    h = rng.random(6001)
    h[:3] = [0.0, 1.0, np.nextafter(1.0, 0)]
    for dt in ("float64", "float32"):
        both(ra_gpu, "histogram", h.astype(dt), bins=nbins, range=(0, 1))
    both(ra_gpu, "histogram", h, bins=np.sort(rng.random(nbins + 1)))
    k = rng.integers(0, nbins, 6001)
    k[-1] = nbins - 1
    both(ra_gpu, "bincount", k)
    both(ra_gpu, "bincount", np.full(6001, nbins - 1))       # one hot bin
    both(ra_gpu, "histogram", np.full(6001, 0.5), bins=nbins, range=(0, 1))


@pytest.mark.parametrize("dtype,bins,rng", [
    ("float64", 8, (-1, 3)), ("float32", 8, (-1, 3)), ("int64", 8, (-1, 3)),
    ("float32", 1000, (0, 1))])   # float32 guess off by one before correction
def test_values_on_and_beside_every_edge(ra_gpu, dtype, bins, rng):
    kw = dict(bins=bins, range=rng)
    edges = np.histogram_bin_edges(np.empty(0, dtype), **kw).astype(dtype)
    if dtype == "int64":
        h = np.arange(-4, 7)
    else:
        h = np.concatenate([
            edges, np.nextafter(edges, edges.dtype.type(-9)),
            np.nextafter(edges, edges.dtype.type(9)),
            np.array([-1, 3, -5, 5, np.nan, np.inf, -np.inf], dtype=dtype)])
    if bins == 1000:
        ok = h[(h >= 0) & (h <= 1)]
        g = np.minimum((ok * np.float32(1000)).astype(int), 999)
        assert np.any(ok < edges[g]) or np.any(ok >= edges[g + 1])
    both(ra_gpu, "histogram", h, **kw)
    both(ra_gpu, "histogram", h, bins=edges[[0, 2, 2, 3, 8]])
    both(ra_gpu, "histogram", h, density=True, **kw)


VIEWS = {
    "contiguous": lambda np_, x: x,
    "offset": lambda np_, x: x[1:],
    "step2": lambda np_, x: x[::2],
    "reversed": lambda np_, x: x[::-1],
    "dense2d": lambda np_, x: x[:1024].reshape(32, 32),
    "transposed": lambda np_, x: x[:1024].reshape(32, 32).T,
    "broadcast": lambda np_, x: np_.broadcast_to(x[:300], (5, 300)),
}


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("dtype", ["float64", "float32", "int8"])
def test_load_paths(ra_gpu, view, dtype):
    h = values(1031, dtype, hi=11)
    both(ra_gpu, "histogram", h, VIEWS[view], bins=4)
    both(ra_gpu, "histogram", h, VIEWS[view], bins=[1, 2, 4.5, 20])
    if dtype == "int8" and VIEWS[view](np, h).ndim == 1:
        both(ra_gpu, "bincount", h, VIEWS[view])


@pytest.mark.parametrize("nedges", ["5", "lds", "lds+1"])
def test_edges_mode_uneven_and_repeated(ra_gpu, geo, nedges):
    nedges = eval(nedges, {"lds": geo["edges_lds_max"]})
    rng = np.random.default_rng(nedges)
    edges = np.sort(rng.normal(size=nedges))
    edges[1:nedges // 2:2] = edges[0:nedges // 2 - 1:2]   # repeats: empty bins
    edges[-2] = edges[-1]                                 # closed last bin
    h = np.concatenate([rng.normal(size=5000), edges,
                        np.nextafter(edges, -9), np.nextafter(edges, 9),
                        [np.nan, np.inf, -np.inf]])
    both(ra_gpu, "histogram", h, bins=edges)
    both(ra_gpu, "histogram", h.astype(np.float32), bins=edges)
    both(ra_gpu, "histogram", (h[:5000] * 100).astype(np.int32),
         bins=np.unique((edges * 100).astype(np.int64)))


def test_two_ranks_one_gpu(monkeypatch):
    import test_gpu_argreduce as spmd
    monkeypatch.setattr(spmd, "PATCH", PATCH)
    spmd.run_spmd_gpu("""
        rng = np.random.default_rng(5)
        h = rng.normal(size=10001)
        k = rng.integers(0, 5000, size=10001)
        g = rng.integers(0, 9, size=(53, 71)).astype(np.float32)
        a, b, c = np_.array(h), np_.array(k), np_.array(g)
        return [np_.histogram(a, bins=3000)[0], np_.histogram(a[::-3])[0],
                np_.histogram(a, bins=[-1, 0, 0, 2])[0],
                np_.histogram(c.T, bins=1)[0], np_.bincount(b),
                np_.bincount(b[:40], minlength=7000)]
    """)
