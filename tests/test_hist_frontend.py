"""histogram / bincount through the public interface on the oracle backend
(the portable HostHist hook): counts, edges, dtypes and error messages equal
NumPy's, with array_equal."""

import numpy as np
import pytest

from hist_util import both, same

RNG = np.random.default_rng(11)
F64 = RNG.normal(size=1001)
DATA = {dt: RNG.integers(-50, 50, 1001).astype(dt)
        for dt in ("int64", "int32", "int16", "int8")}
DATA.update({"float64": F64, "float32": F64.astype(np.float32),
             "bool": RNG.integers(0, 2, 1001).astype(bool)})


@pytest.mark.filterwarnings("ignore:Converting input from bool")
@pytest.mark.parametrize("dtype", sorted(DATA))
def test_histogram_signatures_and_dtypes(ra, dtype):
    h = DATA[dtype]
    both(ra, "histogram", h)
    both(ra, "histogram", h, bins=7)
    both(ra, "histogram", h, bins=np.int64(3), range=(-1, 2.5))
    both(ra, "histogram", h, bins=[-2, -0.5, 0, 0, 1, 40])
    both(ra, "histogram", h, bins=np.array([0, 1, 3]))
    both(ra, "histogram", h, bins=5, density=True)
    both(ra, "histogram", h, bins=[-3.0, -1, 0.25, 2], density=True)
    got = ra.histogram(ra.fromarray(h), bins=ra.fromarray(np.arange(4.0)))
    same(got, np.histogram(h, bins=np.arange(4.0)))


def test_histogram_ranges_views_and_empty(ra):
    for h in (F64, DATA["float32"], DATA["int64"]):
        both(ra, "histogram", h, range=(0, 1))
        both(ra, "histogram", h, bins=4, range=(2, 2))       # widened by 0.5
        both(ra, "histogram", h, lambda np_, x: x[::-3])
        both(ra, "histogram", h, lambda np_, x: x[1:901].reshape(30, 30).T[::2])
    both(ra, "histogram", np.full(40, 3, dtype=np.int8), bins=3)  # degenerate
    both(ra, "histogram", np.zeros(0), bins=4)
    both(ra, "histogram", np.zeros(0, dtype=np.float32), bins=[1, 2, 4])
    both(ra, "histogram", F64, bins=[1.5])                    # no bins at all
    nan = np.array([np.nan, -np.inf, np.inf, 0.0, 0.5, 1.0])
    both(ra, "histogram", nan, bins=2, range=(0, 1))
    both(ra, "histogram", nan, bins=[0, 0.5, 1])


@pytest.mark.parametrize("dtype", ["int64", "int32", "int16", "int8", "bool"])
def test_bincount(ra, dtype):
    h = np.abs(DATA[dtype])
    both(ra, "bincount", h)
    both(ra, "bincount", h, minlength=77)
    both(ra, "bincount", h, lambda np_, x: x[::-2])
    both(ra, "bincount", h[:0], minlength=5)


def test_numpy_dispatch_stays_distributed(ra):
    i32 = np.abs(DATA["int32"])
    hist, edges = np.histogram(ra.fromarray(F64), bins=6, range=(-1, 1))
    cnt = np.bincount(ra.fromarray(i32), minlength=9)
    assert isinstance(hist, ra.ndarray) and isinstance(edges, np.ndarray)
    assert isinstance(cnt, ra.ndarray)
    same((hist, edges, cnt), np.histogram(F64, bins=6, range=(-1, 1))
         + (np.bincount(i32, minlength=9),))


ERRORS = [
    ("histogram", F64, dict(bins=0)),
    ("histogram", F64, dict(bins=[0, 2, 1])),
    ("histogram", F64, dict(bins=np.ones((2, 2)))),
    ("histogram", F64, dict(range=(1, 0))),
    ("histogram", F64, dict(range=(0, np.inf))),
    ("histogram", np.array([1.0, np.nan]), {}),
    ("histogram", np.array([1.0, -np.inf], dtype=np.float32), dict(bins=3)),
    ("bincount", np.array([3, -1, 2]), {}),
    ("bincount", np.array([1.0, 2.0]), {}),
    ("bincount", np.ones((2, 3), dtype=np.int64), {}),
    ("bincount", np.array([1, 2]), dict(minlength=-1)),
]


@pytest.mark.parametrize("fn,host,kw", ERRORS)
def test_errors_are_numpys(ra, fn, host, kw):
    with pytest.raises(Exception) as ref:
        getattr(np, fn)(host, **kw)
    with pytest.raises(type(ref.value)) as got:
        getattr(ra, fn)(ra.fromarray(host), **kw)
    assert (type(got.value), str(got.value)) == (type(ref.value),
                                                 str(ref.value))
    assert int(ra.arange(10).sum()) == 45        # still usable


def test_out_of_scope_raises_not_implemented(ra):
    a, i = ra.fromarray(F64), ra.fromarray(np.abs(DATA["int64"]))
    big = ra.fromarray(np.array([2 ** 53 + 1, 5], dtype=np.int64))
    cplx = ra.fromarray(F64[:9] + 1j)
    for call in (lambda: ra.histogram(a, weights=a),
                 lambda: ra.histogram(cplx),
                 lambda: np.histogram(cplx, bins=3),
                 lambda: ra.histogram(a, bins="auto"),
                 lambda: np.histogram(a, bins="fd"),
                 lambda: ra.bincount(i, weights=a),
                 lambda: ra.histogram(big, bins=[0, 2 ** 53 + 1]),
                 lambda: np.histogram2d(a, a),
                 lambda: np.histogramdd(a)):
        with pytest.raises(NotImplementedError):
            call()
