"""median / percentile / quantile on the CPU oracle backend: argument
handling, NumPy's messages, what is refused, result dtypes and shapes, and
the NumPy dispatch."""

import numpy as np
import pytest

from hist_util import both, same

H = (np.arange(101) * 37 % 101 - 50).astype(np.float32)


@pytest.mark.parametrize("dtype", ["float64", "float32", "int64", "uint8"])
@pytest.mark.parametrize("q", [30, 30.5, [30, 60.5], [[0, 100], [50, 1]],
                               np.float32(12.5), np.array(7)])
def test_result_dtype_and_shape_are_numpys(ra, dtype, q):
    h = H.astype(dtype)
    for method in ("linear", "lower", "midpoint"):
        both(ra, "percentile", h, q=q, method=method)
        both(ra, "nanquantile", h, q=np.asarray(q) / 100, method=method)
    both(ra, "quantile", h, q=0.25)
    both(ra, "quantile", h, q=1)
    both(ra, "median", h)
    both(ra, "median", h[:-1], overwrite_input=True)
    both(ra, "nanmedian", h)


@pytest.mark.parametrize("dtype", ["float64", "float32", "int64", "uint8"])
@pytest.mark.parametrize("axis", [0, -1, (0, 2), (2, 1), (0, 1, 2)])
def test_along_axes(ra, axis, dtype):
    h = np.resize(H, (4, 5, 6)).astype(dtype)
    if h.dtype.kind == "f":
        h[1, 2, 3] = np.nan
    for view in (lambda np_, x: x, lambda np_, x: x[:, ::2, 1:]):
        both(ra, "median", h, view, axis=axis)
    for method in ("linear", "higher", "nearest", "midpoint"):
        for q in (30.5, [[0, 100], [50, 1]], np.float32(62.5)):
            both(ra, "percentile", h, q=q, method=method, axis=axis)
    both(ra, "median", h[:0], axis=1)
    with pytest.raises(np.exceptions.AxisError):
        ra.median(ra.fromarray(h), axis=3)


def test_numpy_functions_dispatch(ra):
    a = ra.fromarray(H)
    same(np.median(a), np.median(H))
    same(np.percentile(a, [5, 95], method="higher"),
         np.percentile(H, [5, 95], method="higher"))
    same(np.nanquantile(a, 0.5), np.nanquantile(H, 0.5))
    same(ra.percentile(a, ra.fromarray(np.array([5., 95.]))),
         np.percentile(H, [5., 95.]))
    same(ra.median(list(H)), np.median(H))      # host data: NumPy's own


@pytest.mark.parametrize("fn,q,msg", [
    ("percentile", 101, "Percentiles must be in the range [0, 100]"),
    ("percentile", [50, -1], "Percentiles must be in the range [0, 100]"),
    ("nanpercentile", np.nan, "Percentiles must be in the range [0, 100]"),
    ("quantile", 1.5, "Quantiles must be in the range [0, 1]"),
    ("nanquantile", [0.5, -0.1], "Quantiles must be in the range [0, 1]")])
def test_q_out_of_range_raises_numpys_message(ra, fn, q, msg):
    for leg, x in ((ra, ra.fromarray(H)), (np, H)):
        with pytest.raises(ValueError) as e:
            getattr(leg, fn)(x, q)
        assert str(e.value) == msg


@pytest.mark.parametrize("fn,kw", [
    ("nanmedian", dict(axis=0)), ("nanquantile", dict(q=.5, axis=0)),
    ("nanpercentile", dict(q=[5, 50], axis=(0,))),
    ("median", dict(keepdims=True)), ("median", dict(out=np.empty(()))),
    ("percentile", dict(q=5, keepdims=True, out=np.empty(()))),
    ("percentile", dict(q=5, weights=np.ones(101), method="inverted_cdf")),
    ("percentile", dict(q=5, interpolation="lower")),
    ("quantile", dict(q=.5, method="hazen")),
    ("nanpercentile", dict(q=5, method="inverted_cdf"))])
def test_not_implemented(ra, fn, kw):
    with pytest.raises(NotImplementedError, match=fn):
        getattr(ra, fn)(ra.fromarray(H), **kw)


@pytest.mark.parametrize("h", [H > 0, H.astype(np.complex64),
                               H.astype(np.float16)])
def test_bool_complex_and_half_are_refused(ra, h):
    for fn, kw in (("median", {}), ("percentile", dict(q=5))):
        with pytest.raises(NotImplementedError, match="not supported"):
            getattr(ra, fn)(ra.fromarray(h), **kw)


def test_empty_input_follows_numpy(ra):
    e = np.empty(0, dtype=np.float32)
    with pytest.warns(RuntimeWarning):
        both(ra, "median", e)
    with pytest.warns(RuntimeWarning):
        both(ra, "nanpercentile", e, q=[5, 50])
