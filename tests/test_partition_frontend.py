"""partition / argpartition through the public interface on the oracle
backend (the portable HostSort.split_run hook).  The flat path has ONE defined
result, the stable split about the elements at the kth ranks, restated here in
plain NumPy and compared exactly, values by their bits."""

import numpy as np
import pytest

RNG = np.random.default_rng(11)
F64 = RNG.integers(-4, 5, 1001).astype(np.float64)
F64[::9] = np.nan
F64[1::9] = -0.0
DATA = {dt: RNG.integers(-50, 50, 1001).astype(dt)
        for dt in ("int64", "int32", "int16", "int8")}
DATA.update({"float64": F64, "float32": F64.astype(np.float32),
             "bool": RNG.integers(0, 2, 1001).astype(bool)})


def expected_argpartition(h, kth):
    """The defined result: buckets below / equal to / between the elements at
    the kth ranks, in ascending order, each in input order."""
    s = np.sort(h, kind="stable")
    ks = np.unique(np.atleast_1d(kth) % h.size)
    lo = np.searchsorted(s, h, "left")
    piv = np.unique(np.searchsorted(s, s[ks], "left"))
    b = 2 * np.searchsorted(piv, lo, "left") + np.isin(lo, piv)
    return np.argsort(b, kind="stable")


def exact(ra, host, kth, view=lambda x: x, **kw):
    a, h = view(ra.fromarray(host)), view(host)
    idx = expected_argpartition(h.reshape(-1), kth)
    got = ra.partition(a, kth, **kw).asarray()
    assert got.dtype == h.dtype and got.shape == idx.shape
    assert got.tobytes() == h.reshape(-1)[idx].tobytes(), (h.dtype, kth)
    got = ra.argpartition(a, kth, **kw).asarray()
    assert got.dtype == np.int64 and np.array_equal(got, idx), (h.dtype, kth)


def contract(got, h, kth, axis):
    """NumPy's contract along `axis`: the element at each kth is the sorted
    array's, and both sides hold the sorted array's elements."""
    got, s = np.moveaxis(got, axis, -1), np.sort(np.moveaxis(h, axis, -1))
    assert got.shape == s.shape
    cuts = [0] + sorted(set(k % s.shape[-1] for k in kth)) + [s.shape[-1]]
    for k in cuts[1:-1]:
        assert np.array_equal(got[..., k], s[..., k], equal_nan=True)
    for a, b in zip(cuts, cuts[1:]):
        assert np.array_equal(np.sort(got[..., a:b]), s[..., a:b],
                              equal_nan=True)


@pytest.mark.parametrize("dtype", sorted(DATA))
@pytest.mark.parametrize("kth", [0, 500, 1000, -1, 890, [3, 500, -2],
                                 [0, 1, 2, 3, 4, 5, 6, 7]])
def test_flat_path_is_the_stable_split(ra, dtype, kth):
    h = DATA[dtype]                 # kth 890 and up: the pivot is NaN
    exact(ra, h, kth)
    exact(ra, h, (np.atleast_1d(kth) % 334).tolist(), lambda x: x[::-3])
    exact(ra, h[:990].reshape(9, 110), (np.atleast_1d(kth) % 990).tolist(),
          lambda x: x.T, axis=None)
    exact(ra, h[:1], 0)


@pytest.mark.parametrize("axis", [0, 1, -1])
def test_nd_and_many_kth_meet_numpys_contract(ra, axis):
    h = DATA["float32"][:990].reshape(9, 110)
    a = ra.fromarray(h)
    contract(ra.partition(a, [2, 5], axis=axis).asarray(), h, [2, 5], axis)
    idx = ra.argpartition(a, 4, axis=axis).asarray()
    contract(np.take_along_axis(h, idx, axis), h, [4], axis)
    nine = list(range(0, 900, 100))         # more pivots than one split takes
    flat = DATA["int16"]
    contract(ra.partition(ra.fromarray(flat), nine).asarray(), flat, nine, 0)


def test_numpy_dispatch_methods_and_in_place(ra):
    h = DATA["float64"]
    a = ra.fromarray(h)
    idx = expected_argpartition(h, 77)
    for got in (np.partition(a, 77), np.argpartition(a, 77),
                a.argpartition(77)):
        assert isinstance(got, ra.ndarray)
    assert np.array_equal(np.argpartition(a, 77).asarray(), idx)
    assert np.array_equal(a.argpartition(77).asarray(), idx)
    assert np.partition(a, 77).asarray().tobytes() == h[idx].tobytes()
    view = a[1:]
    view.partition(5)               # in place, through the view
    assert a.asarray()[1:].tobytes() == \
        h[1:][expected_argpartition(h[1:], 5)].tobytes()
    assert isinstance(ra.partition(h, 3), np.ndarray)   # host data: NumPy's


@pytest.mark.parametrize("shape,kth,kw", [
    ((5,), 5, {}), ((5,), -6, {}), ((5,), [1, 7], {}), ((5,), 1.5, {}),
    ((5,), [[1]], {}), ((3, 4), 3, {"axis": 0}), ((3, 4), 1, {"axis": 2})])
def test_errors_are_numpys(ra, shape, kth, kw):
    h = np.zeros(shape)
    for fn in ("partition", "argpartition"):
        with pytest.raises(Exception) as np_err:
            getattr(np, fn)(h, kth, **kw)
        with pytest.raises(type(np_err.value)) as err:
            getattr(ra, fn)(ra.fromarray(h), kth, **kw)
        assert str(err.value) == str(np_err.value)


def test_unsupported_forms_raise_and_empty_is_empty(ra):
    a = ra.fromarray(F64)
    for fn in (ra.partition, ra.argpartition):
        with pytest.raises(NotImplementedError, match="order="):
            fn(a, 1, order="f0")
        with pytest.raises(NotImplementedError, match="complex"):
            fn(ra.fromarray(np.zeros(4, dtype=np.complex128)), 1)
        with pytest.raises(NotImplementedError, match="4 dimensions"):
            fn(ra.fromarray(np.zeros((1, 2, 1, 2, 1))), 0)
    h = np.zeros((0, 3), dtype=np.int16)     # NumPy checks no bounds here
    assert np.partition(h, 5).shape == h.shape
    got = ra.partition(ra.fromarray(h), 5).asarray()
    assert got.shape == h.shape and got.dtype == h.dtype
    got = ra.argpartition(ra.fromarray(h), 1).asarray()
    assert got.shape == h.shape and got.dtype == np.int64
