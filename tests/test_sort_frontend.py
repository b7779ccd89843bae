"""sort / argsort through the public interface on the oracle backend (the
portable HostSort hooks): shapes, dtypes, values and error messages equal
NumPy's stable sort, values by their bits."""

import numpy as np
import pytest

RNG = np.random.default_rng(3)
F64 = RNG.integers(-4, 5, 1001).astype(np.float64)
F64[::9] = np.nan
F64[1::9] = -0.0
DATA = {dt: RNG.integers(-50, 50, 1001).astype(dt)
        for dt in ("int64", "int32", "int16", "int8")}
DATA.update({"float64": F64, "float32": F64.astype(np.float32),
             "bool": RNG.integers(0, 2, 1001).astype(bool)})


def same(got, ref):
    got = got.asarray()
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert got.tobytes() == np.ascontiguousarray(ref).tobytes()


def both(ra, host, view=lambda x: x, **kw):
    a, h = view(ra.fromarray(host)), view(host)
    same(ra.sort(a, **kw), np.sort(h, kind="stable", **kw))
    same(ra.argsort(a, **kw), np.argsort(h, kind="stable", **kw))


@pytest.mark.parametrize("dtype", sorted(DATA))
def test_1d_nd_views_and_axis_none(ra, dtype):
    h = DATA[dtype]
    both(ra, h)
    both(ra, h, lambda x: x[::-3])
    both(ra, h[:1])
    cube = h[:990].reshape(9, 10, 11)
    for axis in (0, 1, 2, -1, -3, None):
        both(ra, cube, axis=axis)
    both(ra, cube, lambda x: x[1:, ::2].T, axis=1)
    both(ra, h[:16].reshape(2, 2, 2, 2), axis=1)


def test_zero_size_and_0d(ra):
    both(ra, np.zeros(0))
    both(ra, np.zeros((3, 0, 2), dtype=np.int16), axis=1)
    both(ra, np.zeros((3, 0, 2), dtype=np.int16), axis=None)
    with pytest.raises(np.exceptions.AxisError) as np_err:
        np.sort(np.float64(3.0))
    with pytest.raises(np.exceptions.AxisError) as err:
        ra.sort(np.float64(3.0))            # 0-d input is NumPy's to judge
    assert str(err.value) == str(np_err.value)


@pytest.mark.parametrize("kind", [None, "quicksort", "mergesort", "heapsort",
                                  "stable"])
def test_every_kind_gives_the_stable_result(ra, kind):
    h = DATA["int8"]
    same(ra.argsort(ra.fromarray(h), kind=kind), np.argsort(h, kind="stable"))
    same(ra.sort(ra.fromarray(h), kind=kind), np.sort(h, kind="stable"))


def test_unsupported_forms_raise(ra):
    a = ra.fromarray(F64)
    for fn in (ra.sort, ra.argsort):
        with pytest.raises(NotImplementedError, match="order="):
            fn(a, order="f0")
        with pytest.raises(NotImplementedError, match="complex"):
            fn(ra.fromarray(np.zeros(4, dtype=np.complex128)))
        with pytest.raises(NotImplementedError, match="4 dimensions"):
            fn(ra.fromarray(np.zeros((1, 2, 1, 2, 1))))


@pytest.mark.parametrize("shape,axis", [((7,), 1), ((7,), -2), ((3, 4), 2),
                                        ((3, 4), -3)])
def test_axis_error_is_numpys(ra, shape, axis):
    h = np.zeros(shape)
    for fn in ("sort", "argsort"):
        with pytest.raises(np.exceptions.AxisError) as np_err:
            getattr(np, fn)(h, axis=axis)
        with pytest.raises(np.exceptions.AxisError) as err:
            getattr(ra, fn)(ra.fromarray(h), axis=axis)
        assert str(err.value) == str(np_err.value)


def test_numpy_dispatch_methods_and_in_place(ra):
    h = DATA["float32"].reshape(7, 143)
    a = ra.fromarray(h)
    same(np.sort(a, axis=0), np.sort(h, axis=0, kind="stable"))
    same(np.argsort(a), np.argsort(h, kind="stable"))
    same(a.argsort(axis=0), np.argsort(h, axis=0, kind="stable"))
    view = a[:, 3:]
    view.sort(axis=1)               # in place, through the view
    ref = h.copy()
    ref[:, 3:].sort(axis=1, kind="stable")
    same(a, ref)
