"""unique / searchsorted on the oracle backend (the HostUnique hooks):
NumPy parity of the public functions, their routing and their refusals."""

import itertools

import numpy as np
import pytest

H = np.array([3.0, -0.0, np.nan, 0.0, 3.0, np.nan, -1.0, 7.0, 7.0, 7.0])
VIEWS = [lambda x: x, lambda x: x[::-1], lambda x: x.reshape(2, 5).T,
         lambda x: x.reshape(5, 2)[1:, ::-1]]


def same(got, ref):
    got = got.asarray() if hasattr(got, "asarray") else got
    assert got.dtype == ref.dtype and got.shape == np.shape(ref)
    assert np.array_equal(got, ref, equal_nan=got.dtype.kind == "f")


@pytest.mark.parametrize("opts", itertools.product([False, True], repeat=3))
@pytest.mark.parametrize("dtype", ["float64", "int16", "bool"])
def test_unique_option_combinations(ra, opts, dtype):
    host = np.nan_to_num(H).astype(dtype) if dtype != "float64" else H
    for view in VIEWS:
        got = np.unique(view(ra.fromarray(host)), *opts)    # routed by NumPy
        # return_index makes the reference sort stable (first occurrences)
        ref = np.unique(view(host), True, True, True)
        ref = [r for r, keep in zip(ref, (True,) + opts) if keep]
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(ref) and isinstance(got[0], ra.ndarray)
        for g, r in zip(got, ref):
            same(g, r)


def test_unique_host_passthrough_and_empty(ra):
    got = ra.unique([2, 1, 2], return_counts=True)
    assert isinstance(got[0], np.ndarray) and list(got[1]) == [1, 2]
    for g, r in zip(ra.unique(ra.zeros((0, 3), dtype=np.int8), True, True,
                              True),
                    np.unique(np.zeros((0, 3), dtype=np.int8), True, True,
                              True)):
        same(g, r)


@pytest.mark.parametrize("side", ["left", "right"])
def test_searchsorted_routes_and_promotion(ra, side):
    v = np.array([-2, 0, 0, 3, 3, 3, 9], dtype=np.int32)
    x = np.array([[-5, 0, 1], [3, 9, 10]])
    a, rx = ra.fromarray(v), ra.fromarray(x)
    for got in (ra.searchsorted(a, rx, side), np.searchsorted(a, rx, side),
                a.searchsorted(rx, side), ra.searchsorted(v, rx, side),
                ra.searchsorted(a, x, side), ra.searchsorted(a, rx.T, side).T):
        same(got, np.searchsorted(v, x, side))
    # promotion as NumPy's: int32 keys and float needles compare in float64,
    # int64 keys lose their low bits against a float needle
    f = np.array([-0.5, np.nan, 3.0, 2.5])
    same(ra.searchsorted(a, ra.fromarray(f), side), np.searchsorted(v, f, side))
    big = np.array([2 ** 53, 2 ** 53 + 1], dtype=np.int64)
    same(ra.searchsorted(ra.fromarray(big), ra.fromarray(f[:1] + 2.0 ** 53),
                         side),
         np.searchsorted(big, f[:1] + 2.0 ** 53, side))
    for needle in (3, 2.5, np.int8(-7)):
        got = ra.searchsorted(a, needle, side)
        assert type(got) is np.int64 and got == np.searchsorted(v, needle, side)
    same(ra.searchsorted(a, ra.zeros((0, 2)), side), np.zeros((0, 2), np.int64))
    same(ra.searchsorted(ra.zeros(0), rx, side), np.zeros(x.shape, np.int64))
    assert isinstance(ra.searchsorted(v, x, side), np.ndarray)


def test_refusals_name_the_limit(ra):
    a = ra.fromarray(H)
    with pytest.raises(NotImplementedError, match="axis= is not supported"):
        ra.unique(a, axis=0)
    with pytest.raises(NotImplementedError, match="equal_nan=False"):
        ra.unique(a, equal_nan=False)
    same(ra.unique(ra.fromarray(np.array([2, 1, 2])), equal_nan=False),
         np.array([1, 2]))
    with pytest.raises(NotImplementedError, match="complex input"):
        ra.unique(ra.fromarray(H.astype(np.complex128)))
    with pytest.raises(NotImplementedError, match="up to 4 dimensions"):
        ra.unique(ra.zeros((2,) * 5))
    with pytest.raises(NotImplementedError, match="sorter= is not supported"):
        ra.searchsorted(a, 1.0, sorter=np.arange(10))
    with pytest.raises(ValueError, match=r"search side must be 'left' or "
                                         r"'right' \(got 'middle'\)"):
        ra.searchsorted(a, 1.0, side="middle")
    with pytest.raises(ValueError, match="object too deep"):
        ra.searchsorted(ra.zeros((2, 2)), 1.0)
    with pytest.raises(NotImplementedError, match="no search kernel for "
                                                  "dtype complex128"):
        ra.searchsorted(a, 1j)
