"""groupby through the public interface on the oracle backend (the portable
HostGroup hook): all nine methods against NumPy, the label forms, and every
error."""

import numpy as np
import pytest

RNG = np.random.default_rng(3)
LAB = RNG.integers(0, 5, size=23)
LAB[LAB == 3] = 1                       # group 3 is empty
DATA = {dt: RNG.integers(-9, 9, size=(23, 6, 4)).astype(dt)
        for dt in ("float64", "float32", "int64", "int32", "int16", "int8")}
DATA["bool"] = DATA["int8"] > 0


def per_group(h, dim, lab, ng, fn, dtype):
    """fn over the rows of each group, NaN-filled where fn has no answer."""
    x = np.moveaxis(h, dim, 0)
    out = np.full((ng,) + x.shape[1:], np.nan, dtype)
    for k in range(ng):
        if np.any(lab == k):
            out[k] = fn(x[lab == k], axis=0)
    return np.moveaxis(out, 0, dim)


def same(got, ref, exact=True):
    got = got.asarray()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype,
                                                                ref.dtype)
    if exact:
        np.testing.assert_array_equal(got, ref)
    else:
        # the data are small integers, so the sums behind the means are exact
        # and the means agree; the squares are non-negative, so summing at
        # most 23 of them in another order moves the result by under 23 eps
        np.testing.assert_allclose(got, ref, rtol=23 * np.finfo(ref.dtype).eps)


@pytest.mark.parametrize("dtype", sorted(DATA))
@pytest.mark.parametrize("dim", [0, 2])
def test_nine_methods_against_numpy(ra, dtype, dim):
    h = np.moveaxis(DATA[dtype], 0, dim)
    a, ng = ra.fromarray(np.ascontiguousarray(h)), 5
    g = a.groupby(dim, LAB, ng)
    x = h.view(np.uint8) if dtype == "bool" else h
    wide = np.int64 if h.dtype.kind in "ib" else h.dtype
    flt = h.dtype if h.dtype.kind == "f" else np.float64
    cnt = per_group(np.ones(h.shape), dim, LAB, ng, np.sum, np.float64)
    cnt = np.nan_to_num(cnt).astype(np.int64)
    same(g.count(), cnt)
    for name, fn, ident in (("sum", np.sum, 0), ("prod", np.prod, 1)):
        ref = per_group(x.astype(wide), dim, LAB, ng, fn, np.float64)
        same(getattr(g, name)(dim=None),
             np.where(np.isnan(ref), ident, ref).astype(wide))
    for name, fn in (("min", np.min), ("max", np.max)):
        ref = per_group(x, dim, LAB, ng, fn, np.float64)
        got = getattr(g, name)().asarray()
        assert got.dtype == h.dtype
        np.testing.assert_array_equal(got[cnt > 0], ref[cnt > 0])
        if dtype == "bool":
            assert np.all(got[cnt == 0] == (name == "min"))
        else:
            lim = np.finfo(flt) if h.dtype.kind == "f" else np.iinfo(h.dtype)
            edge = (np.inf if h.dtype.kind == "f" else lim.max) \
                if name == "min" else \
                (-np.inf if h.dtype.kind == "f" else lim.min)
            assert np.all(got[cnt == 0] == edge)
    same(g.mean(), per_group(x, dim, LAB, ng, np.mean, flt), exact=False)
    same(g.nanmean(), per_group(x, dim, LAB, ng, np.mean, flt), exact=False)
    same(g.var(), per_group(x.astype(flt), dim, LAB, ng, np.var, flt),
         exact=False)
    same(g.std(), per_group(x.astype(flt), dim, LAB, ng, np.std, flt),
         exact=False)
    total, count = g.mean(ret_separate=True)
    same(total, g.sum().asarray())
    same(count, cnt)


def test_label_forms_default_num_groups_views_and_nanmean(ra):
    h = DATA["float64"].copy()
    h[::3, 1] = np.nan
    a = ra.fromarray(h)
    ref = a.groupby(0, LAB).sum().asarray()
    assert ref.shape == (int(LAB.max()) + 1, 6, 4)      # max(label) + 1
    for lab in (list(LAB), LAB.astype(np.int8), ra.fromarray(LAB)):
        np.testing.assert_array_equal(a.groupby(0, lab).sum().asarray(), ref)
    t = a.T[:, ::-1]                                    # dim moves to 2
    np.testing.assert_array_equal(
        t.groupby(2, LAB, 6).max().asarray()[:, :, :5],
        a.groupby(0, LAB).max().asarray().T[:, ::-1])
    total, count = a.groupby(0, LAB, 5).nanmean(ret_separate=True)
    assert count.dtype == np.int64
    x = np.where(np.isnan(h), 0, h)
    for k in (0, 1, 2, 4):
        np.testing.assert_array_equal(total.asarray()[k],
                                      np.add.reduce(x[LAB == k], axis=0))
        np.testing.assert_array_equal(
            count.asarray()[k], (~np.isnan(h[LAB == k])).sum(axis=0))
    with np.errstate(all="raise"):          # 0 / 0 is NaN, and silent
        assert np.isnan(a.groupby(0, LAB, 5).nanmean().asarray()[3]).all()
    assert isinstance(a.groupby(0, LAB), ra.Groupby)
    empty = ra.fromarray(np.zeros((0, 3))).groupby(0, [], 2)
    np.testing.assert_array_equal(empty.min().asarray(),
                                  np.full((2, 3), np.inf))


ERRORS = [
    (dict(lab=np.array([0, 1, -1] + [0] * 20)), ValueError, "labels must lie"),
    (dict(lab=LAB, ng=4), ValueError, "labels must lie"),
    (dict(lab=LAB.astype(float)), ValueError, "must be an integer array"),
    (dict(lab=LAB[:-1]), ValueError, "has shape (22,)"),
    (dict(lab=LAB.reshape(1, -1)), ValueError, "has shape (1, 23)"),
    (dict(dim=3), ValueError, "out of range"),
    (dict(dim=-1), ValueError, "out of range"),
    (dict(ng=0), ValueError, "at least 1"),
    (dict(key="complex"), NotImplementedError, "complex"),
    (dict(key="5d"), NotImplementedError, "up to 4 dimensions"),
]


@pytest.mark.parametrize("kw,exc,what", ERRORS)
def test_errors(ra, kw, exc, what):
    src = {"complex": DATA["float64"] + 1j,
           "5d": DATA["int8"].reshape(23, 6, 2, 2, 1)}.get(
               kw.get("key"), DATA["float32"])
    with pytest.raises(exc, match=what.replace("(", r"\(").replace(")", r"\)")):
        ra.fromarray(src).groupby(kw.get("dim", 0), kw.get("lab", LAB),
                                  kw.get("ng", 5))
    assert int(ra.arange(10).sum()) == 45        # still usable
