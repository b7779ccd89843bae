"""The NumPy models of tests/rt_ref.py against ordinary NumPy, so the
reference the GPU kernel suite compares with is not itself the unknown;
plus the exact-sum bound on the inputs that suite feeds the scans."""

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

import rt_ref
from rt_ref import geom

RNG = np.random.default_rng(7)


def _strided(buf, off, shape, strides):
    return as_strided(buf[off:], shape=shape,
                      strides=tuple(s * buf.itemsize for s in strides))


VIEWS = [   # (buffer size, off, shape, strides): every access stays inside
    (64, 0, (7,), (1,)),
    (64, 3, (7,), (2,)),
    (64, 40, (9,), (-3,)),
    (200, 5, (3, 5), (7, 1)),
    (200, 5, (5, 3), (1, 7)),
    (200, 100, (3, 5), (-20, 2)),
    (200, 4, (3, 5), (0, 1)),
    (400, 9, (2, 3, 4), (50, 12, 1)),
    (400, 9, (4, 3, 2), (1, 12, 50)),
    (900, 11, (2, 3, 4, 5), (200, 60, 11, 2)),
]


@pytest.mark.parametrize("size,off,shape,strides", VIEWS)
def test_offsets_reach_and_geom(size, off, shape, strides):
    buf = np.arange(size, dtype=np.int64)
    v = _strided(buf, off, shape, strides)
    o = rt_ref.offsets(off, shape, strides)
    assert np.array_equal(buf[o], v)          # buf holds its own offsets
    assert rt_ref.reach(off, shape, strides) == (v.min(), v.max())
    assert np.array_equal(rt_ref.read(buf, off, shape, strides), v)
    if 0 not in strides:
        assert geom(v, buf) == (off, tuple(strides))
    assert rt_ref.reach(3, (4, 0), (1, 1)) is None


@pytest.mark.parametrize("size,off,shape,strides", VIEWS)
def test_copy_box_is_strided_slice_assignment(size, off, shape, strides):
    src = RNG.integers(-100, 100, size).astype(np.int32)
    dst = np.full(500, -7, dtype=np.int32)
    n = int(np.prod(shape))
    dshape = tuple(reversed(shape))
    dview_str = np.empty(dshape, dtype=np.int8).T.strides   # a transpose
    want = dst.copy()
    _strided(want, 13, shape, dview_str)[...] = _strided(src, off, shape,
                                                         strides)
    got = rt_ref.copy_box(dst, src, shape, dview_str, strides, 13, off)
    assert np.array_equal(got, want)
    assert (got != -7).sum() <= n and np.all(dst == -7)


@pytest.mark.parametrize("op", rt_ref.OPS)
@pytest.mark.parametrize("dtype", rt_ref.DT7)
def test_combine_box_is_numpy_ufunc(dtype, op):
    info = None if np.dtype(dtype).kind == "f" else np.iinfo(dtype)
    if info is None:
        d = RNG.integers(-8, 9, 60).astype(dtype)
        s = RNG.integers(-8, 9, 60).astype(dtype)
        d[5] = s[9] = d[11] = s[11] = np.nan
    else:
        d = RNG.integers(info.min, info.max, 60, endpoint=True).astype(dtype)
        s = RNG.integers(info.min, info.max, 60, endpoint=True).astype(dtype)
    d[::7] = 0
    s[::5] = 0
    with np.errstate(all="ignore"):
        want = {"add": lambda: np.add(d, s), "mul": lambda: np.multiply(d, s),
                "min": lambda: np.minimum(d, s),
                "max": lambda: np.maximum(d, s),
                "land": lambda: np.logical_and(d, s).astype(dtype),
                "lor": lambda: np.logical_or(d, s).astype(dtype)}[op]()
    got = rt_ref.combine_box(d, s, (60,), (1,), (1,), 0, 0, op)
    assert got.dtype == want.dtype == np.dtype(dtype)
    assert np.array_equal(got, want, equal_nan=info is None)
    # a strided box leaves the rest alone; stride 0 broadcasts the source
    got = rt_ref.combine_box(d, s, (3, 4), (12, 2), (0, 1), 5, 2, "add")
    want = d.copy()
    with np.errstate(all="ignore"):
        _strided(want, 5, (3, 4), (12, 2))[...] += s[2:6]
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("dtype", rt_ref.DT4)
@pytest.mark.parametrize("n", [1, 17, 100, 257])
def test_cumsum_models_are_numpy_cumsum(dtype, n):
    x = RNG.integers(-8, 9, n).astype(dtype)
    for chunk in (16, 100):
        b = rt_ref.chunk_sums(x, chunk)
        assert b.dtype == x.dtype and b.size == -(-n // chunk)
        assert np.array_equal(b, np.add.reduceat(x, np.arange(0, n, chunk)))
        excl, total = rt_ref.exclusive_scan(b)
        assert np.array_equal(excl, np.cumsum(b) - b) and total == x.sum()
        got = rt_ref.cumsum_apply(x, excl, 5, chunk)
        assert got.dtype == x.dtype
        assert np.array_equal(got, np.cumsum(x) + 5)
        assert np.array_equal(got, rt_ref.cumsum_full(x, 5))
    buf = np.arange(1000, dtype=np.int64)
    assert np.array_equal(rt_ref.line(buf, 900, -3, n), buf[900::-3][:n])


@pytest.mark.parametrize("size,off,shape,strides",
                         [v for v in VIEWS if len(v[2]) >= 2])
def test_axis_scan_is_numpy_cumsum(size, off, shape, strides):
    inp = RNG.integers(-8, 9, size).astype(np.float32)
    out = np.full(2000, -1, dtype=np.float32)
    pshape = tuple(s + 2 for s in shape)
    ostr = tuple(x // 4 for x in np.empty(pshape, np.float32).strides)
    for axis in range(len(shape)):
        v = _strided(inp, off, shape, strides)
        got, tot = rt_ref.axis_scan(out, inp, shape, strides, ostr, off, 17,
                                    axis)
        want = out.copy()
        _strided(want, 17, shape, ostr)[...] = np.cumsum(v, axis=axis)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(tot, v.sum(axis=axis).reshape(-1))


@pytest.mark.parametrize("size,off,shape,strides", VIEWS)
def test_mask_models_are_boolean_getitem(size, off, shape, strides):
    a = RNG.integers(-100, 100, size).astype(np.int16)
    m = (RNG.integers(0, 3, 700) * 5).astype(np.uint8)   # 0, 5 or 10
    mstr = tuple(x for x in np.empty(tuple(s + 1 for s in shape),
                                     np.uint8).strides)
    av, mv = _strided(a, off, shape, strides), _strided(m, 3, shape, mstr)
    got = rt_ref.mask_compact(a, m, off, 3, shape, strides, mstr)
    assert got.dtype == a.dtype and np.array_equal(got, av[mv != 0])
    for chunk in (4, 1000):
        c = rt_ref.mask_counts(m, 3, shape, mstr, chunk)
        assert c.dtype == np.int64 and c.sum() == got.size
        assert c.size == -(-av.size // chunk)
        assert c[0] == (mv.reshape(-1)[:chunk] != 0).sum()


@pytest.mark.parametrize("size,off,shape,strides", VIEWS)
def test_flat_copy_is_reshape_slice(size, off, shape, strides):
    x = RNG.integers(-100, 100, size).astype(np.int32)
    v = _strided(x, off, shape, strides)
    n_all = v.size
    for flat0, n in ((0, n_all), (1, n_all - 1), (2, 3), (n_all - 1, 1),
                     (n_all, 0), (3, 0)):
        got = rt_ref.flat_gather(x, off, shape, strides, flat0, n)
        assert np.array_equal(got, v.reshape(-1)[flat0:flat0 + n])
        if 0 in strides:
            continue            # scatter into a broadcast box is ill-defined
        dense = np.arange(n, dtype=np.int32) + 1000
        got = rt_ref.flat_scatter(x, dense, off, shape, strides, flat0, n)
        want = x.copy()
        wv = _strided(want, off, shape, strides)
        flat = wv.reshape(-1).copy()
        flat[flat0:flat0 + n] = dense
        wv[...] = flat.reshape(shape)
        assert np.array_equal(got, want)


def test_exact_float_sums_rule():
    assert rt_ref.exact_float_sums(np.full(100, 8.0), "float32", 1000)
    assert not rt_ref.exact_float_sums(np.full(100, 8.5), "float32")
    assert not rt_ref.exact_float_sums(np.full(100, 9.0), "float32")
    assert not rt_ref.exact_float_sums(np.full(1 << 21, 8.0), "float32")
    assert rt_ref.exact_float_sums(np.full(1 << 21, 8.0), "float64")


def test_gpu_suite_scan_inputs_keep_every_partial_sum_exact():
    """The exact-comparison rule of tests/test_gpu_rt_kernels.py: every
    float input its scan and add/mul-combine cases generate is integer
    valued with |x| <= 8, and sum(|x|) + |base| of every scanned line is
    under 2^24 (float32) / 2^53 (float64), so any summation order gives
    the same bits."""
    import os
    import rt_cases
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.skip("libramba_rt.so not built (chunk size comes from it)")
    C = hip_backend._load_lib().rt_scan_chunk()
    seen = 0
    for dtype, x, base in rt_cases.float_scan_inputs(C):
        assert rt_ref.exact_float_sums(x, dtype, base), (dtype, x.size, base)
        seen += 1
    assert seen > 20
    for dtype, x in rt_cases.float_combine_inputs():
        v = np.asarray(x, dtype=np.float64)
        assert np.all(v == np.round(v)) and np.all(np.abs(v) <= 8)
        # one add or mul of two such values: at most 64, exact in float32
