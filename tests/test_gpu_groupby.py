"""groupby reductions on the HIP backend: every regime, load path and
threshold of rt_group_reduce against the np.<ufunc>.at model, through the
public interface, with the host fallback taken away.  Float data are small
integers (products: powers of two), so every summation order gives the same
bits and every comparison is array_equal; one test takes generic floats
against math.fsum with a derived bound."""

import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "bool"]
OPS = {"sum": np.add, "prod": np.multiply, "min": np.minimum,
       "max": np.maximum}
ROWS, ROWS_SPLIT, LINE_SELECT, LINE_GATHER = range(4)


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):      # reaching HostGroup is a TypeError
    from ramba_amd import groupby
    monkeypatch.setattr(groupby.HostGroup, "group_partial", None)


@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend as hb
    return hb._load_lib()


@pytest.fixture(scope="module")
def geo(lib):
    from ramba_amd import hip_backend as hb
    return hb.group_geometry(lib)


def regime(lib, h, dim, ngroups):       # of a C-contiguous host array
    arr = lambda v: (ctypes.c_int64 * len(v))(*v)
    code = {"float64": 0, "float32": 1, "int64": 2, "int32": 3, "int16": 4,
            "int8": 5, "bool": 6}[str(h.dtype)]
    return lib.rt_group_regime(h.ndim, arr(h.shape),
                               arr([s // h.itemsize for s in h.strides]),
                               dim, code, ngroups)


def values(shape, dtype, prod=False):
    k = np.arange(int(np.prod(shape))).reshape(shape) * 7 // 3
    if dtype == "bool":
        return k % 2 == 0
    if prod:        # exact in any order: +-1, 2, 0.5 (integers: 1, -1, 2, 0)
        return np.array([1, -1, 2, 0.5, -1, 0.5, 2, 1])[k % 8].astype(dtype)
    return (k % 7 - 3).astype(dtype)


def labels(n, ngroups):      # group ngroups - 1 stays empty when ngroups > 2
    return (np.arange(n) * 5 // 2) % max(1, ngroups - (ngroups > 2))


def model(h, dim, lab, ngroups, op):
    from ramba_amd import groupby as gb
    code = list(OPS).index(op)
    x = np.moveaxis(h.view(np.uint8) if h.dtype == np.bool_ else h, dim, 0)
    dt = gb.acc_dtype(h.dtype, code)
    out = np.full((ngroups,) + x.shape[1:], gb.identity(h.dtype, code), dt)
    OPS[op].at(out, lab, x.astype(dt))
    return np.moveaxis(out, 0, dim).astype(gb.result_dtype(h.dtype, code))


def check(ra, h, dim, ngroups, view=lambda x: x, ops=OPS, lab=None, hp=None):
    hv = view(h)
    lab = labels(hv.shape[dim], ngroups) if lab is None else lab
    for op in ops:
        src = hp if op == "prod" and hp is not None else h
        got = getattr(view(ra.fromarray(src)).groupby(dim, lab, ngroups),
                      op)().asarray()
        ref = model(view(src), dim, lab, ngroups, op)
        assert got.dtype == ref.dtype and got.shape == ref.shape, (op, got)
        np.testing.assert_array_equal(got, ref, err_msg=f"{op} {h.dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_dtype_and_op_in_every_regime(ra_gpu, lib, geo, dtype):
    big = geo["select_max"] + 24
    cases = [((37, 5, 9), 0, 6, ROWS), ((2 * geo["chunk"] + 3, 5), 0, 3,
                                        ROWS_SPLIT),
             ((3, 700), 1, 5, LINE_SELECT), ((3, 700), 1, big, LINE_GATHER)]
    for shape, dim, ng, want in cases:
        h, hp = values(shape, dtype), values(shape, dtype, prod=True)
        assert regime(lib, h, dim, ng) == want
        check(ra_gpu, h, dim, ng, hp=hp)


@pytest.mark.parametrize("shape,dim", [((6, 7, 8), d) for d in range(3)]
                         + [((3, 4, 5, 6), d) for d in range(4)])
def test_dim_at_each_position(ra_gpu, shape, dim):
    for dtype in ("float32", "int16"):
        check(ra_gpu, values(shape, dtype), dim, 3, ops=("sum", "min"))


@pytest.mark.parametrize("dtype", ["float64", "float32", "int8"])
@pytest.mark.parametrize("inner", ["1", "V-1", "V", "V+1", "255*V", "256*V",
                                   "256*V+1", "257*V"])
def test_inner_extents_around_the_load_unit_and_the_tile(ra_gpu, inner, dtype):
    n = eval(inner, {"V": 16 // np.dtype(dtype).itemsize})
    check(ra_gpu, values((9, n), dtype), 0, 4, ops=("sum", "max"))


@pytest.mark.parametrize("rows", ["1", "tile-1", "tile", "tile+1",
                                  "4*tile+1"])
def test_group_sizes_around_the_member_tile(ra_gpu, geo, rows):
    k = eval(rows, {"tile": geo["member_tile"]})
    h = values((k, 40), "float32")
    check(ra_gpu, h, 0, 1, ops=("sum", "min"))      # all rows in one group
    check(ra_gpu, h, 0, 2, ops=("sum",))
    check(ra_gpu, h, 0, 5, ops=("sum",), lab=np.full(k, 2))    # 4 empty


@pytest.mark.parametrize("ngroups", ["1", "smax", "smax+1", "3*n"])
def test_group_counts_around_select_max(ra_gpu, lib, geo, ngroups):
    n = 2 * geo["gather_chunk"] + 77        # more than two gather chunks
    ng = eval(ngroups, {"smax": geo["select_max"], "n": n})
    for dtype in ("float64", "int32"):
        h = values((n,), dtype)
        assert regime(lib, h, 0, ng) == (LINE_SELECT
                                         if ng <= geo["select_max"]
                                         else LINE_GATHER)
        check(ra_gpu, h, 0, ng, ops=("sum", "max"))
        check(ra_gpu, h, 0, ng + 1, ops=("sum",), lab=np.full(n, ng))
        check(ra_gpu, values((50, 33), dtype), 0, min(ng, 200),
              ops=("sum", "min"))
    h = values((4 * geo["block"] * 4 + 3,), "float32")   # several blocks
    check(ra_gpu, np.tile(h, 5), 0, 3, ops=("sum",))


VIEWS = {
    "reversed_rows": (lambda x: x[::-1], 0),
    "reversed_lanes": (lambda x: x[:, ::-1], 0),
    "transposed": (lambda x: x.T, 1),
    "transposed_line": (lambda x: x.T, 0),
    "offset": (lambda x: x[:, 1:49], 0),     # whole units, misaligned
    "offset_line": (lambda x: x[:, 1:49], 1),
    "step": (lambda x: x[::2, ::3], 0),
}


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("dtype", ["float64", "float32", "int8"])
def test_views(ra_gpu, view, dtype):
    fn, dim = VIEWS[view]
    h = values((48, 64), dtype)
    check(ra_gpu, h, dim, 5, view=fn, ops=("sum", "min"))
    check(ra_gpu, h, dim, 30, view=fn, ops=("sum",))


@pytest.mark.parametrize("src,step,shape,dim", [
    ((33,), 1, (6, 33), 1),             # LINE_SELECT, every line the same
    ((33, 1, 8), 1, (33, 6, 8), 0),     # ROWS, a broadcast outer axis
    ((34, 1), 2, (17, 6), 0)])          # ROWS, the lanes themselves broadcast
def test_zero_stride_broadcast_axis(ra_gpu, src, step, shape, dim):
    h = values(src, "float32")
    view = lambda x: x[::step]
    lab = labels(shape[dim], 4)
    got = view(ra_gpu.fromarray(h)).broadcast_to(shape) \
        .groupby(dim, lab, 4).sum().asarray()
    np.testing.assert_array_equal(
        got, model(np.broadcast_to(view(h), shape), dim, lab, 4, "sum"))


@pytest.mark.filterwarnings("ignore:invalid value encountered")
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,dim,ng", [((40, 12), 0, 3), ((700,), 0, 3),
                                          ((700,), 0, 40)])
def test_nan_inf_and_signed_zero(ra_gpu, shape, dim, ng, dtype):
    h = values(shape, dtype)
    flat = h.reshape(-1)
    flat[::11], flat[5::13], flat[7::17] = np.nan, np.inf, -np.inf
    flat[3::19] = -0.0
    lab = labels(shape[dim], ng)
    check(ra_gpu, h, dim, ng, ops=("min", "max", "sum"), lab=lab)
    total, count = ra_gpu.fromarray(h).groupby(dim, lab, ng) \
        .nanmean(ret_separate=True)
    x = np.moveaxis(h, dim, 0)
    ref_t = np.zeros((ng,) + x.shape[1:], dtype)
    ref_c = np.zeros((ng,) + x.shape[1:], np.int64)
    np.add.at(ref_t, lab, np.where(np.isnan(x), 0, x).astype(dtype))
    np.add.at(ref_c, lab, ~np.isnan(x))
    np.testing.assert_array_equal(total.asarray(), np.moveaxis(ref_t, 0, dim))
    np.testing.assert_array_equal(count.asarray(), np.moveaxis(ref_c, 0, dim))
    assert count.dtype == np.int64


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("want", [ROWS, ROWS_SPLIT, LINE_SELECT, LINE_GATHER])
def test_generic_floats_within_the_summation_bound(ra_gpu, lib, geo, want,
                                                   dtype):
    """|sum - fsum| <= gamma_{n-1} sum|x_i| (Higham, Accuracy and Stability,
    eq. 4.4: any order of n - 1 additions), n the group's size and u the
    dtype's unit roundoff; fsum is the exact sum rounded once to float64, so
    one more u covers the reference's own rounding to the dtype."""
    shape, dim, ng = {ROWS: ((300, 24), 0, 7),
                      ROWS_SPLIT: ((2 * geo["chunk"] + 9, 24), 0, 2),
                      LINE_SELECT: ((5000,), 0, 7),
                      LINE_GATHER: ((5000,), 0, 40)}[want]
    h = np.random.default_rng(want).normal(size=shape).astype(dtype)
    assert regime(lib, h, dim, ng) == want
    lab = labels(shape[dim], ng)
    g = ra_gpu.fromarray(h).groupby(dim, lab, ng)
    got = np.moveaxis(g.sum().asarray(), dim, 0)
    x = np.moveaxis(h, dim, 0)
    u = np.finfo(dtype).eps / 2
    for k in range(ng):
        rows = x[lab == k].astype(np.float64)
        n = len(rows)
        if n == 0:
            assert not got[k].any()
            continue
        exact = np.array([math.fsum(c) for c in rows.reshape(n, -1).T])
        bound = ((n - 1) * u / (1 - (n - 1) * u) + u) \
            * np.abs(rows).reshape(n, -1).sum(axis=0)
        assert np.all(np.abs(got[k].reshape(-1) - exact) <= bound), k
    if want == ROWS:        # sequential, ascending: np.add.at bit for bit
        np.testing.assert_array_equal(g.sum().asarray(),
                                      model(h, dim, lab, ng, "sum"))
    assert np.array_equal(g.sum().asarray(), np.moveaxis(got, 0, dim))
