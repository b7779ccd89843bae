"""rt_group_reduce validates its arguments on the host before any HIP call;
runs without a GPU: every call here fails validation or has a zero extent."""

import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.skip("libramba_rt.so not built")
    return hip_backend._load_lib()


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


P = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)  # never read
ONES = i64(1, 1, 1, 1)
NULL64 = ctypes.POINTER(ctypes.c_int64)()
REJECTED = [
    (dict(nd=0), "nd out of range"), (dict(nd=5), "nd out of range"),
    (dict(shp=NULL64), "NULL shape"), (dict(strides=None), "NULL strides"),
    (dict(ostr=None), "NULL strides"),
    (dict(shape=(-1,)), "negative extent"),
    (dict(shape=(1 << 40,)), "out of range"),
    (dict(nd=2, shape=(1 << 39, 1 << 39)), "shape too large"),
    (dict(axis=-1), "axis out of range"), (dict(axis=1), "axis out of range"),
    (dict(dtype=-1), "bad dtype"), (dict(dtype=7), "bad dtype"),
    (dict(op=-1), "bad op"), (dict(op=5), "bad op"),
    (dict(ng=0), "ngroups < 1"), (dict(ng=1 << 31), "ngroups out of range"),
    (dict(shape=(1 << 31,)), "too long for int32 members"),
    (dict(nd=2, shape=(4, 1 << 30), ng=1 << 20), "result too large"),
    (dict(in_=None), "NULL in"), (dict(members=None), "NULL members"),
    (dict(seg=None), "NULL seg"), (dict(out=None), "NULL out"),
    (dict(scratch=None), "NULL scratch"),            # 1-D: LINE_SELECT
    (dict(scratch=ctypes.c_void_p(P.value + 8)), "not 16-byte aligned"),
]


def call(lib, nd=1, shape=(4,), shp=None, strides=ONES, ostr=ONES, axis=0,
         dtype=0, op=0, ng=2, in_=P, members=P, seg=P, out=P, scratch=P):
    return lib.rt_group_reduce(
        0, in_, 0, nd, i64(*shape) if shp is None else shp, strides, axis,
        dtype, op, 0, members, seg, ng, out, ostr, scratch)


@pytest.mark.parametrize("kw,what", REJECTED)
def test_rejected_argument_is_named(lib, kw, what):
    rc = call(lib, **kw)
    msg = lib.rt_last_error().decode()
    assert rc != 0, f"rt_group_reduce accepted a call that should fail: {what}"
    assert msg.startswith("rt_group_reduce:") and what in msg, msg


def test_zero_extent_regimes_and_scratch(lib):
    from ramba_amd.hip_backend import group_geometry
    assert call(lib, shape=(0,), in_=None, out=None, members=None) == 0
    assert call(lib, nd=3, shape=(3, 0, 1 << 30), axis=2, in_=None) == 0
    g = group_geometry(lib)
    assert g["block"] == 256 and g["chunk"] >= g["member_tile"] >= 1
    k = 2 * g["chunk"] + 1

    def regime(shape, strides, axis, ng):
        return lib.rt_group_regime(len(shape), i64(*shape), i64(*strides),
                                   axis, 1, ng)
    # ROWS, ROWS_SPLIT at its row threshold, and the two LINE regimes at
    # select_max (a transposed box puts the unit stride on the group axis)
    smax = g["select_max"]
    assert [regime((k - 1, 8), (8, 1), 0, 2), regime((k, 8), (8, 1), 0, 2),
            regime((k, 8), (1, k), 0, 2), regime((k,), (1,), 0, smax),
            regime((k,), (-1,), 0, smax + 1)] == [0, 1, 2, 2, 3]
    assert regime((k, 256 * g["split_blocks"]), (256 * g["split_blocks"], 1),
                  0, 1) == 0                     # enough tiles: no split
    assert regime((4,), (1,), 1, 2) == -1
    scratch = lib.rt_group_scratch
    assert scratch(2, i64(9, 8), i64(8, 1), 0, 1, 0, 3) == 0
    assert scratch(2, i64(k, 8), i64(8, 1), 0, 1, 0, 2) \
        == (k // g["chunk"] + 2) * 8 * 4
    assert scratch(1, i64(k), i64(1), 0, 5, 0, 2) % 16 == k % 16   # + labels
    assert scratch(1, i64(k), i64(1), 0, 7, 0, 2) == -1
