"""rt_select_pass validates its arguments on the host before any HIP call,
and rt_sort_decode inverts rt_sort_canon; runs without a GPU: every call here
fails validation or has a zero extent."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.skip("libramba_rt.so not built")
    return hip_backend._load_lib()


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


P = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)  # never read
NULL64 = ctypes.POINTER(ctypes.c_int64)()
REJECTED = [
    (dict(nd=0), "nd out of range"), (dict(nd=5), "nd out of range"),
    (dict(shp=NULL64), "NULL shape"), (dict(strides=None), "NULL strides"),
    (dict(shape=(-1,)), "negative extent"),
    (dict(shape=(1 << 40,)), "out of range"),
    (dict(nd=2, shape=(1 << 39, 1 << 39)), "shape too large"),
    (dict(dtype=-1), "bad dtype"), (dict(dtype=7), "bad dtype"),
    (dict(shift=-8), "bad shift"), (dict(shift=4), "bad shift"),
    (dict(shift=64), "bad shift"), (dict(dtype=3, shift=32), "bad shift"),
    (dict(dtype=6, shift=8), "bad shift"),
    (dict(nq=0), "nq out of range"), (dict(nq=9), "nq out of range"),
    (dict(pre=None), "NULL prefixes"),
    (dict(shift=40, pre=(1 << 47,)), "outside the decided digits"),
    (dict(dtype=3, shift=8, pre=(1 << 32,)), "outside the decided digits"),
    (dict(shift=56, pre=(1,)), "outside the decided digits"),
    (dict(shift=40, nq=2, pre=(1 << 48, 1 << 48)), "duplicate prefix"),
    (dict(buf=P, cursor=None), "collect buffer without a cursor"),
    (dict(cap=-1), "negative collect_cap"),
    (dict(canonical=1, nd=2, shape=(2, 2)), "dense 1-D run"),
    (dict(canonical=1, strides=i64(2)), "dense 1-D run"),
    (dict(in_=None), "NULL in"), (dict(counts=None), "NULL counts"),
]


def call(lib, nd=1, shape=(4,), shp=None, strides=i64(1, 1, 1, 1), dtype=2,
         canonical=0, shift=56, nq=1, pre=(0,), in_=P, counts=P, buf=None,
         cap=0, cursor=P):
    pre = None if pre is None else (ctypes.c_uint64 * len(pre))(*pre)
    return lib.rt_select_pass(
        0, in_, 0, nd, i64(*shape) if shp is None else shp, strides, dtype,
        canonical, shift, nq, pre, counts, None, buf, cap, cursor)


@pytest.mark.parametrize("kw,what", REJECTED)
def test_rejected_argument_is_named(lib, kw, what):
    rc = call(lib, **kw)
    msg = lib.rt_last_error().decode()
    assert rc != 0, f"rt_select_pass accepted a call that should fail: {what}"
    assert msg.startswith("rt_select_pass:") and what in msg, msg


def test_zero_extent_and_geometry(lib):
    assert call(lib, shape=(0,), in_=None, counts=None) == 0
    assert call(lib, nd=3, shape=(3, 0, 1 << 39), shift=0, nq=2,
                pre=(1 << 8, 2 << 8), in_=None) == 0
    from ramba_amd.hip_backend import select_geometry
    assert select_geometry(lib) == {"grid_cap": select_geometry(lib)[
        "grid_cap"], "block": 256, "nq_max": 8, "digit_bits": 8}


TABLE = r"""
#include <cstdio>
#include <cstring>
#include "ramba_sortkey.h"
template <typename T> int run(const char *name, const T *v, int n) {
    typedef typename rt_sort_key<T>::U U;
    for (int i = 0; i < n; ++i) {
        U raw, back;
        memcpy(&raw, &v[i], sizeof(T));
        const U key = rt_sort_canon<T>(raw);
        back = rt_sort_decode<T>(key);
        printf("%s %llu %llu %llu\n", name, (unsigned long long)raw,
               (unsigned long long)key, (unsigned long long)back);
    }
    return 0;
}
int main() {
    const double d[] = {0.0, -0.0, 1.5, -1.5, 1e308, -1e308, 5e-324, -5e-324,
                        __builtin_inf(), -__builtin_inf(), __builtin_nan(""),
                        -__builtin_nan("7")};
    const float f[] = {0.f, -0.f, 1.5f, -1.5f, 3e38f, -3e38f, 1e-45f, -1e-45f,
                       __builtin_inff(), -__builtin_inff(),
                       __builtin_nanf(""), -__builtin_nanf("7")};
    const int64_t l[] = {0, -1, 1, INT64_MIN, INT64_MAX, (1LL << 53) + 1};
    const int16_t s[] = {0, -1, 1, INT16_MIN, INT16_MAX};
    const uint8_t u[] = {0, 1, 128, 255};
    return run("float64", d, 12) | run("float32", f, 12) | run("int64", l, 6)
           | run("int16", s, 5) | run("uint8", u, 4);
}
"""


def test_decode_inverts_canon_in_the_header_and_in_numpy(tmp_path):
    """The header, compiled for the host, and selection.canon / decode agree
    on a value table: decode(canon(x)) is x, but +0.0 for a zero and the
    default NaN for a NaN, and canon(decode(k)) is k."""
    from ramba_amd import selection
    (tmp_path / "t.cpp").write_text(TABLE)
    subprocess.run(["c++", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "t.cpp", "-o", "t"], check=True, cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "t")], check=True,
                         capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    assert len(rows) == 39
    for name, raw, key, back in rows:
        U = selection.key_dtype(name)
        x = np.array([int(raw)], dtype=U).view(name)
        assert int(selection.canon(x)[0]) == int(key), (name, x)
        got = selection.decode(int(key), name)
        assert got.dtype == x.dtype and got.view(U) == int(back), (name, x)
        assert int(selection.canon(np.array([got]))[0]) == int(key)
        want = x[0] + x.dtype.type(0)               # -0.0 + 0.0 is +0.0
        if x.dtype.kind == "f" and np.isnan(x[0]):
            assert np.isnan(got) and not np.signbit(got)
        else:
            assert got == want and np.signbit(got) == np.signbit(want)
