"""The generated kernels' scalar helpers (codegen.PREAMBLE: rt_sincos,
rt_ffloordiv, rt_fmod, rt_fdiv, rt_imod), compiled for the HOST from the
very text the GPU kernels get, and checked against the correctly rounded
fixtures in tests/golden/numeric/.

No GPU: the text is wrapped with empty __device__ / __forceinline__
definitions and batch entry points, built with the ROCm clang++ using
-O2 -ffp-contract=off (the contraction setting rt_kernel_get passes to
hiprtc) and loaded with ctypes.  This runs the polynomial, all three
Cody-Waite stages, the quadrant switch for negative n and the NumPy
floor_divide / remainder algorithm on every CPU run; only rt_sincos'
|x| >= 1e6 hand-off differs from the device (libm here, ocml there).
"""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from ramba_amd import codegen

from numeric_util import assert_exact, fixture, spacings

WRAPPER = r"""
#include <math.h>
#define __device__
#define __forceinline__ inline
%s
extern "C" {
void b_sincos(const double *x, double *s, double *c, long n) {
    for (long i = 0; i < n; ++i) rt_sincos(x[i], s + i, c + i);
}
void b_ffloordiv(const double *a, const double *b, double *o, long n) {
    for (long i = 0; i < n; ++i) o[i] = rt_ffloordiv(a[i], b[i]);
}
void b_ffloordivf(const float *a, const float *b, float *o, long n) {
    for (long i = 0; i < n; ++i) o[i] = rt_ffloordivf(a[i], b[i]);
}
void b_fmod(const double *a, const double *b, double *o, long n) {
    for (long i = 0; i < n; ++i) o[i] = rt_fmod(a[i], b[i]);
}
void b_fmodf(const float *a, const float *b, float *o, long n) {
    for (long i = 0; i < n; ++i) o[i] = rt_fmodf(a[i], b[i]);
}
void b_fdiv(const i64 *a, const i64 *b, i64 *o, long n) {
    for (long i = 0; i < n; ++i) o[i] = rt_fdiv(a[i], b[i]);
}
void b_imod(const i64 *a, const i64 *b, i64 *o, long n) {
    for (long i = 0; i < n; ++i) o[i] = rt_imod(a[i], b[i]);
}
}
"""


def _find_clangxx():
    """The clang++ of the ROCm installation whose hipcc build() uses."""
    roots = []
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(
            os.path.realpath(hipcc))))
    roots += [os.environ.get("ROCM_PATH", ""), "/opt/rocm"]
    for r in roots:
        for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++",
                    "bin/amdclang++"):
            p = os.path.join(r, sub) if r else ""
            if p and os.path.isfile(p) and os.access(p, os.X_OK):
                return p
    return shutil.which("amdclang++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _find_clangxx()
    if cxx is None:
        pytest.skip("no ROCm clang++ found")
    d = tmp_path_factory.mktemp("preamble_host")
    src = d / "preamble_host.cpp"
    src.write_text(WRAPPER % codegen.PREAMBLE)
    so = d / "preamble_host.so"
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC",
                    "-shared", str(src), "-o", str(so), "-lm"], check=True)
    return ctypes.CDLL(str(so))


def _call(host, name, dtype, *ins, nout=1):
    ins = [np.ascontiguousarray(a, dtype=dtype) for a in ins]
    outs = [np.empty_like(ins[0]) for _ in range(nout)]
    ptr = ctypes.c_void_p
    getattr(host, name)(*[ptr(a.ctypes.data) for a in ins + outs],
                        ctypes.c_long(ins[0].size))
    return outs[0] if nout == 1 else outs


def test_rt_sincos_against_correctly_rounded(host):
    z = fixture("sincos")
    x = z["x64"]
    s, c = _call(host, "b_sincos", np.float64, x, nout=2)
    fast = np.abs(x) < 1.0e6
    # the third Cody-Waite stage's witness must be part of the input
    assert float.fromhex("0x1.6c6cbc45dc8dep+5") in x
    for got, want in ((s, z["sin64"]), (c, z["cos64"])):
        d = spacings(got, want)
        print("rt_sincos host: fast max", d[fast].max(),
              "fallback max", d[~fast].max())
        assert d[fast].max() <= 1.0      # fdlibm's bound for this algorithm
        assert d[~fast].max() <= 4.0     # sincos hand-off (OpenCL bound)
        ok = ~np.isnan(want)
        assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
    # sin(-0.0) is -0.0, sin(+0.0) is +0.0
    s0, _ = _call(host, "b_sincos", np.float64, np.array([-0.0, 0.0]),
                  nout=2)
    assert np.signbit(s0[0]) and not np.signbit(s0[1])


@pytest.mark.parametrize("tag,dtype,sfx", [("64", np.float64, ""),
                                           ("32", np.float32, "f")])
def test_float_floordiv_mod_match_numpy(host, tag, dtype, sfx):
    z = fixture("binary")
    a, b = z["a" + tag], z["b" + tag]
    assert_exact(_call(host, "b_ffloordiv" + sfx, dtype, a, b),
                 z["floordiv" + tag])
    assert_exact(_call(host, "b_fmod" + sfx, dtype, a, b), z["mod" + tag])
    with np.errstate(all="ignore"):
        # the fixture records NumPy; it must still be what NumPy computes
        assert_exact(np.floor_divide(a, b), z["floordiv" + tag])
        assert_exact(np.mod(a, b), z["mod" + tag])
        # and it separates NumPy's algorithm from floor(a / b)
        naive = np.floor(a / b)
    want = z["floordiv" + tag]
    differ = ~((naive == want) | (np.isnan(naive) & np.isnan(want)))
    assert differ.sum() > 1000


def test_int_floordiv_mod_zero_divisor_and_overflow(host):
    lo = np.iinfo(np.int64).min
    v = np.array([0, 1, -1, 2, -2, 7, -7, 10, lo, lo + 1,
                  np.iinfo(np.int64).max], dtype=np.int64)
    a, b = [m.ravel() for m in np.meshgrid(v, v, indexing="ij")]
    with np.errstate(all="ignore"):
        want_q, want_r = np.floor_divide(a, b), np.mod(a, b)
    q = _call(host, "b_fdiv", np.int64, a, b)
    r = _call(host, "b_imod", np.int64, a, b)
    assert np.array_equal(q, want_q)
    assert np.array_equal(r, want_r)
    zero = b == 0
    assert not q[zero].any() and not r[zero].any()
    m1 = (a == lo) & (b == -1)
    assert q[m1][0] == lo and r[m1][0] == 0
