"""rt_gemm (the MFMA GEMM kernel) against NumPy, and `A @ B` on top of it.

Shapes follow rt_gemm_tile(): one element, one past / one short of every tile
side, a second grid row and column, two full K trips plus a tail.  Operands
and C are carved out of larger poisoned allocations, so a read outside an
operand corrupts the product and a write outside C shows in the guards.
Every box is checked to lie inside its allocation before the launch.
"""

import ctypes

import numpy as np
import pytest

from ramba_amd.hip_backend import RT_DTYPE

pytestmark = pytest.mark.gpu

G = 64                          # guard elements at both ends of a buffer
POISON = -12345.0
DTYPES = ["float32", "float64"]
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}      # unit roundoff
WIDE = {"float32": np.float64, "float64": np.longdouble}
VARIANTS = ["aligned", "strided", "transposed", "accumulate"]


@pytest.fixture(scope="module")
def be(ra_gpu):
    from ramba_amd import deferred
    return deferred.get_runtime().backend


def shape_of(be, dtype, case):
    bm, bn, bk = be.gemm_tile(dtype)
    return [(1, 1, 1), (bm + 1, bn - 1, bk + 1), (2 * bm + 3, 17, 2 * bk + 5),
            (5, 2 * bn + 1, 1)][case]


def carve(data, off, ld, transposed=False):
    """A poisoned flat buffer holding `data` at element offset G + off with
    leading dimension ld (stored transposed if asked): (buffer, offset of
    element (0,0), row stride, column stride)."""
    rows, cols = data.T.shape if transposed else data.shape
    assert ld >= cols
    buf = np.full(2 * G + off + rows * ld, POISON, dtype=data.dtype)
    box = buf[G + off:G + off + rows * ld].reshape(rows, ld)[:, :cols]
    box[...] = data.T if transposed else data
    return buf, G + off, (1, ld) if transposed else (ld, 1)


def gemm(be, a, b, c0, variant):
    """Run rt_gemm on carved buffers; returns C after checking that nothing
    but the M x N box of its buffer changed."""
    (m, k), n = a.shape, b.shape[1]
    dtype = a.dtype.name
    up4 = lambda x: -(-x // 4) * 4               # rows stay 16-byte aligned
    odd = lambda x: x + 1 + x % 2
    # The four kernels, by (A loads, B loads).  aligned: (16-byte, 16-byte).
    # strided: transposed A, B and an odd-ldc C at odd offsets (element,
    # element).  transposed: transposed A alone (element, 16-byte).
    # accumulate: B at an odd offset with an odd stride (16-byte, element),
    # C += A @ B.
    if variant in ("strided", "transposed"):
        abuf, aoff, (a_rs, a_cs) = carve(a, 1, odd(m), transposed=True)
    else:
        abuf, aoff, (a_rs, a_cs) = carve(a, 0, up4(k))
    if variant == "strided":
        cbuf, coff, (ldc, _) = carve(c0, 3, odd(n))
    else:
        cbuf, coff, (ldc, _) = carve(c0, 0, up4(n))
    if variant in ("strided", "accumulate"):
        bbuf, boff, (b_rs, b_cs) = carve(b, 1, odd(n))
    else:
        bbuf, boff, (b_rs, b_cs) = carve(b, 0, up4(n))
    for size, off, ext, st in ((abuf.size, aoff, (m, k), (a_rs, a_cs)),
                               (bbuf.size, boff, (k, n), (b_rs, b_cs)),
                               (cbuf.size, coff, (m, n), (ldc, 1))):
        last = off + (ext[0] - 1) * st[0] + (ext[1] - 1) * st[1]
        assert G <= off and last < size - G, (variant, off, last, size)
    dev = [be.torch.from_numpy(x).cuda() for x in (abuf, bbuf, cbuf)]
    ptr = [ctypes.c_void_p(t.data_ptr() + o * t.element_size())
           for t, o in zip(dev, (aoff, boff, coff))]
    rc = be.lib.rt_gemm(be._stream(), ptr[2], ptr[0], ptr[1], m, n, k, a_rs,
                        a_cs, b_rs, b_cs, ldc, RT_DTYPE[dtype],
                        int(variant == "accumulate"))
    assert rc == 0, be.lib.rt_last_error().decode()
    got = dev[2].cpu().numpy()
    box = got[coff:coff + m * ldc].reshape(m, ldc)[:, :n].copy()
    got[coff:coff + m * ldc].reshape(m, ldc)[:, :n] = c0
    assert np.array_equal(got, cbuf), "rt_gemm wrote outside C"
    return box


def c_start(rng, m, n, dtype, variant, integer):
    if variant != "accumulate":
        return np.full((m, n), POISON, dtype=dtype)
    if integer:
        return rng.integers(-8, 9, (m, n)).astype(dtype)
    return rng.standard_normal((m, n)).astype(dtype)


def assert_within(c, a, b, dtype, c0=None):
    """|C - ref| <= K u (|A| @ |B|): the forward error bound of a length-K
    dot product summed in any order.  With a start value C0 the sum has one
    more term: (K + 1) u (|C0| + |A| @ |B|)."""
    w = WIDE[dtype]
    ref, mag, terms = a.astype(w) @ b.astype(w), abs(a).astype(w) @ abs(
        b).astype(w), a.shape[1]
    if c0 is not None:
        ref, mag, terms = ref + c0.astype(w), mag + abs(c0).astype(w), terms + 1
    err = np.abs(c.astype(w) - ref)
    print(dtype, a.shape, b.shape, "max err / bound:",
          float(np.max(err / np.maximum(terms * U[dtype] * mag, 1e-300))))
    assert np.all(err <= terms * U[dtype] * mag)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rt_gemm_exact_on_small_integers(be, dtype, case, variant):
    # every partial sum is exactly representable: any order gives these bits
    m, n, k = shape_of(be, dtype, case)
    rng = np.random.default_rng(case)
    a = rng.integers(-8, 9, (m, k))
    b = rng.integers(-8, 9, (k, n))
    c0 = c_start(rng, m, n, dtype, variant, integer=True)
    want = a @ b + (c0.astype(np.int64) if variant == "accumulate" else 0)
    got = gemm(be, a.astype(dtype), b.astype(dtype), c0, variant)
    assert np.array_equal(got, want.astype(dtype))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rt_gemm_rounding_bound(be, dtype, case, variant):
    m, n, k = shape_of(be, dtype, case)
    rng = np.random.default_rng(10 + case)
    a = rng.standard_normal((m, k)).astype(dtype)
    b = rng.standard_normal((k, n)).astype(dtype)
    c0 = c_start(rng, m, n, dtype, variant, integer=False)
    got = gemm(be, a, b, c0, variant)
    assert_within(got, a, b, dtype, c0 if variant == "accumulate" else None)


@pytest.mark.parametrize("variant", ["aligned", "strided"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rt_gemm_nonfinite_in_the_k_tail(be, dtype, variant):
    # K = BK + 1: the inf row of B is alone in the K tail, where a one-sided
    # zero fill would multiply it by whatever lies beside A
    m, n, k = shape_of(be, dtype, 1)
    rng = np.random.default_rng(7)
    a = rng.standard_normal((m, k)).astype(dtype)
    b = rng.standard_normal((k, n)).astype(dtype)
    b[-1, :] = np.inf
    a[m // 2, 3] = np.nan
    got = gemm(be, a, b, c_start(rng, m, n, dtype, variant, False), variant)
    with np.errstate(invalid="ignore"):
        want = a @ b
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf)
    assert np.array_equal(got[inf], want[inf])


def test_matmul_public_path(ra_gpu):
    ra = ra_gpu
    rng = np.random.default_rng(3)
    a = rng.standard_normal((300, 500))
    b = rng.standard_normal((500, 200))
    A, B = ra.fromarray(a), ra.fromarray(b)
    assert_within((A @ B).asarray(), a, b, "float64")
    a32 = a.astype(np.float32)
    c = (ra.fromarray(a32) @ B).asarray()
    assert c.dtype == np.float64
    assert_within(c, a32.astype(np.float64), b, "float64")
    at = rng.standard_normal((500, 301))
    assert_within((ra.fromarray(at).T[1:] @ B).asarray(), at.T[1:], b,
                  "float64")


def test_matmul_materialises_no_mkn_temporary(ra_gpu, be):
    ra, torch, n = ra_gpu, be.torch, 512
    A = ra.fromfunction(lambda i, j: (i - j) * 1e-3, (n, n))
    B = ra.fromfunction(lambda i, j: (i + 2 * j) * 1e-3, (n, n))
    ra.sync()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    C = A @ B
    ra.sync()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print("peak allocation grew by", grew, "bytes")
    assert grew < n ** 3 * 8 // 4
    assert C.shape == (n, n)
