"""rt_gemm_batched against NumPy through the C ABI (poisoned buffers, guard
elements between and around the slices of C), and the public matmul forms
that run on it and on rt_gemv."""

import ctypes

import numpy as np
import pytest

from ramba_amd.hip_backend import RT_DTYPE
from test_gpu_gemm import DTYPES, POISON, assert_within, be  # noqa: F401
from test_gpu_gemv import odd, place, up4

pytestmark = pytest.mark.gpu

B = 3
VARIANTS = ["dense", "a_shared", "b_shared", "odd", "accumulate"]


def bgemm(be, a, b, c0, variant):
    """rt_gemm_batched on placed buffers (a / b 2-D when shared): C,
    checked to be all that changed."""
    (m, n), k, dtype = c0.shape[1:], a.shape[-1], a.dtype.name
    ld, off = (odd, 1) if variant == "odd" else (up4, 0)
    lda, ldb, ldc = ld(k), ld(n), ld(n)
    a_bs = 0 if a.ndim == 2 else ld(m * lda + 4)
    b_bs = 0 if b.ndim == 2 else ld(k * ldb + 4)
    c_bs = ld(m * ldc + 8)                  # guard rows between the slices
    abuf, aoff, _ = place(a, off, ((a_bs,) if a.ndim == 3 else ()) + (lda, 1))
    bbuf, boff, _ = place(b, off, ((b_bs,) if b.ndim == 3 else ()) + (ldb, 1))
    cbuf, coff, cview = place(c0, off, (c_bs, ldc, 1))
    dev = [be.torch.from_numpy(x).cuda() for x in (abuf, bbuf, cbuf)]
    ptr = [ctypes.c_void_p(t.data_ptr() + o * t.element_size())
           for t, o in zip(dev, (aoff, boff, coff))]
    rc = be.lib.rt_gemm_batched(
        be._stream(), ptr[2], ptr[0], ptr[1], B, m, n, k, lda, 1, ldb, 1, ldc,
        a_bs, b_bs, c_bs, RT_DTYPE[dtype], int(variant == "accumulate"))
    assert rc == 0, be.lib.rt_last_error().decode()
    got = dev[2].cpu().numpy()
    box = np.lib.stride_tricks.as_strided(
        got[coff:], c0.shape, [s * got.itemsize for s in (c_bs, ldc, 1)])
    c = box.copy()
    box[...] = c0
    assert np.array_equal(got, cbuf), "rt_gemm_batched wrote outside C"
    return c


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", range(2))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rt_gemm_batched(be, dtype, case, variant, integer):
    bm, bn, bk = be.gemm_tile(dtype)
    m, n, k = [(1, 1, 1), (bm + 1, bn - 1, bk + 1)][case]
    rng = np.random.default_rng(case)
    draw = (lambda *s: rng.integers(-8, 9, s).astype(dtype)) if integer \
        else (lambda *s: rng.standard_normal(s).astype(dtype))
    a = draw(m, k) if variant == "a_shared" else draw(B, m, k)
    b = draw(k, n) if variant == "b_shared" else draw(B, k, n)
    c0 = draw(B, m, n) if (acc := variant == "accumulate") else np.full((B, m, n), POISON, dtype=dtype)
    got = bgemm(be, a, b, c0, variant)
    for i in range(B):
        ai, bi = a[i] if a.ndim == 3 else a, b[i] if b.ndim == 3 else b
        if integer:     # every partial sum is exactly representable
            want = ai.astype(np.int64) @ bi.astype(np.int64) \
                + (c0[i].astype(np.int64) if acc else 0)
            assert np.array_equal(got[i], want.astype(dtype))
        else:
            assert_within(got[i], ai, bi, dtype, c0[i] if acc else None)


# (shape of a, shape of b, dtype of a); b is float64: float32 must promote
FORMS = [((300, 500), (500,), "float64"), ((500,), (500, 300), "float64"),
         ((3, 130, 70), (3, 70, 50), "float64"),
         ((3, 130, 70), (70, 50), "float64"),
         ((2, 1, 40, 30), (3, 30, 20), "float64"),
         ((70,), (3, 70, 50), "float64"), ((40, 30), (30,), "float32"),
         ((40, 30), (2, 30, 20), "float32")]


@pytest.mark.parametrize("sa,sb,dta", FORMS, ids=str)
def test_matmul_forms_public_path(ra_gpu, sa, sb, dta):
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(sa).astype(dta), rng.standard_normal(sb)
    got = (ra_gpu.fromarray(a) @ ra_gpu.fromarray(b)).asarray()
    want = a @ b
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    a = a.astype(np.float64)
    a2 = a[None] if a.ndim == 1 else a
    b2 = b[:, None] if b.ndim == 1 else b
    batch = np.broadcast_shapes(a2.shape[:-2], b2.shape[:-2])
    a3 = np.broadcast_to(a2, batch + a2.shape[-2:])
    b3 = np.broadcast_to(b2, batch + b2.shape[-2:])
    got = got.reshape(batch + (a2.shape[-2], b2.shape[-1]))
    for i in np.ndindex(*batch):            # the bound, product by product
        assert_within(got[i], a3[i], b3[i], "float64")


# peak growth under a quarter of A (A @ x) / of the B.M.K.N temporary
@pytest.mark.parametrize("sa,sb,limit", [
    ((2048, 2048), (2048,), 2048 ** 2 * 8 // 4),
    ((4, 128, 128), (4, 128, 128), 4 * 128 ** 3 * 8 // 4)], ids=str)
def test_matmul_forms_build_no_product_temporary(ra_gpu, be, sa, sb, limit):
    ra, torch = ra_gpu, be.torch
    A = ra.fromfunction(lambda *i: (sum(i) - 2 * i[0]) * 1e-3, sa)
    Bm = ra.fromfunction(lambda *i: (sum(i) + i[-1]) * 1e-3, sb)
    ra.sync()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    C = A @ Bm
    ra.sync()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print("peak allocation grew by", grew, "bytes")
    assert grew < limit and C.size
