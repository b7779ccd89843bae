"""rt_gemv against NumPy through the C ABI, at shapes from the geometry of
the kernel each layout selects; A, x, y and the scratch live in poisoned
buffers with guard bands, so a stray read or write shows."""

import ctypes

import numpy as np
import pytest

from ramba_amd.hip_backend import RT_DTYPE
from test_gpu_gemm import DTYPES, G, POISON, assert_within, be  # noqa: F401

pytestmark = pytest.mark.gpu

# layout -> (kernel regime, A's (row, column) strides for an M x K matrix)
up4 = lambda n: -(-n // 4) * 4
odd = lambda n: n + 1 + n % 2
LAYOUTS = {"k_aligned": (0, 0, lambda m, k: (up4(k), 1)),
           "k_odd": (1, 1, lambda m, k: (odd(k), 1)),
           "m_aligned": (2, 0, lambda m, k: (1, up4(m))),
           "m_odd": (3, 1, lambda m, k: (1, odd(m))),
           "strided": (3, 3, lambda m, k: (2 * k + 1, 2))}
# (layout, accumulate, ksplit); 7 is above the k steps of every shape
VARIANTS = [("k_aligned", 0, 1), ("k_odd", 0, 1), ("m_aligned", 0, 1),
            ("m_odd", 0, 1), ("strided", 0, 1), ("k_aligned", 1, 1),
            ("k_aligned", 0, 3), ("m_aligned", 1, 3), ("k_odd", 0, 7),
            ("m_odd", 1, 7)]


def shape_of(be, dtype, layout, case):
    r, s = be.gemv_geometry(dtype, LAYOUTS[layout][0])
    return [(1, 1), (r + 1, s - 1), (2 * r + 3, 2 * s + 5),
            (3, 4 * s + 1)][case]


def place(data, off, strides):
    """`data` at element G + off of a poisoned buffer, G guards after it."""
    span = sum((n - 1) * s for n, s in zip(data.shape, strides)) + 1
    buf = np.full(2 * G + off + span, POISON, dtype=data.dtype)
    view = np.lib.stride_tricks.as_strided(
        buf[G + off:], data.shape, [s * data.itemsize for s in strides])
    view[...] = data
    return buf, G + off, view


def gemv(be, a, x, y0, variant):
    """rt_gemv on placed buffers: y, checked to be all that changed."""
    layout, acc, ks = variant
    (m, k), dtype = a.shape, a.dtype.name
    _, off, strides = LAYOUTS[layout]
    a_rs, a_cs = strides(m, k)
    vs = 2 if layout == "strided" else 1
    abuf, aoff, _ = place(a, off, (a_rs, a_cs))
    xbuf, xoff, _ = place(x, off, (vs,))
    ybuf, yoff, yview = place(y0, off, (vs,))
    dev = [be.torch.from_numpy(b).cuda() for b in (abuf, xbuf, ybuf)]
    ptr = [ctypes.c_void_p(t.data_ptr() + o * t.element_size())
           for t, o in zip(dev, (aoff, xoff, yoff))]
    scratch = be.torch.full((ks * m,), POISON, dtype=dev[0].dtype,
                            device="cuda")
    rc = be.lib.rt_gemv(be._stream(), ptr[2], ptr[0], ptr[1], m, k, a_rs,
                        a_cs, vs, vs, RT_DTYPE[dtype], acc, ks,
                        ctypes.c_void_p(scratch.data_ptr()))
    assert rc == 0, be.lib.rt_last_error().decode()
    yview[...] = POISON
    got = dev[2].cpu().numpy()
    y = got[yoff:yoff + (m - 1) * vs + 1:vs].copy()
    got[yoff:yoff + (m - 1) * vs + 1:vs] = POISON
    assert np.array_equal(got, ybuf), "rt_gemv wrote outside y"
    return y


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
@pytest.mark.parametrize("variant", VARIANTS, ids=str)
@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rt_gemv(be, dtype, case, variant, integer):
    m, k = shape_of(be, dtype, variant[0], case)
    rng = np.random.default_rng(case)
    draw = (lambda s: rng.integers(-8, 9, s).astype(dtype)) if integer \
        else (lambda s: rng.standard_normal(s).astype(dtype))
    a, x, y0 = draw((m, k)), draw(k), draw(m)
    got = gemv(be, a, x, y0, variant)
    if integer:         # every partial sum is exactly representable
        want = a.astype(np.int64) @ x.astype(np.int64) \
            + (y0.astype(np.int64) if variant[1] else 0)
        assert np.array_equal(got, want.astype(dtype))
    else:
        assert_within(got[:, None], a, x[:, None], dtype,
                      y0[:, None] if variant[1] else None)


@pytest.mark.parametrize("layout", list(LAYOUTS)[:4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rt_gemv_nonfinite_in_the_k_tail(be, dtype, layout):
    # K = S + 1: the inf of x is alone in the K tail
    r, s = be.gemv_geometry(dtype, LAYOUTS[layout][0])
    m, k = r + 1, s + 1
    rng = np.random.default_rng(7)
    a, x, y0 = (rng.standard_normal(s).astype(dtype) for s in ((m, k), k, m))
    x[-1] = np.inf
    a[m // 2, 3] = np.nan
    got = gemv(be, a, x, y0, (layout, 0, 1))
    with np.errstate(invalid="ignore"):
        want = a @ x
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    assert np.array_equal(np.isinf(got), np.isinf(want))


@pytest.mark.parametrize("layout", ["k_aligned", "m_aligned"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rt_gemv_ksplit_gives_the_same_bits_every_run(be, dtype, layout):
    m, k = shape_of(be, dtype, layout, 2)
    a, x, y0 = (np.random.default_rng(3).standard_normal(s).astype(dtype)
                for s in ((m, k), k, m))
    runs = [gemv(be, a, x, y0, (layout, 0, 3)) for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()
