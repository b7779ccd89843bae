"""2-D matmul over CPU ranks (gloo, worlds 1, 2 and 4): the ring schedule of
runtime.matmul_op on the oracle backend with the portable host hooks, and
the host-side argument validation of rt_gemm (no GPU: every call there
fails validation or has nothing to launch).  Integer-valued data, so every
comparison is array_equal.
"""

import ctypes
import os

import pytest

from test_take_gloo import run_spmd

# (M, K, N): odd everything; M < world; K < world; even split
SHAPES = [(7, 5, 3), (2, 9, 4), (9, 2, 4), (8, 8, 8)]

BODY = """
    from ramba_amd import runtime
    calls, op = [], runtime.Runtime.matmul_op
    runtime.Runtime.matmul_op = lambda *a: calls.append(1) or op(*a)
    rng = np.random.default_rng(5)
    a = rng.integers(-8, 9, ({m}, {k})).astype(np.{dtype})
    b = rng.integers(-8, 9, ({k}, {n})).astype(np.{dtype})
    A, B = (a, b) if np_ is np else (np_.fromarray(a), np_.fromarray(b))
    C = A @ B
    assert np_ is np or calls, "A @ B did not reach matmul_op"
    return C
"""


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("m,k,n,dtype", [s + ("float64",) for s in SHAPES]
                         + [(7, 5, 3, "float32")])
def test_matmul_ring(world, m, k, n, dtype):
    run_spmd(BODY.format(m=m, k=k, n=n, dtype=dtype), world=world)


@pytest.mark.parametrize("world", [1, 2])
def test_matmul_operand_forms(world):
    # promotion, a sliced transposed operand, np.dot / ndarray.dot, K == 0
    # (each of the three products must reach matmul_op; K == 0 must not)
    run_spmd("""
        from ramba_amd import runtime
        calls, op = [], runtime.Runtime.matmul_op
        runtime.Runtime.matmul_op = lambda *a: calls.append(1) or op(*a)
        a = np_.arange(42).reshape(6, 7) * 1.0
        b = (np_.arange(30).reshape(6, 5) % 7).astype(np.float32)
        z = np_.zeros((5, 0)) @ np_.zeros((0, 3))
        parts = [a.T[1:] @ b, np.dot(a.T, b)[1:], a.T.dot(b)[:6], z.T]
        runtime.Runtime.matmul_op = op
        assert np_ is np or len(calls) == 3, calls
        return np_.concatenate(parts)
    """, world=world)


@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.fail(f"{hip_backend.LIBPATH} not built (run build())")
    return hip_backend._load_lib()


def test_rt_gemm_rejects_bad_arguments(lib):
    buf = (ctypes.c_double * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p)      # non-NULL, never read

    def call(c=P, a=P, b=P, M=4, N=4, K=4, ldc=4, dtype=0, acc=0):
        return lib.rt_gemm(0, c, a, b, M, N, K, K, 1, N, 1, ldc, dtype, acc)

    for kw, what in [(dict(M=-1), "negative extent"),
                     (dict(N=-1), "negative extent"),
                     (dict(K=-1), "negative extent"),
                     (dict(M=1 << 40), "out of range"),
                     (dict(K=1 << 40), "out of range"),
                     (dict(M=1 << 39, N=1 << 39, ldc=1 << 39), "too large"),
                     (dict(M=1 << 39, K=1 << 39), "too large"),
                     (dict(K=1 << 39, N=1 << 39, ldc=1 << 39), "too large"),
                     (dict(c=None), "NULL c"), (dict(a=None), "NULL a/b"),
                     (dict(b=None), "NULL a/b"), (dict(ldc=3), "ldc < N"),
                     (dict(dtype=2), "bad dtype"), (dict(dtype=-1), "bad dtype"),
                     (dict(acc=2), "bad accumulate"),
                     (dict(acc=-1), "bad accumulate")]:
        assert call(**kw) != 0, kw
        msg = lib.rt_last_error().decode()
        assert msg.startswith("rt_gemm:") and what in msg, (kw, msg)
    # nothing to do: no launch, NULL data allowed
    assert call(M=0, c=None, a=None, b=None) == 0
    assert call(N=0, ldc=0, c=None) == 0
    assert call(K=0, acc=1, a=None, b=None) == 0


def test_rt_gemm_tile_is_whole_mfma_shapes(lib):
    for dtype, (tm, tk) in ((0, (16, 4)), (1, (32, 2))):
        t = [ctypes.c_int() for _ in range(3)]
        assert lib.rt_gemm_tile(dtype, *map(ctypes.byref, t)) == 0
        bm, bn, bk = (x.value for x in t)
        assert min(bm, bn, bk) > 0
        assert bm % tm == 0 and bn % tm == 0 and bk % tk == 0
    assert lib.rt_gemm_tile(2, *map(ctypes.byref, t)) != 0
    assert "rt_gemm_tile: bad dtype" in lib.rt_last_error().decode()
