"""runtime.matvec_op / vecmat_op / bmm_op over CPU ranks (gloo, oracle
backend, integer-valued data), and the host-side validation of rt_gemv,
rt_gemv_plan and rt_gemm_batched (nothing there launches)."""

import ctypes

import pytest

from test_gemm_gloo import lib  # noqa: F401  (fixture)
from test_take_gloo import run_spmd

COUNT = """
    from ramba_amd import runtime
    calls = []
    def counted(name):
        op = getattr(runtime.Runtime, name)
        setattr(runtime.Runtime, name,
                lambda *a: calls.append(name) or op(*a))
    [counted(n) for n in ("matvec_op", "vecmat_op", "bmm_op")]
    rng = np.random.default_rng(11)
    def mk(*shape, dtype=np.float64):
        x = rng.integers(-8, 9, shape).astype(dtype)
        return x if np_ is np else np_.fromarray(x)
"""

# (a, b, op to reach): M, K, N and batch under the world of 4; odd extents
FORMS = [((7, 5), (5,), "matvec_op"), ((2, 9), (9,), "matvec_op"),
         ((9, 3), (3,), "matvec_op"), ((5,), (5, 7), "vecmat_op"),
         ((3,), (3, 9), "vecmat_op"), ((9,), (9, 2), "vecmat_op"),
         ((5, 3, 4), (5, 4, 2), "bmm_op"), ((3, 2, 5), (5, 3), "bmm_op"),
         ((2, 1, 3, 4), (3, 4, 2), "bmm_op"), ((4,), (3, 4, 5), "bmm_op"),
         ((3, 5, 4), (4,), "bmm_op")]


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("sa,sb,op", FORMS)
def test_float_forms_reach_their_op(world, sa, sb, op):
    run_spmd(COUNT + f"""
    C = mk(*{sa}) @ mk(*{sb})
    assert np_ is np or calls == ["{op}"], calls
    return C
    """, world=world)


@pytest.mark.parametrize("world", [1, 2])
def test_other_forms_keep_the_composition(world):
    # float32 promotes; int64, 1-D . 1-D and zero sizes reach no new op
    run_spmd(COUNT + """
    p = mk(6, 5, dtype=np.float32) @ mk(5)
    assert p.dtype == np.float64 and (np_ is np or calls == ["matvec_op"])
    del calls[:]
    parts = [p, mk(6, 5, dtype=np.int64) @ mk(5, dtype=np.int64) * 1.0,
             (mk(5) @ mk(5)) * np_.ones(1), np_.zeros((0, 4)) @ np_.ones(4),
             np_.ones(0) @ np_.zeros((0, 3)), np_.zeros((4, 0)) @ np_.ones(0),
             (np_.zeros((2, 3, 0)) @ np_.zeros((2, 0, 2))).reshape(12),
             (np_.zeros((0, 3, 2)) @ np_.zeros((2, 2))).reshape(0)]
    assert not calls, calls
    return np_.concatenate(parts)
    """, world=world)


_BUF = (ctypes.c_double * 66)()                  # never read
P = ctypes.c_void_p((ctypes.addressof(_BUF) + 15) // 16 * 16)
BIG = 1 << 39

def check(lib, who, call, table):
    for kw, what in table:
        assert call(**kw) != 0, kw
        msg = lib.rt_last_error().decode()
        assert msg.startswith(who + ":") and what in msg, (kw, msg)


def test_rt_gemv_rejects_bad_arguments(lib):
    def call(y=P, a=P, x=P, M=4, K=4, dtype=0, acc=0, ks=1, scratch=P):
        return lib.rt_gemv(0, y, a, x, M, K, K, 1, 1, 1, dtype, acc, ks,
                           scratch)

    check(lib, "rt_gemv", call, [
        (dict(M=-1), "negative extent"), (dict(K=-1), "negative extent"),
        (dict(M=1 << 40), "out of range"), (dict(K=1 << 40), "out of range"),
        (dict(M=BIG, K=BIG), "too large"), (dict(dtype=2), "bad dtype"),
        (dict(dtype=-1), "bad dtype"), (dict(acc=2), "bad accumulate"),
        (dict(ks=0), "bad ksplit"), (dict(ks=-3), "bad ksplit"),
        (dict(ks=2, scratch=None), "NULL scratch"), (dict(y=None), "NULL y"),
        (dict(a=None), "NULL a/x"), (dict(x=None), "NULL a/x")])
    assert call(M=0, y=None, a=None, x=None, scratch=None) == 0
    assert call(K=0, acc=1, a=None, x=None) == 0


def test_rt_gemv_plan_splits_k_only_for_few_rows(lib):
    def plan(M, K, a_rs, a_cs, cus=256, dtype=1):
        regime, ks = ctypes.c_int(), ctypes.c_int64()
        assert lib.rt_gemv_plan(P, M, K, a_rs, a_cs, dtype, cus,
                                ctypes.byref(regime), ctypes.byref(ks)) == 0
        r, s = ctypes.c_int(), ctypes.c_int()
        assert lib.rt_gemv_geometry(dtype, regime.value, ctypes.byref(r),
                                    ctypes.byref(s)) == 0
        return regime.value, ks.value, r.value, s.value

    for a_rs, a_cs, regime in ((1 << 20, 1, 0), (1, 1 << 20, 2),
                               ((1 << 20) + 1, 1, 1), (3, 1 << 20, 3)):
        got, ks, r, s = plan(4 * 256 * 256, 1 << 20, a_rs, a_cs)
        assert (got, ks) == (regime, 1)             # M alone fills 256 CUs
        got, ks, r, s = plan(3, 1 << 20, a_rs, a_cs)
        assert got == regime and 1 < ks <= (1 << 20) // s // 2
        assert plan(3, 3 * s, a_rs, a_cs)[1] == 1   # K too short to split


def test_rt_gemm_batched_rejects_bad_arguments(lib):
    def call(c=P, a=P, b=P, batch=3, M=4, N=4, K=4, ldc=4, c_bs=16,
             dtype=0, acc=0):
        return lib.rt_gemm_batched(0, c, a, b, batch, M, N, K, K, 1, N, 1,
                                   ldc, M * K, 0, c_bs, dtype, acc)

    check(lib, "rt_gemm_batched", call, [
        (dict(batch=-1), "negative batch"),
        (dict(batch=1 << 40), "batch out of range"),
        (dict(batch=BIG, M=256, N=1, K=1, ldc=1, c_bs=256), "batch too large"),
        (dict(batch=BIG, M=1, N=1, K=256, ldc=1, c_bs=1), "batch too large"),
        (dict(batch=BIG, M=1, N=256, K=1, ldc=256, c_bs=256),
         "batch too large"),
        (dict(c_bs=15), "c_bs"), (dict(M=-1), "negative extent"),
        (dict(K=1 << 40), "out of range"),
        (dict(M=BIG, K=BIG), "shape too large"), (dict(ldc=3), "ldc < N"),
        (dict(c=None), "NULL c"), (dict(a=None), "NULL a/b"),
        (dict(b=None), "NULL a/b"), (dict(dtype=2), "bad dtype"),
        (dict(acc=2), "bad accumulate")])
    assert call(batch=0, c=None, a=None, b=None) == 0
    assert call(M=0, c_bs=0, c=None, a=None, b=None) == 0
    assert call(K=0, acc=1, a=None, b=None) == 0
