"""Index-pure rematerialisation across flushes (common.remat) on the CPU
oracle backend: an array whose content is a cheap pure function of the
index is recomputed by later groups instead of being read.

Every result is compared with the switch off using np.array_equal (the same
operations run in the same order, so the bits must match) and with NumPy at
the suite's usual 1e-12.  Each case asserts through the debug-level
substitution counter (common.remat_substitutions) that at least one
substitution happened, so it cannot pass vacuously.
"""

import numpy as np
import pytest

from ramba_amd import common


def _count():
    return common.remat_substitutions


@pytest.fixture
def remat0(ra):
    """Threshold 0 for the test, settings restored afterwards."""
    saved = (common.remat, common.remat_min_bytes)
    common.remat, common.remat_min_bytes = 1, 0
    yield ra
    ra.sync()
    common.remat, common.remat_min_bytes = saved


def _host(x):
    return x.asarray() if hasattr(x, "asarray") else np.asarray(x)


def ab(prog, ra, tol=1e-12, expect_subst=True):
    """Run prog(ra) with remat on and off and prog(np); returns the
    substitution count of the `on` run."""
    common.remat = 1
    c0 = _count()
    on = [_host(x) for x in prog(ra)]
    nsub = _count() - c0
    common.remat = 0
    c0 = _count()
    off = [_host(x) for x in prog(ra)]
    assert _count() == c0, "substitution with the switch off"
    common.remat = 1
    ref = [np.asarray(x) for x in prog(np)]
    assert len(on) == len(off) == len(ref)
    for a, b, r in zip(on, off, ref):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a, b, equal_nan=True)
        assert a.shape == r.shape
        assert r.size <= 1 or np.any(r != 0), "degenerate all-zero case"
        np.testing.assert_allclose(a, r, rtol=tol, atol=tol)
    if expect_subst:
        assert nsub >= 1, "no substitution happened"
    return nsub


def _sync(np_):
    if hasattr(np_, "sync"):
        np_.sync()


# ---------------------------------------------------------------------------
# results unchanged
# ---------------------------------------------------------------------------

class TestResults:
    def test_flagship_chain(self, remat0):
        def prog(np_):
            A = np_.arange(1000) / 1000.0
            _sync(np_)
            B = np_.sin(A)
            C = np_.cos(A)
            D = B * B + C ** 2
            return B, C, D
        ab(prog, remat0)

    @pytest.mark.parametrize("sl", [slice(1, None), slice(None, None, 2),
                                    slice(None, None, -1),
                                    slice(3, -5, 3)],
                             ids=["1:", "::2", "::-1", "3:-5:3"])
    def test_sliced_reads(self, remat0, sl):
        def prog(np_):
            A = np_.arange(1027) * 0.25 + 3.0
            _sync(np_)
            return (A[sl] * 2.0 - 1.0,)
        ab(prog, remat0)

    def test_stencil_shape_float32(self, remat0):
        # not affine in the index, and five different weights: a wrong
        # offset, step or axis in the composed recipe changes the result
        # (a Laplacian of an affine input is zero whatever it computes).
        # Small integers and multiples of 0.5: float32 stays exact.
        def prog(np_):
            X = np_.fromfunction(lambda x, y: x * x + y * x, (67, 7),
                                 dtype=np.float32)
            _sync(np_)
            return (0.5 * X[:-2, 1:-1] + 2.0 * X[2:, 1:-1]
                    + 3.0 * X[1:-1, :-2] - 1.5 * X[1:-1, 2:]
                    - 4.0 * X[1:-1, 1:-1],)
        n = ab(prog, remat0)
        assert n >= 5

    def test_constant_fill(self, remat0):
        def prog(np_):
            Z = np_.full((33, 5), 2.5)
            _sync(np_)
            return (Z[1:, :] + Z[:-1, :],)
        ab(prog, remat0)

    def test_int64_arange_start_step(self, remat0):
        def prog(np_):
            A = np_.arange(5, 500, 3)
            _sync(np_)
            return (A * 2 + A[::-1], A[10:20])
        ab(prog, remat0)

    def test_transposed_and_broadcast_reads(self, remat0):
        def prog(np_):
            X = np_.fromfunction(lambda x, y: x * x * 10 - y * x - y, (6, 9),
                                 dtype=np.int64)
            _sync(np_)
            return (X.T + 1, X[2] + X, np_.broadcast_to(X[:, 3:4], (6, 9)) * 2,
                    X[::-1, 1::2] - 3 * X[:, :4], X.T[2:, ::-1] * 2)
        ab(prog, remat0)

    def test_reduction_of_pure_array(self, remat0):
        def prog(np_):
            A = np_.arange(777) * 0.5
            _sync(np_)
            return (np.asarray(float(A[5:].sum())),)
        ab(prog, remat0)


# ---------------------------------------------------------------------------
# invalidation: every write must be seen by the next read
# ---------------------------------------------------------------------------

class TestInvalidation:
    """Each program reads the pure array (a substitution), writes it, then
    reads it again; the second read must see the new values."""

    def _run(self, remat0, write):
        def prog(np_):
            A = np_.arange(64) * 0.5
            _sync(np_)
            first = A[1:] + 1.0          # substituted read
            _sync(np_)
            r = write(np_, A)
            A = A if r is None else r
            _sync(np_)
            return first, A + 0.0, A[::-1] * 2.0
        ab(prog, remat0)

    def test_slice_setitem(self, remat0):
        def w(np_, A):
            A[3:9] = -1.0
        self._run(remat0, w)

    def test_iadd(self, remat0):
        def w(np_, A):
            A += 1
        self._run(remat0, w)

    def test_iadd_unflushed_then_read(self, remat0):
        # the compound assign reads the old content through the recipe;
        # the new content (recipe + 1) is itself index-pure again
        def prog(np_):
            A = np_.arange(64) * 0.5
            _sync(np_)
            A += 1
            B = A * 3.0
            _sync(np_)
            return A + 0.0, B, A[2:] - A[:-2]
        ab(prog, remat0)

    def test_masked_write(self, remat0):
        def w(np_, A):
            m = np_.arange(64) % 3 == 0
            A[m] = 9.0
        self._run(remat0, w)

    def test_assign_from_numpy(self, remat0):
        def w(np_, A):
            A[:] = np.linspace(0.0, 1.0, 64)
        self._run(remat0, w)

    def test_fromarray_scatter(self, remat0):
        ra = remat0
        A = ra.arange(64) * 0.5
        ra.sync()
        assert A.bdarray.pure is not None
        ra._deferred.get_runtime().scatter_numpy(A.bdarray,
                                                 np.full(64, 7.0))
        assert A.bdarray.pure is None
        assert np.array_equal((A + 1.0).asarray(), np.full(64, 8.0))

    def test_write_through_second_view(self, remat0):
        def w(np_, A):
            V = A[10:20]
            V[:] = 0
        self._run(remat0, w)

    def test_out_style_targets(self, remat0):
        # out= is not supported by the frontend (it must refuse, not write
        # behind the engine's back); the region-write form that replaces it
        # (concatenate/pad write into views of one target) invalidates
        ra = remat0
        A = ra.arange(64) * 0.5
        ra.sync()
        with pytest.raises(TypeError):
            np.add(A, 1.0, out=A)
        assert A.bdarray.pure is not None

        def w(np_, A):
            src = np_.arange(64) * 0.5
            A[0:32] = src[32:]
            A[32:] = np_.concatenate([src[:16], src[:16]])
        self._run(remat0, w)

    def test_reshape_cumsum_result_over_pure(self, remat0):
        def w(np_, A):
            A[:] = np_.cumsum(np_.arange(64) * 0.5)
        self._run(remat0, w)

        def w2(np_, A):
            M = np_.fromfunction(lambda x, y: x * 8 + y, (8, 8),
                                 dtype=np.float64)
            A[:] = M.reshape(64) * 2.0
        self._run(remat0, w2)

    def test_read_before_write_in_one_group(self, remat0):
        # the substituted read keeps the OLD values although the write
        # lands in the same fused group
        def prog(np_):
            A = np_.arange(64) * 0.5
            _sync(np_)
            B = A[1:] * 2.0
            A[:-1] = 7.0
            _sync(np_)
            return B, A + 0.0
        ab(prog, remat0)


# ---------------------------------------------------------------------------
# cheapness gate: no recipe may be recorded
# ---------------------------------------------------------------------------

class TestGate:
    def _pure(self, ra, make):
        A = make(ra)
        ra.sync()
        return A.bdarray.pure

    def test_positive_control(self, remat0):
        assert self._pure(remat0, lambda ra: ra.arange(100) * 0.5) is not None

    def test_node_cap(self, remat0):
        def make(ra):
            a = ra.arange(100)
            return ((a * 2 + 1) * 3 - 4) * 5 + (a * 7 - 2) * (a + 9)
        assert self._pure(remat0, make) is None

    def test_mod(self, remat0):
        assert self._pure(remat0, lambda ra: ra.arange(100) % 7) is None

    def test_transcendental(self, remat0):
        assert self._pure(remat0, lambda ra: ra.sin(ra.arange(100))) is None

    def test_division_and_pow(self, remat0):
        assert self._pure(remat0, lambda ra: 1.0 / (ra.arange(100) + 1)) \
            is None
        assert self._pure(remat0, lambda ra: ra.arange(100) ** 2) is None

    def test_written_twice_in_group(self, remat0):
        def make(ra):
            a = ra.arange(100) * 0.5
            a[:] = 3.0
            return a
        assert self._pure(remat0, make) is None

        def make2(ra):
            e = ra.empty(100)
            e[:] = 3.0
            return e
        assert self._pure(remat0, make2) is None

    def test_non_identity_view_write(self, remat0):
        def make(ra):
            a = ra.empty(100)
            ra.sync()
            a[::2] = 1.0
            return a
        assert self._pure(remat0, make) is None

    def test_memory_operand(self, remat0):
        ra = remat0
        src = ra.fromarray(np.arange(100.0))
        assert self._pure(ra, lambda ra: src * 2.0) is None


# ---------------------------------------------------------------------------
# threshold
# ---------------------------------------------------------------------------

def test_threshold(ra):
    saved = (common.remat, common.remat_min_bytes)
    try:
        common.remat = 1
        common.remat_min_bytes = 256 << 20      # the default
        A = ra.arange(1_000_000) * 0.5          # 8 MB
        ra.sync()
        c0 = _count()
        r_default = (A[1:] + 1.0).asarray()
        assert _count() == c0
        common.remat_min_bytes = 0
        r_zero = (A[1:] + 1.0).asarray()
        assert _count() > c0
        assert np.array_equal(r_default, r_zero)
    finally:
        common.remat, common.remat_min_bytes = saved


def test_default_switches():
    import os
    assert "RAMBA_REMAT" in os.environ or common.remat == 1
    assert "RAMBA_REMAT_MIN_BYTES" in os.environ \
        or common.remat_min_bytes == 256 << 20


# ---------------------------------------------------------------------------
# fuzz A/B: remat on vs off must be bit-identical
# ---------------------------------------------------------------------------

def _fuzz_ab(ra, seeds):
    from fuzz_programs import build_program
    nsub_seeds = 0
    for sd in seeds:
        impl, _ = build_program(sd, mode="numpy")
        with np.errstate(all="ignore"):
            common.remat = 1
            c0 = _count()
            on = impl(ra)
            nsub_seeds += _count() > c0
            common.remat = 0
            off = impl(ra)
        common.remat = 1
        on = on if isinstance(on, (tuple, list)) else (on,)
        off = off if isinstance(off, (tuple, list)) else (off,)
        assert len(on) == len(off)
        for a, b in zip(on, off):
            a, b = _host(a), _host(b)
            assert a.dtype == b.dtype and a.shape == b.shape, sd
            assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), sd
    return nsub_seeds


def test_fuzz_ab_bit_identical(remat0):
    n = _fuzz_ab(remat0, range(2000))
    print(f"fuzz A/B: {n}/2000 seeds with at least one substitution")
