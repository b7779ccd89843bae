"""Integer-array indexing (a[idx]) and take(): parity vs NumPy on the CPU
oracle backend (single rank), plus the rt_take_rows argument checks on the
built library.  Gather moves bits: every comparison is array_equal.
"""

import ctypes
import os

import numpy as np
import pytest

from conftest import run_both

_MASK_DTYPES = ["float64", "float32", "int64", "int32", "int16", "int8",
                "uint8", "bool"]


def _a345(np_):
    # the ramba leg goes through an op so the source is not index-pure only
    return np_.arange(60).reshape(3, 4, 5)


def _eq(ra, impl):
    """run_both + identical shape (run_both alone would let () vs (1,)
    style differences through array_equal's broadcasting-free compare)."""
    r, n = run_both(impl, ra)
    assert r.shape == n.shape, (r.shape, n.shape)
    assert r.dtype == n.dtype, (r.dtype, n.dtype)
    return r, n


I2 = [1, 0]

# the index forms of the issue, as functions of (array, index-array)
FORMS_3D = {
    "a[i]": lambda a, i: a[i],
    "a[i,]": lambda a, i: a[i, ],
    "a[:,i]": lambda a, i: a[:, i],
    "a[:,:,i]": lambda a, i: a[:, :, i],
    "a[0,i]": lambda a, i: a[0, i],
    "a[i,0]": lambda a, i: a[i, 0],
    "a[:,0,i]": lambda a, i: a[:, 0, i],
    "a[:,i,0]": lambda a, i: a[:, i, 0],
    "a[0,:,i]": lambda a, i: a[0, :, i],
    "a[i,:,0]": lambda a, i: a[i, :, 0],
    "a[0,i,0]": lambda a, i: a[0, i, 0],
    "a[0,1,i]": lambda a, i: a[0, 1, i],
    "a[1:,i]": lambda a, i: a[1:, i],
    "a[::2,i]": lambda a, i: a[::2, i],
    "a[i,1:3]": lambda a, i: a[i, 1:3],
    "a[i,::-1]": lambda a, i: a[i, ::-1],
    "a[...,i]": lambda a, i: a[..., i],
    "a[i,...]": lambda a, i: a[i, ...],
    "a[...,i,:]": lambda a, i: a[..., i, :],
    "a[0,...,i]": lambda a, i: a[0, ..., i],
    "a[i,...,0]": lambda a, i: a[i, ..., 0],
    "a[...,0,i]": lambda a, i: a[..., 0, i],
}


class TestForms:
    @pytest.mark.parametrize("form", sorted(FORMS_3D))
    def test_form_1d_index(self, ra, form):
        f = FORMS_3D[form]
        _eq(ra, lambda np_: f(_a345(np_), [2, 0]))

    @pytest.mark.parametrize("form", sorted(FORMS_3D))
    def test_form_2d_index(self, ra, form):
        f = FORMS_3D[form]
        _eq(ra, lambda np_: f(_a345(np_), np.array([[1, 2], [2, 0]])))

    def test_issue_shapes(self, ra):
        a = _a345(ra)
        i = np.array([2, 0])
        assert a[0, :, i].shape == (2, 4)
        assert a[i, :, 0].shape == (2, 4)
        assert a[:, 0, i].shape == (3, 2)
        assert a[0, i].shape == (2, 5)
        assert a[:, i].shape == (3, 2, 5)
        assert a[:, [[1, 2], [3, 0]]].shape == (3, 2, 2, 5)

    def test_1d_float_source(self, ra):
        _eq(ra, lambda np_: (np_.arange(7) * 0.5)[[3, 0, 2]])
        _eq(ra, lambda np_: (np_.arange(7) * 0.5)[np.array([[6, 6], [0, 1]])])

    def test_negative_step_view_source(self, ra):
        _eq(ra, lambda np_: (np_.arange(7) * 0.5)[::-1][[0, 5, -1]])
        _eq(ra, lambda np_: _a345(np_)[::-1, :, ::-2][[2, 0], 1:])

    def test_transposed_source(self, ra):
        _eq(ra, lambda np_: _a345(np_).transpose(2, 0, 1)[[4, 0, 4]])
        _eq(ra, lambda np_: _a345(np_).T[:, [3, 1]])

    def test_duplicates_negatives(self, ra):
        _eq(ra, lambda np_: _a345(np_)[:, [1, 1, 1, 3, 1]])
        _eq(ra, lambda np_: _a345(np_)[[-1, -3, -2]])
        _eq(ra, lambda np_: (np_.arange(7) * 1.0)[[-7, -1, -1]])


class TestIndexKinds:
    @pytest.mark.parametrize("dt", [np.int32, np.int64, np.uint8, np.int8,
                                    np.uint16, np.uint64])
    def test_numpy_dtypes(self, ra, dt):
        _eq(ra, lambda np_: _a345(np_)[:, np.array([3, 0, 2], dtype=dt)])

    def test_ramba_index_computed(self, ra):
        def impl(np_):
            idx = np_.arange(5)[::-1] % 3
            return (np_.arange(7) * 2.0)[idx]
        _eq(ra, impl)

    def test_ramba_index_int32_2d(self, ra):
        def impl(np_):
            idx = (np_.arange(6) % 4).reshape(2, 3).astype(np.int32)
            return _a345(np_)[:, idx]
        _eq(ra, impl)

    def test_ramba_index_reused_as_is(self, ra):
        idx = ra.fromarray(np.array([4, 1, 1], dtype=np.int64))
        got = (ra.arange(7) * 1.0)[idx].asarray()
        assert np.array_equal(got, (np.arange(7) * 1.0)[[4, 1, 1]])

    def test_empty_index(self, ra):
        _eq(ra, lambda np_: _a345(np_)[:, []])
        _eq(ra, lambda np_: _a345(np_)[np.zeros((0, 2), dtype=np.int64)])
        _eq(ra, lambda np_: (np_.arange(7) * 1.0)[[]])

    def test_zero_length_row(self, ra):
        _eq(ra, lambda np_: np_.zeros((4, 0, 3))[[1, 2]])
        _eq(ra, lambda np_: _a345(np_)[[1, 2], 2:2])

    @pytest.mark.parametrize("dt", _MASK_DTYPES)
    def test_every_dtype(self, ra, dt):
        def impl(np_):
            a = (np_.arange(24) % 5).reshape(6, 4).astype(dt)
            return a[[5, 0, -2, 0]], a[:, [3, 3, 0]]
        r0 = impl(ra)
        n0 = impl(np)
        for r, n in zip(r0, n0):
            r = r.asarray()
            assert r.dtype == n.dtype and np.array_equal(r, n)

    def test_result_is_a_copy(self, ra):
        a = ra.arange(6) * 1.0
        b = a[[0, 1]]
        a[0:2] = 9.0
        assert np.array_equal(b.asarray(), [0.0, 1.0])


class TestTake:
    @pytest.mark.parametrize("axis", [None, 0, 1, -1])
    def test_axes(self, ra, axis):
        _eq(ra, lambda np_: np_.take(_a345(np_), [2, 0, -1], axis=axis))
        _eq(ra, lambda np_: _a345(np_).take(np.array([[1], [0]]), axis=axis))

    def test_scalar_index(self, ra):
        _eq(ra, lambda np_: np_.take(_a345(np_), 1, axis=2))

    def test_numpy_dispatch_stays_distributed(self, ra):
        a = _a345(ra)
        r = np.take(a, [3, 0], axis=1)
        assert isinstance(r, ra.ndarray)
        assert np.array_equal(r.asarray(),
                              np.take(_a345(np), [3, 0], axis=1))

    def test_out_and_mode_unsupported(self, ra):
        a = ra.arange(5)
        with pytest.raises(NotImplementedError):
            ra.take(a, [0], out=ra.zeros(1))
        with pytest.raises(NotImplementedError):
            ra.take(a, [0], mode="wrap")
        with pytest.raises(NotImplementedError):
            a.take([0], mode="clip")


class TestErrors:
    @pytest.mark.parametrize("idx,k", [([0, 7], 7), ([-8, 0], -8),
                                       ([3, 100, -100], -100)])
    def test_out_of_bounds_1d(self, ra, idx, k):
        a = ra.arange(7) * 1.0
        with pytest.raises(IndexError) as e:
            a[idx]
        assert str(e.value) == (f"index {k} is out of bounds for axis 0 "
                                "with size 7")

    def test_out_of_bounds_axis_named_in_indexed_array(self, ra):
        a = _a345(ra)
        with pytest.raises(IndexError) as e:
            a[0, :, [1, 5]]
        assert str(e.value) == "index 5 is out of bounds for axis 2 with size 5"
        with pytest.raises(IndexError) as e:
            a[:, np.array([4], dtype=np.int32)]
        assert str(e.value) == "index 4 is out of bounds for axis 1 with size 4"
        with pytest.raises(IndexError) as e:
            a[..., ra.fromarray(np.array([0, -6]))]
        assert str(e.value) == ("index -6 is out of bounds for axis 2 with "
                                "size 5")

    def test_out_of_bounds_on_empty_axis(self, ra):
        with pytest.raises(IndexError):
            ra.zeros((0, 3))[[0]]

    def test_float_index(self, ra):
        a = ra.arange(7)
        msg = "arrays used as indices must be of integer (or boolean) type"
        for idx in ([1.0, 2.0], np.array([0.5]), ra.arange(3) * 1.0):
            with pytest.raises(IndexError) as e:
                a[idx]
            assert str(e.value) == msg

    def test_unsupported_forms(self, ra):
        a = _a345(ra)
        with pytest.raises(IndexError, match="two or more index arrays"):
            a[[0, 1], [1, 2]]
        with pytest.raises(IndexError, match="two or more index arrays"):
            a[[0, 1], :, np.array([1, 2])]
        with pytest.raises(IndexError, match="None"):
            a[None, [0, 1]]
        with pytest.raises(IndexError, match="None"):
            a[[0, 1], None]
        with pytest.raises(IndexError, match="boolean list"):
            a[[True, False, True]]
        with pytest.raises(IndexError, match="boolean"):
            a[:, np.array([True, False, True, False])]

    def test_setitem_raises_and_leaves_array(self, ra):
        a = ra.arange(6) * 1.0
        before = a.asarray().copy()
        for idx in ([0, 1], np.array([0, 1]), (np.array([2]),),
                    ra.fromarray(np.array([3]))):
            with pytest.raises((IndexError, NotImplementedError)):
                a[idx] = 1
        b = _a345(ra)
        with pytest.raises((IndexError, NotImplementedError)):
            b[:, [0, 1]] = 1
        assert np.array_equal(a.asarray(), before)
        assert np.array_equal(b.asarray(), _a345(np))

    def test_setitem_runs_no_gather(self, ra, monkeypatch):
        from ramba_amd import runtime
        monkeypatch.setattr(runtime.Runtime, "take_op",
                            lambda *a, **k: pytest.fail("gather ran"))
        a = ra.arange(6) * 1.0
        with pytest.raises((IndexError, NotImplementedError)):
            a[[0, 1]] = 1


class TestSourceReuse:
    """The no-copy case: a constructed identity-view source whose shards
    span axes 1.. is gathered from directly."""

    @staticmethod
    def _count_groups(monkeypatch):
        from ramba_amd import runtime
        seen = []
        orig = runtime.Runtime.execute_group

        def counting(self, group):
            seen.append(tuple(group.shape))
            return orig(self, group)
        monkeypatch.setattr(runtime.Runtime, "execute_group", counting)
        return seen

    def test_table_gather_adds_no_copy_group(self, ra, monkeypatch):
        table = ra.fromarray(np.arange(40.0).reshape(10, 4))
        idx = ra.fromarray(np.array([7, 7, 0], dtype=np.int64))
        ra.sync()
        seen = self._count_groups(monkeypatch)
        out = table[idx]
        # only the bounds reduction over the (3,) index ran; no (10, 4) copy
        assert (10, 4) not in seen, seen
        assert seen == [(3,)], seen
        assert np.array_equal(out.asarray(),
                              np.arange(40.0).reshape(10, 4)[[7, 7, 0]])

    def test_view_source_is_copied_once(self, ra, monkeypatch):
        table = ra.fromarray(np.arange(40.0).reshape(10, 4))
        ra.sync()
        seen = self._count_groups(monkeypatch)
        out = table[::2][[1, 4]]
        assert seen.count((5, 4)) == 1, seen
        assert np.array_equal(out.asarray(),
                              np.arange(40.0).reshape(10, 4)[::2][[1, 4]])


# ---------------------------------------------------------------------------
# C ABI: argument validation runs before any HIP call, so it is testable on
# a machine without a GPU
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.fail(f"{hip_backend.LIBPATH} not built (run build())")
    return hip_backend._load_lib()


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _call(lib, dst=8, src=8, n=1, nd_inner=1, elemsize=8):
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf)
    return lib.rt_take_rows(
        0, ctypes.c_void_p(base if dst else None),
        ctypes.c_void_p(base if src else None), None, None, n, 1, 1,
        nd_inner, _i64(1, 1, 1), _i64(1, 1, 1), _i64(1, 1, 1), 1, 1,
        elemsize, None)


class TestCAbiValidation:
    def test_export_present(self, lib):
        assert hasattr(lib, "rt_take_rows")

    @pytest.mark.parametrize("es", [0, 3, 5, 16, -1])
    def test_bad_elemsize(self, lib, es):
        assert _call(lib, elemsize=es) != 0
        assert b"elemsize" in lib.rt_last_error()

    @pytest.mark.parametrize("nd", [-1, 4, 9])
    def test_bad_nd_inner(self, lib, nd):
        assert _call(lib, nd_inner=nd) != 0
        assert b"nd_inner" in lib.rt_last_error()

    def test_negative_n(self, lib):
        assert _call(lib, n=-1) != 0
        assert b"negative n" in lib.rt_last_error()

    def test_null_pointers(self, lib):
        assert _call(lib, dst=0) != 0
        assert b"NULL" in lib.rt_last_error()
        assert _call(lib, src=0) != 0
        assert b"NULL" in lib.rt_last_error()

    def test_n_zero_is_a_no_op(self, lib):
        assert _call(lib, n=0) == 0
        assert _call(lib, n=0, dst=0, src=0) == 0

    def test_regime_choice(self, lib):
        """The host-side regime table the GPU tests rely on: rows under
        256 B narrow; wide rows vectorised only when extent, strides and
        pointers are 16-byte multiples."""
        def regime(inner, sstr, dstr, srs, drs, es, dst=4096, src=8192):
            return lib.rt_take_regime(
                ctypes.c_void_p(dst), ctypes.c_void_p(src), len(inner),
                _i64(*inner), _i64(*sstr), _i64(*dstr), srs, drs, es)
        assert regime((), (), (), 1, 1, 8) == 0              # 1-D gather
        assert regime((31,), (1,), (1,), 48, 31, 8) == 0     # 248 B
        assert regime((128,), (1,), (1,), 160, 128, 8) == 1  # 1 KiB rows
        assert regime((129,), (1,), (1,), 192, 129, 4) == 2  # 516 B, odd
        assert regime((128,), (1,), (1,), 160, 128, 8, dst=4104) == 2
        assert regime((128,), (1,), (1,), 161, 128, 8) == 2  # row stride
        assert regime((3, 50), (96, 1), (50, 1), 288, 150, 2) == 2
        assert regime((2, 3, 16), (96, 32, 1), (48, 16, 1), 192, 96, 8) == 1
        assert regime((3, 7), (64, 1), (7, 1), 192, 21, 2) == 0
        assert regime((1,), (1,), (1,), 1, 1, 3) == -1
