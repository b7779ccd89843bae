"""Two ranks on one MI355X (gloo transport) for the runtime kernels whose
cross-rank geometry tests/test_gpu_multirank.py leaves out: reshape with
flat intervals that cut rows mid-row on both sides, small-dtype and logical
axis-reduction merges, a[mask] on int8, int64 cumsum of a strided view and
of a 3-D array along the split axis.  Each result is compared with NumPy by
array_equal (integer data: no tolerance)."""

import pytest

from test_gpu_multirank import run_spmd_gpu

pytestmark = pytest.mark.gpu

# the body runs once as impl(ramba_amd) and once as impl(numpy); `fa` puts a
# host array on whichever it is, `flat` brings any result back as int64 with
# its dtype code appended, so array_equal also compares the result dtypes
PRELUDE = """
        import numpy as _np
        fa = (lambda h: h) if np_ is _np else np_.fromarray
        def flat(*rs):
            out = []
            for r in rs:
                r = r.asarray() if hasattr(r, "asarray") else _np.asarray(r)
                out.append(r.astype(_np.int64).reshape(-1))
                out.append(_np.array([ord(r.dtype.char), r.ndim, r.size]))
            return _np.concatenate(out)
        def vals(n, dtype):
            v = (_np.arange(n, dtype=_np.int64) * 7) % 251 - 100
            return v.astype(dtype)
"""


def _run(body):
    run_spmd_gpu(PRELUDE + body)


def test_reshape_cuts_rows_mid_row_2rank_gpu():
    # 37 x 53 -> 53 x 37: rank boundaries at rows 19 | 27 of the two shapes,
    # so every flat interval starts and ends inside a row of the other side
    _run("""
        a = fa(vals(37 * 53, "int64").reshape(37, 53))
        b = fa(vals(41 * 29, "int32").reshape(41, 29))
        c = fa(vals(37 * 53, "int8").reshape(37, 53))
        return flat(a.reshape((53, 37)), b.reshape((1189,)),
                    c.reshape((53, 37)), a.reshape((1961,)))
    """)


def test_small_dtype_and_logical_axis_merges_2rank_gpu():
    _run("""
        rs = []
        for dtype in ("int8", "int16"):
            a = fa(vals(403 * 37, dtype).reshape(403, 37))
            rs += [a.min(axis=0), a.max(axis=0), a.sum(axis=0)]
        rng = _np.random.default_rng(3)
        hb = rng.integers(0, 2, (403, 37)).astype(bool)
        hb[:, 5] = True           # a column all() keeps, one any() drops
        hb[:, 7] = False
        hb[300, 9] = False
        b = fa(hb)
        rs += [b.any(axis=0), b.all(axis=0)]
        return flat(*rs)
    """)


def test_mask_getitem_int8_2d_2rank_gpu():
    _run("""
        h = vals(211 * 47, "int8").reshape(211, 47)
        m = (_np.arange(211 * 47) % 3 == 0).reshape(211, 47)
        a, mk = fa(h), fa(m)
        return flat(a[mk], a[fa(_np.zeros((211, 47), dtype=bool))])
    """)


def test_flat_cumsum_of_strided_view_2rank_gpu():
    _run("""
        a = fa(vals(30011, "int64"))
        return flat(a[5:30000:3].cumsum(), a[::-1].cumsum(),
                    a[29000:100:-7].cumsum())
    """)


def test_cumsum_3d_along_split_axis_2rank_gpu():
    _run("""
        a = fa(vals(67 * 9 * 11, "int64").reshape(67, 9, 11))
        return flat(a.cumsum(axis=0), a.cumsum(axis=2))
    """)
