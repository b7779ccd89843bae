"""The older ramba_rt entry points (rt_copy_box, rt_combine_box, rt_cumsum,
rt_mask_compact, rt_axis_scan, rt_flat_copy) validate their arguments on
the host before any HIP call, like rt_take_rows and rt_arg_*: a bad
argument comes back as a return code and a message naming the entry point
and the argument, never as a launch.  Runs without a GPU: every call here
either fails validation or has a zero extent (return 0, no launch)."""

import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from ramba_amd import hip_backend
    if not os.path.exists(hip_backend.LIBPATH):
        pytest.skip("libramba_rt.so not built")
    return hip_backend._load_lib()


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


_BUF = (ctypes.c_double * 64)()
P = ctypes.cast(_BUF, ctypes.c_void_p)     # a non-NULL pointer, never read
ONES = i64(1, 1, 1, 1)
HUGE = (1 << 39, 1 << 39)


def rejected(lib, rc, who, what):
    msg = lib.rt_last_error().decode()
    assert rc != 0, f"{who} accepted a call that should fail on {what!r}"
    assert msg.startswith(who + ":") and what in msg, (msg, who, what)


def test_chunk_constants(lib):
    # whole items per thread of a 256-thread block; host arithmetic only
    for chunk in (lib.rt_scan_chunk(), lib.rt_mask_chunk()):
        assert chunk > 0 and chunk % 256 == 0


def test_copy_box_rejects(lib):
    def call(nd=1, shape=(4,), dst=P, src=P, es=8, dstr=ONES, sstr=ONES,
             shp=None):
        return lib.rt_copy_box(0, dst, src, nd,
                               i64(*shape) if shp is None else shp, dstr,
                               sstr, 0, 0, es)
    w = "rt_copy_box"
    rejected(lib, call(nd=0), w, "nd out of range")
    rejected(lib, call(nd=5, shape=(1, 1, 1, 1, 1)), w, "nd out of range")
    rejected(lib, call(shape=(-4,)), w, "negative extent")
    rejected(lib, call(nd=2, shape=(0, -1)), w, "negative extent")
    rejected(lib, call(nd=2, shape=HUGE), w, "shape too large")
    rejected(lib, call(shape=(1 << 40,)), w, "out of range")
    rejected(lib, call(dst=None), w, "NULL dst/src")
    rejected(lib, call(src=None), w, "NULL dst/src")
    rejected(lib, call(dstr=None), w, "NULL strides")
    rejected(lib, call(sstr=None), w, "NULL strides")
    rejected(lib, call(shp=ctypes.POINTER(ctypes.c_int64)()), w, "NULL shape")
    for es in (0, 3, 16, -1):
        rejected(lib, call(es=es), w, "bad elemsize")
    # zero extent: nothing to do, no launch, NULL data allowed
    assert call(shape=(0,)) == 0
    assert call(nd=3, shape=(3, 0, 1 << 39), dst=None, src=None) == 0


def test_combine_box_rejects(lib):
    def call(nd=1, shape=(4,), dst=P, src=P, dtype=0, op=0, dstr=ONES,
             sstr=ONES):
        return lib.rt_combine_box(0, dst, src, nd, i64(*shape), dstr, sstr,
                                  0, 0, dtype, op)
    w = "rt_combine_box"
    rejected(lib, call(nd=0), w, "nd out of range")
    rejected(lib, call(nd=5, shape=(1, 1, 1, 1, 1)), w, "nd out of range")
    rejected(lib, call(shape=(-1,)), w, "negative extent")
    rejected(lib, call(nd=2, shape=HUGE), w, "shape too large")
    rejected(lib, call(dst=None), w, "NULL dst/src")
    rejected(lib, call(src=None), w, "NULL dst/src")
    rejected(lib, call(dstr=None), w, "NULL strides")
    for dt in (-1, 7, 100):
        rejected(lib, call(dtype=dt), w, "bad dtype")
    for op in (-1, 6):
        rejected(lib, call(op=op), w, "bad op")
    assert call(shape=(0,)) == 0
    assert call(nd=2, shape=(5, 0), dst=None, src=None) == 0


def test_cumsum_rejects(lib):
    def call(phase, n=10, nblocks=1, in_=P, out=P, bsums=P, total=P,
             dtype=2):
        return lib.rt_cumsum(0, in_, 0, 1, n, out, 0, bsums, nblocks, total,
                             0.0, 0, dtype, phase)
    w = "rt_cumsum"
    for ph in (0, 4, -1, 99):     # no phase falls through to another
        rejected(lib, call(ph), w, "bad phase")
    for ph in (1, 2, 3):
        for dt in (-1, 4, 6):
            rejected(lib, call(ph, dtype=dt), w, "bad dtype")
        rejected(lib, call(ph, n=-1), w, "negative n")
        rejected(lib, call(ph, nblocks=0), w, "nblocks < 1")
        rejected(lib, call(ph, nblocks=-3), w, "nblocks < 1")
        rejected(lib, call(ph, nblocks=1 << 31), w, "nblocks too large")
        rejected(lib, call(ph, bsums=None), w, "NULL bsums")
    rejected(lib, call(1, in_=None), w, "NULL in")
    rejected(lib, call(3, in_=None), w, "NULL in")
    rejected(lib, call(3, out=None), w, "NULL out")
    # zero elements: phases 1 and 3 have nothing to do
    assert call(1, n=0) == 0
    assert call(3, n=0, in_=None, out=None, bsums=None) == 0


def test_mask_compact_rejects(lib):
    M = lib.rt_mask_chunk()

    def call(phase=1, nd=1, shape=(10,), a=P, m=P, out=P, bcounts=P,
             nchunks=1, dtype=0, astr=ONES, mstr=ONES):
        return lib.rt_mask_compact(0, a, m, out, nd, i64(*shape), astr, mstr,
                                   bcounts, nchunks, dtype, phase)
    w = "rt_mask_compact"
    rejected(lib, call(nd=0), w, "nd out of range")
    rejected(lib, call(nd=5, shape=(1, 1, 1, 1, 1)), w, "nd out of range")
    rejected(lib, call(shape=(-10,)), w, "negative extent")
    rejected(lib, call(nd=2, shape=HUGE), w, "shape too large")
    rejected(lib, call(astr=None), w, "NULL strides")
    rejected(lib, call(mstr=None), w, "NULL strides")
    for dt in (-1, 7):
        rejected(lib, call(dtype=dt), w, "bad dtype")
    for ph in (0, 2, 4, -1):
        rejected(lib, call(phase=ph), w, "bad phase")
    # nchunks must be ceil(n / chunk): every chunk of n owns a bcounts slot
    for n, bad in ((10, 0), (10, 2), (M, 2), (M + 1, 1), (M + 1, 3),
                   (3 * M, 2), (10, -1)):
        for ph in (1, 3):
            rejected(lib, call(phase=ph, shape=(n,), nchunks=bad), w,
                     "nchunks")
    rejected(lib, call(nd=2, shape=(M, 3), nchunks=2), w, "nchunks")
    rejected(lib, call(m=None), w, "NULL m")
    rejected(lib, call(bcounts=None), w, "NULL bcounts")
    rejected(lib, call(phase=3, a=None), w, "NULL a/out")
    rejected(lib, call(phase=3, out=None), w, "NULL a/out")
    assert call(shape=(0,), nchunks=1) == 0
    assert call(phase=3, nd=2, shape=(0, 7), a=None, m=None, out=None,
                bcounts=None, nchunks=0) == 0


def test_axis_scan_rejects(lib):
    def call(nd=2, shape=(4, 4), axis=0, in_=P, out=P, totals=P, dtype=0,
             tot2=None, nchunks=1, istr=ONES, ostr=ONES):
        return lib.rt_axis_scan(0, in_, out, totals, nd, i64(*shape), istr,
                                ostr, axis, dtype, tot2, nchunks)
    w = "rt_axis_scan"
    rejected(lib, call(nd=1, shape=(4,)), w, "nd out of range")
    rejected(lib, call(nd=5, shape=(1, 1, 1, 1, 1)), w, "nd out of range")
    rejected(lib, call(axis=2), w, "axis out of range")
    rejected(lib, call(axis=-1), w, "axis out of range")
    rejected(lib, call(shape=(4, -4)), w, "negative extent")
    rejected(lib, call(shape=HUGE), w, "shape too large")
    rejected(lib, call(istr=None), w, "NULL strides")
    rejected(lib, call(ostr=None), w, "NULL strides")
    for dt in (-1, 4, 6):
        rejected(lib, call(dtype=dt), w, "bad dtype")
    rejected(lib, call(nchunks=0), w, "nchunks < 1")
    rejected(lib, call(nchunks=-2, tot2=P), w, "nchunks < 1")
    rejected(lib, call(nchunks=2, tot2=None), w, "needs tot2")
    rejected(lib, call(nchunks=1 << 45, tot2=P), w, "too large")
    rejected(lib, call(in_=None), w, "NULL in/out/totals")
    rejected(lib, call(out=None), w, "NULL in/out/totals")
    rejected(lib, call(totals=None), w, "NULL in/out/totals")
    assert call(shape=(0, 4)) == 0
    assert call(shape=(4, 0), in_=None, out=None, totals=None) == 0
    assert call(nd=3, shape=(4, 0, 2), axis=2, nchunks=3, tot2=P) == 0


def test_flat_copy_rejects(lib):
    def call(nd=2, shape=(3, 5), flat0=0, n=15, boxed=P, dense=P, es=8,
             scatter=0, strides=ONES):
        return lib.rt_flat_copy(0, boxed, dense, nd, i64(*shape), strides,
                                flat0, n, es, scatter)
    w = "rt_flat_copy"
    rejected(lib, call(nd=0), w, "nd out of range")
    rejected(lib, call(nd=5, shape=(1, 1, 1, 1, 1)), w, "nd out of range")
    rejected(lib, call(shape=(3, -5)), w, "negative extent")
    rejected(lib, call(shape=HUGE), w, "shape too large")
    rejected(lib, call(strides=None), w, "NULL strides")
    for es in (0, 3, 16):
        rejected(lib, call(es=es), w, "bad elemsize")
    for sc in (-1, 2):
        rejected(lib, call(scatter=sc), w, "bad scatter")
    rejected(lib, call(flat0=-1, n=3), w, "negative flat0")
    rejected(lib, call(n=-1), w, "negative n")
    for sc in (0, 1):             # a subrange outside the box
        rejected(lib, call(flat0=0, n=16, scatter=sc), w, "flat0 + n")
        rejected(lib, call(flat0=15, n=1, scatter=sc), w, "flat0 + n")
        rejected(lib, call(flat0=16, n=0, scatter=sc), w, "flat0 + n")
        rejected(lib, call(flat0=7, n=(1 << 63) - 1, scatter=sc), w,
                 "flat0 + n")
        rejected(lib, call(shape=(3, 0), flat0=0, n=1, scatter=sc), w,
                 "flat0 + n")
    rejected(lib, call(boxed=None), w, "NULL boxed/dense")
    rejected(lib, call(dense=None), w, "NULL boxed/dense")
    assert call(n=0) == 0
    assert call(flat0=15, n=0, boxed=None, dense=None) == 0
    assert call(shape=(3, 0), flat0=0, n=0) == 0


def test_dtype_table_and_removed_entry(lib):
    # the binding's dtype codes are the list the GPU kernel tests drive the
    # C side with; the single-pass lookback scan entry point is gone
    import rt_ref
    from ramba_amd import hip_backend
    assert hip_backend.RT_DTYPE == {
        **{n: i for i, n in enumerate(rt_ref.DT7)}, "bool": 6}
    assert not hasattr(lib, "rt_cumsum_scan")
