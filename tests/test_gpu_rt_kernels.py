"""The box, flat, mask and scan runtime kernels against NumPy, through the
C ABI of libramba_rt.so: rt_copy_box, rt_combine_box, rt_cumsum (phases
1-3), rt_axis_scan, rt_mask_compact and rt_flat_copy at the geometry the
frontend never produces — offsets, permuted / negative / zero / padded
strides, every dtype code, block- and chunk-boundary sizes, and one case per
capped grid that is large enough for a second grid-stride trip.

Rules ("Runtime kernel geometry"):
  * exact comparison — np.array_equal plus a dtype check, no tolerance.
    Float inputs to scans and add / mul combines are small integers
    (tests/rt_cases.py; the bound is asserted on the CPU by
    tests/test_rt_ref_host.py), so every summation order gives the same
    bits;
  * guard bands — every destination is larger than what the call may write
    and pre-filled with a sentinel that must survive outside the box;
  * host bounds check — `inb` proves from (off, shape, strides) that both
    sides of every launch stay inside their allocations before it goes out.
The NumPy models are tests/rt_ref.py.  No case passes arguments meant to
fail: bad arguments belong to tests/test_rt_validation_host.py."""

import ctypes

import numpy as np
import pytest

import rt_cases as rc
import rt_ref
from rt_ref import DT4, DT7, OPS, geom

pytestmark = pytest.mark.gpu

G = 64                       # guard elements on each side of a buffer
ES_DT = {1: "int8", 2: "int16", 4: "int32", 8: "int64"}


def i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


def sentinel(dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return dt.type(-12345.0)
    return dt.type(0xA5 if dt.kind == "u" else -99)


class Dev:
    def __init__(self, backend):
        self.lib = backend.lib
        self.torch = backend.torch
        self.C = self.lib.rt_scan_chunk()
        self.M = self.lib.rt_mask_chunk()

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def up(self, h):
        return self.torch.from_numpy(np.ascontiguousarray(h)).cuda()

    def full(self, n, dtype):
        return self.up(np.full(n, sentinel(dtype), dtype=dtype))

    @staticmethod
    def down(t):
        return t.cpu().numpy()      # syncs with the launch stream

    @staticmethod
    def ptr(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + int(off) * t.element_size())

    def ok(self, rcode, what):
        assert rcode == 0, (what, self.lib.rt_last_error().decode())


@pytest.fixture(scope="module")
def dev(ra_gpu):
    from ramba_amd import deferred
    return Dev(deferred.get_runtime().backend)


def inb(size, off, shape, strides, what):
    """The box at (off, shape, strides) lies inside an allocation of `size`
    elements: asserted on the host before every launch."""
    r = rt_ref.reach(off, shape, strides)
    if r is not None:
        assert 0 <= r[0] and r[1] < size, (what, r, size)


def guarded(base_shape, dtype, fill=None):
    """(flat buffer with G guard elements at both ends, its interior as an
    array of base_shape).  Everything starts as the sentinel."""
    n = int(np.prod(base_shape))
    buf = np.full(n + 2 * G, sentinel(dtype), dtype=dtype)
    base = buf[G:G + n].reshape(base_shape)
    if fill is not None:
        base[...] = np.resize(np.asarray(fill, dtype=dtype),
                              n).reshape(base_shape)     # repeats if short
    return buf, base


def check_written(got, want, touched, what, nan_ok=False):
    """got == want everywhere, and the sentinel survives wherever the model
    says the call writes nothing."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    keep = np.ones(got.size, dtype=bool)
    keep[np.asarray(touched).reshape(-1)] = False
    sent = sentinel(got.dtype)
    assert np.all(got[keep] == sent), (what, "wrote outside the box",
                                       np.flatnonzero(got[keep] != sent)[:8])
    assert np.array_equal(got, want, equal_nan=nan_ok), (
        what, np.flatnonzero(~((got == want) | (nan_ok & (got != got)
                                               & (want != want))))[:8])


def pad_view(shape, lo, extra):
    """(container shape with `extra` more per axis, slices of the box)"""
    sl = tuple(slice(lo, lo + s) for s in shape)
    return tuple(s + extra for s in shape), sl


def distinct(n, dtype):
    """Values that tell positions apart (period 251, range [-100, 150])."""
    v = (np.arange(n, dtype=np.int64) * 7) % 251 - 100
    if np.dtype(dtype).kind == "u":
        v = v + 100
    return v.astype(dtype)


# =============================================================================
# rt_copy_box
# =============================================================================

COPY_SHAPES = [(1,), (255,), (256,), (257,), (7, 5), (3, 4, 5), (2, 3, 4, 5),
               (1, 1, 1, 1)]
COPY_VARIANTS = ["dense", "transposed_dst", "negative_src", "broadcast_src",
                 "padded_offsets"]


def _copy_views(shape, dtype, variant):
    n = int(np.prod(shape))
    vals = distinct(4 * n + 64, dtype)
    dbuf, dbase = guarded(shape, dtype)
    sbuf, sbase = guarded(shape, dtype, vals)
    dview, sview = dbase, sbase
    if variant == "transposed_dst":
        dbuf, dbase = guarded(tuple(reversed(shape)), dtype)
        dview = dbase.T
    elif variant == "negative_src":
        sview = np.flip(sbase)          # src_off lands on the last element
    elif variant == "broadcast_src":
        sbuf, sbase = guarded((1,) + tuple(shape[1:]), dtype, vals)
        sview = np.broadcast_to(sbase, shape)      # stride 0 on axis 0
    elif variant == "padded_offsets":
        dshape, dsl = pad_view(shape, 2, 3)
        sshape, ssl = pad_view(shape, 1, 2)
        dbuf, dbase = guarded(dshape, dtype)
        sbuf, sbase = guarded(sshape, dtype, vals)
        dview, sview = dbase[dsl], sbase[ssl]
    return dbuf, dview, sbuf, sview


def _run_copy(dev, dbuf, dview, sbuf, sview, what):
    shape = dview.shape
    es = dbuf.itemsize
    doff, dstr = geom(dview, dbuf)
    soff, sstr = geom(sview, sbuf)
    inb(dbuf.size, doff, shape, dstr, what)
    inb(sbuf.size, soff, shape, sstr, what)
    d, s = dev.up(dbuf), dev.up(sbuf)
    dev.ok(dev.lib.rt_copy_box(dev.stream(), dev.ptr(d), dev.ptr(s),
                               len(shape), i64(shape), i64(dstr), i64(sstr),
                               doff, soff, es), what)
    want = rt_ref.copy_box(dbuf, sbuf, shape, dstr, sstr, doff, soff)
    assert np.array_equal(rt_ref.read(want, doff, shape, dstr), sview), what
    check_written(dev.down(d), want, rt_ref.offsets(doff, shape, dstr), what)
    return dstr, sstr, doff, soff


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_copy_box_shapes_strides_offsets(dev, es):
    dtype = ES_DT[es]
    seen = set()
    for shape in COPY_SHAPES:
        for variant in COPY_VARIANTS:
            g = _run_copy(dev, *_copy_views(shape, dtype, variant),
                          (es, shape, variant))
            seen.add((variant, g[2] != G or g[3] != G,
                      any(x < 0 for x in g[1]), 0 in g[1]))
    # the variants really produce the geometry they are named for
    assert ("negative_src", True, True, False) in seen
    assert ("broadcast_src", False, False, True) in seen
    assert ("padded_offsets", True, False, False) in seen


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_copy_box_second_grid_stride_trip(dev, es):
    shape = (2049, 257)
    assert shape[0] * shape[1] > 2048 * 256        # the launch cap
    _run_copy(dev, *_copy_views(shape, ES_DT[es], "padded_offsets"),
              (es, shape))
    _run_copy(dev, *_copy_views(shape, ES_DT[es], "transposed_dst"),
              (es, shape, "T"))


def test_copy_box_zero_extent_writes_nothing(dev):
    for shape in [(0,), (3, 0, 5), (0, 4), (2, 3, 4, 0)]:
        dbuf = np.full(200, sentinel("int32"), dtype="int32")
        d, s = dev.up(dbuf), dev.up(dbuf + 1)
        st = [1] * len(shape)
        dev.ok(dev.lib.rt_copy_box(dev.stream(), dev.ptr(d), dev.ptr(s),
                                   len(shape), i64(shape), i64(st), i64(st),
                                   G, G, 4), shape)
        assert np.array_equal(dev.down(d), dbuf)


# =============================================================================
# rt_combine_box
# =============================================================================

def _combine_views(shape, dtype, variant, dvals, svals):
    dbuf, dbase = guarded(shape, dtype, dvals)
    sbuf, sbase = guarded(shape, dtype, svals)
    dview, sview = dbase, sbase
    if variant == "src_stride0":          # the axcs_apply broadcast
        ax = len(shape) - 2
        sshape = tuple(1 if d == ax else s for d, s in enumerate(shape))
        sbuf, sbase = guarded(sshape, dtype, svals)
        sview = np.broadcast_to(sbase, shape)
    elif variant == "strided_dst":        # padded container, nonzero offset
        dshape, dsl = pad_view(shape, 1, 3)
        dbuf, dbase = guarded(dshape, dtype)
        dview = dbase[dsl]
        dview[...] = np.asarray(dvals).reshape(-1)[:dview.size].reshape(shape)
    return dbuf, dview, sbuf, sview


def _run_combine(dev, dbuf, dview, sbuf, sview, op, what, nan_ok=False):
    shape = dview.shape
    doff, dstr = geom(dview, dbuf)
    soff, sstr = geom(sview, sbuf)
    inb(dbuf.size, doff, shape, dstr, what)
    inb(sbuf.size, soff, shape, sstr, what)
    d, s = dev.up(dbuf), dev.up(sbuf)
    dev.ok(dev.lib.rt_combine_box(
        dev.stream(), dev.ptr(d), dev.ptr(s), len(shape), i64(shape),
        i64(dstr), i64(sstr), doff, soff, DT7.index(str(dbuf.dtype)),
        OPS.index(op)), what)
    want = rt_ref.combine_box(dbuf, sbuf, shape, dstr, sstr, doff, soff, op)
    with np.errstate(all="ignore"):
        assert np.array_equal(rt_ref.read(want, doff, shape, dstr),
                              rt_ref.combine(dview, sview, op),
                              equal_nan=nan_ok), what
    got = dev.down(d)
    check_written(got, want, rt_ref.offsets(doff, shape, dstr), what, nan_ok)
    return got, rt_ref.offsets(doff, shape, dstr)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DT7)
def test_combine_box_every_dtype_and_op(dev, dtype, op):
    for shape in rc.COMBINE_SHAPES:
        n = int(np.prod(shape))
        dv, sv = rc.combine_inputs(dtype, op, n)
        for variant in ("dense", "src_stride0", "strided_dst"):
            got, box = _run_combine(
                dev, *_combine_views(shape, dtype, variant, dv, sv), op,
                (dtype, op, shape, variant))
            if op in ("land", "lor"):
                res = got[box.reshape(-1)]
                assert set(np.unique(res).tolist()) <= {0, 1}
                assert 0 in res and 1 in res


@pytest.mark.parametrize("op", ["min", "max"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_combine_box_float_minmax_propagates_nan(dev, dtype, op):
    shape = (5, 130)
    n = 650
    dv, sv = rc.combine_inputs(dtype, op, n)
    dv[3::7] = np.nan            # NaN on the dst side,
    sv[5::7] = np.nan            # on the src side,
    dv[6::14] = sv[6::14] = np.nan   # and on both
    for variant in ("dense", "strided_dst"):
        got, box = _run_combine(
            dev, *_combine_views(shape, dtype, variant, dv, sv), op,
            (dtype, op, variant), nan_ok=True)
        res = got[box.reshape(-1)]
        assert np.array_equal(np.isnan(res), np.isnan(dv) | np.isnan(sv))


@pytest.mark.parametrize("dtype,op", rc.COMBINE_BIG_CASES)
def test_combine_box_second_grid_stride_trip(dev, dtype, op):
    shape = rc.COMBINE_BIG
    n = shape[0] * shape[1]
    assert n > 2048 * 256
    dv, sv = rc.combine_inputs(dtype, op, n)
    _run_combine(dev, *_combine_views(shape, dtype, "strided_dst", dv, sv),
                 op, (dtype, op, shape))


# =============================================================================
# rt_cumsum phases 1, 2, 3
# =============================================================================

def _bases(dtype):
    """(fbase, ibase): the one the dtype uses is nonzero, and the other is a
    decoy that must not reach the result."""
    if np.dtype(dtype).kind == "f":
        return rc.F_BASE, 77777
    return 55555.0, rc.I_BASE


def _cumsum_case(dev, dtype, n, stride, grid=None):
    C, lib, what = dev.C, dev.lib, (dtype, n, stride, grid)
    code = DT4.index(dtype)
    x = rc.cumsum_input(dtype, n)
    span = (n - 1) * abs(stride) + 1
    ibuf = np.full(span + 2 * G, sentinel(dtype), dtype=dtype)
    in_off = G if stride > 0 else G + span - 1
    inb(ibuf.size, in_off, (n,), (stride,), what)
    ibuf[in_off + np.arange(n) * stride] = x
    assert np.array_equal(rt_ref.line(ibuf, in_off, stride, n), x)
    nb = -(-n // C)
    grid = nb if grid is None else grid
    it = dev.up(ibuf)
    bs = dev.full(nb + 2 * G, dtype)
    st = dev.stream()
    # phase 1: chunk sums.  block b writes bsums[b], b < nb
    dev.ok(lib.rt_cumsum(st, dev.ptr(it), in_off, stride, n, None, 0,
                         dev.ptr(bs, G), grid, None, 0.0, 0, code, 1), what)
    want_bs = np.full(nb + 2 * G, sentinel(dtype), dtype=dtype)
    want_bs[G:G + nb] = rt_ref.chunk_sums(x, C)
    check_written(dev.down(bs), want_bs, np.arange(G, G + nb), (what, 1))
    # phase 2: exclusive prefixes of the nb sums in place, and the total
    tot = dev.full(3, dtype)
    dev.ok(lib.rt_cumsum(st, None, 0, 0, 0, None, 0, dev.ptr(bs, G), nb,
                         dev.ptr(tot, 1), 0.0, 0, code, 2), what)
    excl, total = rt_ref.exclusive_scan(want_bs[G:G + nb])
    want_bs[G:G + nb] = excl
    check_written(dev.down(bs), want_bs, np.arange(G, G + nb), (what, 2))
    want_tot = np.full(3, sentinel(dtype), dtype=dtype)
    want_tot[1] = total
    check_written(dev.down(tot), want_tot, [1], (what, "total"))
    assert total == x.sum(dtype=np.float64 if code < 2 else np.int64)
    # phase 3: base + prefix, dense out at a nonzero offset
    out_off = G + 5
    ot = dev.full(n + 2 * G + 5, dtype)
    inb(n + 2 * G + 5, out_off, (n,), (1,), what)
    fbase, ibase = _bases(dtype)
    dev.ok(lib.rt_cumsum(st, dev.ptr(it), in_off, stride, n, dev.ptr(ot),
                         out_off, dev.ptr(bs, G), grid, None, fbase, ibase,
                         code, 3), what)
    want = np.full(n + 2 * G + 5, sentinel(dtype), dtype=dtype)
    want[out_off:out_off + n] = rt_ref.cumsum_apply(x, excl, rc.base_of(dtype),
                                                    C)
    assert np.array_equal(want[out_off:out_off + n],
                          rt_ref.cumsum_full(x, rc.base_of(dtype)))
    check_written(dev.down(ot), want, np.arange(out_off, out_off + n),
                  (what, 3))
    # the input is read-only
    assert np.array_equal(dev.down(it), ibuf)


@pytest.mark.parametrize("stride", rc.CUMSUM_STRIDES)
@pytest.mark.parametrize("dtype", DT4)
def test_cumsum_phases_at_the_seams(dev, dtype, stride):
    for n in rc.cumsum_ns(dev.C):
        _cumsum_case(dev, dtype, n, stride)


@pytest.mark.parametrize("dtype", DT4)
def test_cumsum_three_blocks_over_thirteen_chunks(dev, dtype):
    """Phases 1 and 3 with a grid smaller than the chunk count: each block
    makes several trips and reuses its LDS."""
    n = rc.cumsum_trips_n(dev.C)
    assert -(-n // dev.C) == 13
    _cumsum_case(dev, dtype, n, 1, grid=3)
    _cumsum_case(dev, dtype, n, -1, grid=3)


@pytest.mark.parametrize("dtype", DT4)
def test_cumsum_phase2_alone(dev, dtype):
    code = DT4.index(dtype)
    for L in rc.PHASE2_LENGTHS:
        b = rc.phase2_input(dtype, L)
        buf = np.full(L + 2 * G, sentinel(dtype), dtype=dtype)
        buf[G:G + L] = b
        bs, tot = dev.up(buf), dev.full(3, dtype)
        dev.ok(dev.lib.rt_cumsum(dev.stream(), None, 0, 0, 0, None, 0,
                                 dev.ptr(bs, G), L, dev.ptr(tot, 1), 0.0, 0,
                                 code, 2), (dtype, L))
        excl, total = rt_ref.exclusive_scan(b)
        want = buf.copy()
        want[G:G + L] = excl
        check_written(dev.down(bs), want, np.arange(G, G + L), (dtype, L))
        got_tot = dev.down(tot)
        assert got_tot.dtype == b.dtype and got_tot[1] == total
        assert got_tot[0] == got_tot[2] == sentinel(dtype)


# =============================================================================
# rt_axis_scan
# =============================================================================

def _axis_case(dev, dtype, shape, axis, nchunks, big=False):
    what = (dtype, shape, axis, nchunks)
    nd = len(shape)
    x = rc.axis_input(dtype, shape)
    if big:       # dense input, out padded on the last axis only
        ibuf, iview = guarded(shape, dtype, x)
        obuf, obase = guarded(shape[:-1] + (shape[-1] + 1,), dtype)
        oview = obase[..., :shape[-1]]
    else:         # input: a sliced and transposed view; out: padded container
        ibuf, ibase = guarded(tuple(2 * s + 1 for s in reversed(shape)), dtype)
        iview = ibase[tuple(slice(1, None, 2) for _ in shape)].T
        iview[...] = x
        oshape, osl = pad_view(shape, 1, 3)
        obuf, obase = guarded(oshape, dtype)
        oview = obase[osl]
    assert iview.shape == oview.shape == tuple(shape)
    ioff, istr = geom(iview, ibuf)
    ooff, ostr = geom(oview, obuf)
    inb(ibuf.size, ioff, shape, istr, what)
    inb(obuf.size, ooff, shape, ostr, what)
    nlines = x.size // shape[axis]
    it, ot = dev.up(ibuf), dev.up(obuf)
    tt = dev.full(nlines + 2 * G, dtype)
    t2 = dev.full(nchunks * nlines + 2 * G, dtype) if nchunks > 1 else None
    dev.ok(dev.lib.rt_axis_scan(
        dev.stream(), dev.ptr(it, ioff), dev.ptr(ot, ooff), dev.ptr(tt, G),
        nd, i64(shape), i64(istr), i64(ostr), axis, DT4.index(dtype),
        dev.ptr(t2, G) if t2 is not None else None, nchunks), what)
    want, want_tot = rt_ref.axis_scan(obuf, ibuf, shape, istr, ostr, ioff,
                                      ooff, axis)
    check_written(dev.down(ot), want, rt_ref.offsets(ooff, shape, ostr), what)
    wt = np.full(nlines + 2 * G, sentinel(dtype), dtype=dtype)
    wt[G:G + nlines] = want_tot      # = the last element of each line
    assert np.array_equal(
        want_tot, np.take(rt_ref.read(want, ooff, shape, ostr),
                          shape[axis] - 1, axis=axis).reshape(-1))
    check_written(dev.down(tt), wt, np.arange(G, G + nlines), (what, "tot"))
    if t2 is not None:               # scratch: only its guards are asserted
        g2 = dev.down(t2)
        assert np.all(g2[:G] == sentinel(dtype)), what
        assert np.all(g2[G + nchunks * nlines:] == sentinel(dtype)), what
    assert np.array_equal(dev.down(it), ibuf)


@pytest.mark.parametrize("nd", [2, 3, 4])
@pytest.mark.parametrize("dtype", DT4)
def test_axis_scan_every_axis_and_regime(dev, dtype, nd):
    shape = rc.AXIS_SHAPES[nd]
    for axis in range(nd):
        _axis_case(dev, dtype, shape, axis, 1)      # lines, or waves if last
        for nchunks in rc.AXIS_CHUNKS:              # chunked, uneven split
            assert shape[axis] % nchunks != 0
            _axis_case(dev, dtype, shape, axis, nchunks)


@pytest.mark.parametrize("dtype", DT4)
def test_axis_scan_wave_per_line_lengths(dev, dtype):
    for L in rc.WAVE_LENGTHS:
        _axis_case(dev, dtype, (5, L), 1, 1)
        _axis_case(dev, dtype, (3, 4, L), 2, 1)


@pytest.mark.parametrize("dtype", DT4)
def test_axis_scan_chunked_with_an_empty_trailing_chunk(dev, dtype):
    shape, axis, nchunks = rc.EMPTY_TAIL
    clen = -(-shape[axis] // nchunks)
    assert (nchunks - 1) * clen >= shape[axis]      # the last range is empty
    _axis_case(dev, dtype, shape, axis, nchunks)


@pytest.mark.parametrize("name,shape,axis,nchunks,dtype", rc.AXIS_BIG)
def test_axis_scan_second_grid_stride_trip(dev, name, shape, axis, nchunks,
                                           dtype):
    nlines = int(np.prod(shape)) // shape[axis]
    cap = 4096 * 256                                # threads in a capped grid
    if name == "waves":
        assert axis == len(shape) - 1 and nlines > cap // 64
    elif name == "lines":
        assert axis != len(shape) - 1 and nchunks == 1 and nlines > cap
    else:
        assert nlines * nchunks > cap and nlines * (nchunks - 1) > cap
    _axis_case(dev, dtype, shape, axis, nchunks, big=True)


# =============================================================================
# rt_mask_compact phases 1 and 3, rt_cumsum phase 2 between them
# =============================================================================

PATTERNS = ["none", "all", "third", "first", "last", "full_then_empty"]


def mask_pattern(name, n, M):
    i = np.arange(n)
    sel = {"none": np.zeros(n, bool), "all": np.ones(n, bool),
           "third": i % 3 == 0, "first": i == 0, "last": i == n - 1,
           "full_then_empty": (i // M) % 2 == 0}[name]
    # a selected byte is any nonzero value, not just 1
    return np.where(sel, 1 + i % 255, 0).astype(np.uint8)


def _mask_case(dev, abuf, aview, mbuf, mview, what, vec=None):
    lib, M = dev.lib, dev.M
    shape, dtype = aview.shape, str(abuf.dtype)
    aoff, astr = geom(aview, abuf)
    moff, mstr = geom(mview, mbuf)
    inb(abuf.size, aoff, shape, astr, what)
    inb(mbuf.size, moff, shape, mstr, what)
    n = aview.size
    nchunks = -(-n // M)
    at, mt = dev.up(abuf), dev.up(mbuf)
    a_ptr, m_ptr = dev.ptr(at, aoff), dev.ptr(mt, moff)
    if vec is not None:      # which phase-1 kernel this geometry selects
        assert (len(shape) == 1 and mstr[0] == 1
                and m_ptr.value % 8 == 0) == vec, what
    code = DT7.index(dtype)
    st = dev.stream()
    bc = dev.full(nchunks + 2 * G, "int64")
    args = (len(shape), i64(shape), i64(astr), i64(mstr), dev.ptr(bc, G),
            nchunks, code)
    dev.ok(lib.rt_mask_compact(st, a_ptr, m_ptr, None, *args, 1), what)
    want_bc = np.full(nchunks + 2 * G, sentinel("int64"), dtype="int64")
    want_bc[G:G + nchunks] = rt_ref.mask_counts(mbuf, moff, shape, mstr, M)
    check_written(dev.down(bc), want_bc, np.arange(G, G + nchunks), (what, 1))
    tot = dev.full(3, "int64")
    dev.ok(lib.rt_cumsum(st, None, 0, 0, 0, None, 0, dev.ptr(bc, G), nchunks,
                         dev.ptr(tot, 1), 0.0, 0, 2, 2), what)
    want_sel = rt_ref.mask_compact(abuf, mbuf, aoff, moff, shape, astr, mstr)
    assert np.array_equal(want_sel, aview[mview != 0])
    count = want_sel.size
    got_tot = dev.down(tot)
    assert got_tot[1] == count and got_tot[0] == got_tot[2] == -99, what
    ot = dev.full(count + 2 * G, dtype)
    dev.ok(lib.rt_mask_compact(st, a_ptr, m_ptr, dev.ptr(ot, G), *args, 3),
           what)
    want = np.full(count + 2 * G, sentinel(dtype), dtype=dtype)
    want[G:G + count] = want_sel
    check_written(dev.down(ot), want, np.arange(G, G + count), (what, 3))


def _mask_1d(dev, dtype, n, pattern, mode):
    m = mask_pattern(pattern, n, dev.M)
    abuf, aview = guarded((n,), dtype, distinct(n, dtype))
    if mode == "vec":            # 8-byte-aligned, stride 1: uint64 loads
        mbuf, mview = guarded((n,), "uint8", m)
    elif mode == "byte_off":     # the pointer advanced by one byte
        mbuf = np.zeros(n + 2 * G + 1, dtype=np.uint8)
        mview = mbuf[G + 1:G + 1 + n]
        mview[...] = m
    else:                        # mask stride 2; value stride 3
        mbuf, mbase = guarded((2 * n,), "uint8")
        mview = mbase[::2]
        mview[...] = m
        abuf, abase = guarded((3 * n,), dtype)
        aview = abase[::3]
        aview[...] = distinct(n, dtype)
    _mask_case(dev, abuf, aview, mbuf, mview, (dtype, n, pattern, mode),
               vec=(mode == "vec"))


@pytest.mark.parametrize("dtype", DT7)
def test_mask_compact_1d_sizes_patterns_and_count_paths(dev, dtype):
    M = dev.M
    for n in [1, 7, 8, 9, M - 1, M, M + 1, 3 * M + 5]:
        for pattern in PATTERNS:
            for mode in ("vec", "byte_off", "stride2"):
                _mask_1d(dev, dtype, n, pattern, mode)


@pytest.mark.parametrize("shape", [(37, 59), (5, 21, 23), (3, 5, 7, 29)])
@pytest.mark.parametrize("dtype", DT7)
def test_mask_compact_nd_padded_strides(dev, dtype, shape):
    """Value and mask containers padded differently: two stride sets."""
    n = int(np.prod(shape))
    assert n > dev.M
    for pattern in ("third", "full_then_empty", "last"):
        ashape, asl = pad_view(shape, 1, 2)
        mshape, msl = pad_view(shape, 2, 5)
        abuf, abase = guarded(ashape, dtype)
        mbuf, mbase = guarded(mshape, "uint8")
        mbuf[...] = 9        # padding bytes are nonzero: must not be counted
        aview, mview = abase[asl], mbase[msl]
        aview[...] = distinct(n, dtype).reshape(shape)
        mview[...] = mask_pattern(pattern, n, dev.M).reshape(shape)
        _mask_case(dev, abuf, aview, mbuf, mview, (dtype, shape, pattern),
                   vec=False)


def test_mask_compact_second_grid_stride_trip(dev):
    M = dev.M
    n = 2048 * M + M + 1
    assert -(-n // M) > 2048                        # the grid cap, in chunks
    for mode in ("vec", "byte_off"):
        _mask_1d(dev, "int16", n, "third", mode)


# =============================================================================
# rt_flat_copy, gather and scatter
# =============================================================================

def _flat_views(shape, dtype, kind):
    n = int(np.prod(shape))
    if kind == "contiguous":
        buf, view = guarded(shape, dtype)
    elif kind == "padded":
        pshape, sl = pad_view(shape, 1, 2)
        buf, base = guarded(pshape, dtype)
        view = base[sl]
    elif kind == "transposed":
        buf, base = guarded(tuple(reversed(shape)), dtype)
        view = base.T
    elif kind == "stride3":
        buf, base = guarded((3 * n,), dtype)
        view = base[::3]
    elif kind == "reversed":
        buf, base = guarded((n,), dtype)
        view = base[::-1]
    view[...] = distinct(n, dtype).reshape(shape)
    return buf, view


class FlatBox:
    """One strided box on the device, reused by many (flat0, n) subranges."""

    def __init__(self, dev, shape, dtype, kind):
        self.dev, self.shape, self.dtype = dev, tuple(shape), dtype
        self.buf, self.view = _flat_views(shape, dtype, kind)
        self.off, self.str = geom(self.view, self.buf)
        inb(self.buf.size, self.off, shape, self.str, (shape, kind))
        self.n_all = self.view.size
        self.t = dev.up(self.buf)
        self.blank = np.full(self.buf.size, sentinel(dtype), dtype=dtype)
        self.tblank = dev.up(self.blank)
        self.vals = (distinct(self.n_all, dtype)[::-1] // 2).astype(dtype)
        self.tvals = dev.up(self.vals)
        self.box = rt_ref.offsets(self.off, shape, self.str).reshape(-1)

    def call(self, boxed_t, dense_ptr, flat0, n, scatter, what):
        dev = self.dev
        assert 0 <= flat0 and 0 <= n and flat0 + n <= self.n_all, what
        dev.ok(dev.lib.rt_flat_copy(
            dev.stream(), dev.ptr(boxed_t, self.off), dense_ptr,
            len(self.shape), i64(self.shape), i64(self.str), flat0, n,
            self.buf.itemsize, scatter), what)

    def gather(self, flat0, n):
        what = ("gather", self.shape, self.str, flat0, n)
        dense = self.tblank[:n + 2 * G].clone()
        self.call(self.t, self.dev.ptr(dense, G), flat0, n, 0, what)
        want = np.full(n + 2 * G, sentinel(self.dtype), dtype=self.dtype)
        want[G:G + n] = rt_ref.flat_gather(self.buf, self.off, self.shape,
                                           self.str, flat0, n)
        assert np.array_equal(want[G:G + n],
                              self.view.reshape(-1)[flat0:flat0 + n])
        check_written(self.dev.down(dense), want, np.arange(G, G + n), what)

    def scatter(self, flat0, n):
        what = ("scatter", self.shape, self.str, flat0, n)
        boxed = self.tblank.clone()
        self.call(boxed, self.dev.ptr(self.tvals), flat0, n, 1, what)
        want = rt_ref.flat_scatter(self.blank, self.vals, self.off,
                                   self.shape, self.str, flat0, n)
        # every other element of the box, and of the buffer, is untouched
        check_written(self.dev.down(boxed), want, self.box[flat0:flat0 + n],
                      what)


@pytest.mark.parametrize("scatter", [0, 1])
@pytest.mark.parametrize("kind", ["contiguous", "padded", "transposed"])
def test_flat_copy_every_subrange_of_small_boxes(dev, kind, scatter):
    """Exhaustive: every (flat0, n) of (3,5) and (2,3,4), every elemsize —
    mid-row starts, partial first and last rows, single elements."""
    launches = 0
    for shape in [(3, 5), (2, 3, 4)]:
        for es in (1, 2, 4, 8):
            fb = FlatBox(dev, shape, ES_DT[es], kind)
            for flat0 in range(fb.n_all + 1):
                for n in range(fb.n_all - flat0 + 1):
                    (fb.scatter if scatter else fb.gather)(flat0, n)
                    launches += 1
    assert launches == 4 * (16 * 17 // 2 + 25 * 26 // 2)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_flat_copy_1d_strides(dev, es):
    for kind in ("contiguous", "stride3", "reversed"):
        fb = FlatBox(dev, (1000,), ES_DT[es], kind)
        for flat0, n in [(0, 1000), (1, 998), (255, 257), (999, 1), (0, 256),
                         (500, 0)]:
            fb.gather(flat0, n)
            fb.scatter(flat0, n)
    assert fb.str == (-1,)


@pytest.mark.parametrize("shape", [(3, 70001), (2, 200001)])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_flat_copy_column_chunks_per_row(dev, es, shape):
    """Few rows, inner extent above 65536: each row is split over several
    blocks.  The subrange starts and ends mid-row."""
    inner = shape[1]
    flat0 = inner // 3
    n = shape[0] * inner - flat0 - inner // 5
    rows = -(-n // inner) + 1                       # the launch arithmetic
    assert rows < 2048 and min(2048 // rows, -(-inner // 65536)) > 1
    assert flat0 % inner and (flat0 + n) % inner
    for kind in ("contiguous", "padded"):
        fb = FlatBox(dev, shape, ES_DT[es], kind)
        fb.gather(flat0, n)
        fb.scatter(flat0, n)
        fb.gather(0, fb.n_all)
        fb.scatter(0, fb.n_all)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_flat_copy_more_rows_than_blocks(dev, es):
    shape = (5000, 3)
    assert shape[0] > 4096                          # the grid cap, in rows
    for kind in ("contiguous", "padded", "transposed"):
        fb = FlatBox(dev, shape, ES_DT[es], kind)
        for flat0, n in [(0, 15000), (4, 14990), (1, 4096 * 3 + 2)]:
            fb.gather(flat0, n)
            fb.scatter(flat0, n)


# =============================================================================
# the same kernels through the frontend (the host's own geometry)
# =============================================================================

def _fe_mask(ra, h, m):
    got = ra.fromarray(h)[ra.fromarray(m)].asarray()
    want = h[m]
    assert got.dtype == want.dtype and got.shape == want.shape, (h.dtype,
                                                                 got.dtype)
    assert np.array_equal(got, want), (h.dtype, h.shape)


@pytest.mark.parametrize("dtype", ["int8", "int16", "bool", "int32",
                                   "float32"])
def test_frontend_mask_getitem_small_dtypes(ra_gpu, dev, dtype):
    """a[mask] for the value dtypes behind the RT_DTYPE mapping."""
    M = dev.M
    rng = np.random.default_rng(5)
    for shape in [(M - 1,), (M + 1,), (7, 13, 29)]:
        n = int(np.prod(shape))
        if dtype == "bool":
            h = rng.integers(0, 2, n).astype(bool).reshape(shape)
        else:
            h = distinct(n, dtype).reshape(shape)
        m = (np.arange(n) % 3 == 0).reshape(shape)
        _fe_mask(ra_gpu, h, m)
        _fe_mask(ra_gpu, h, np.zeros(shape, dtype=bool))   # selects nothing
        _fe_mask(ra_gpu, h, np.ones(shape, dtype=bool))


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_frontend_reshape_every_elemsize(ra_gpu, es):
    h = distinct(37 * 53, ES_DT[es]).reshape(37, 53)
    for view, hv in [(lambda a: a, h), (lambda a: a.T, h.T)]:
        for newshape in [(53, 37), (1961,)]:
            got = view(ra_gpu.fromarray(h)).reshape(newshape).asarray()
            want = hv.reshape(newshape)
            assert got.dtype == want.dtype and np.array_equal(got, want), (
                es, newshape)


def test_frontend_flat_cumsum_views_and_cast(ra_gpu, dev):
    C = dev.C
    for n in (C - 1, C + 1):
        h = rc.small_ints((3 * n + 7,), "int64", "fe")
        for view in (lambda a: a[2:2 + 3 * n:3], lambda a: a[::-1][:n],
                     lambda a: a[3 * n::-3][:n], lambda a: a[5:5 + n]):
            got = view(ra_gpu.fromarray(h)).cumsum().asarray()
            want = view(h).cumsum()
            assert got.dtype == want.dtype == np.int64
            assert np.array_equal(got, want), n
        h32 = rc.small_ints((n,), "int32", "fe")    # cast path: int32 -> int64
        got = ra_gpu.fromarray(h32).cumsum().asarray()
        assert got.dtype == np.int64 and np.array_equal(got, h32.cumsum())
        got = ra_gpu.fromarray(h32)[::-1].cumsum().asarray()
        assert np.array_equal(got, h32[::-1].cumsum())


def test_frontend_flat_cumsum_second_trip_of_the_host_grid(ra_gpu, dev):
    """Just above 4096 chunks: the host caps the phase 1 / 3 grid at 4096
    blocks, so the first blocks take a second trip."""
    n = 4096 * dev.C + dev.C + 3
    h = rc.small_ints((n,), "int64", "fe-big")
    got = ra_gpu.fromarray(h).cumsum().asarray()
    assert got.dtype == np.int64 and np.array_equal(got, np.cumsum(h))
