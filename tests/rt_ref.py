"""NumPy models of the older ramba_rt entry points (rt_copy_box,
rt_combine_box, rt_cumsum, rt_axis_scan, rt_mask_compact, rt_flat_copy).

Every model works on FLAT host arrays (the image of a device allocation)
and on the (off, shape, strides) triples the C ABI takes, all in elements.
They are plain index arithmetic; tests/test_rt_ref_host.py checks them
against ordinary NumPy slicing, so the GPU suite
(tests/test_gpu_rt_kernels.py) compares the kernels with a known quantity.
Models return new arrays and never modify their arguments."""

import numpy as np

# dtype codes of the C ABI
DT7 = ["float64", "float32", "int64", "int32", "int16", "int8", "uint8"]
DT4 = DT7[:4]
OPS = ["add", "mul", "min", "max", "land", "lor"]


def offsets(off, shape, strides):
    """Element offset of every box coordinate, as an array of `shape`."""
    o = np.full(tuple(shape), int(off), dtype=np.int64)
    for d, (n, s) in enumerate(zip(shape, strides)):
        sh = [1] * len(shape)
        sh[d] = n
        o = o + (np.arange(n, dtype=np.int64) * int(s)).reshape(sh)
    return o


def reach(off, shape, strides):
    """(lowest, highest) element offset the box touches; None if empty."""
    if any(n == 0 for n in shape):
        return None
    lo = hi = int(off)
    for n, s in zip(shape, strides):
        span = (int(n) - 1) * int(s)
        if span < 0:
            lo += span
        else:
            hi += span
    return lo, hi


def geom(view, buf):
    """(off, strides) in elements of NumPy `view` inside flat array `buf`."""
    isz = buf.itemsize
    d = view.__array_interface__["data"][0] - buf.__array_interface__["data"][0]
    assert d % isz == 0 and all(s % isz == 0 for s in view.strides)
    return d // isz, tuple(s // isz for s in view.strides)


def read(buf, off, shape, strides):
    return buf[offsets(off, shape, strides)]


# -- rt_copy_box / rt_combine_box ---------------------------------------------

def copy_box(dst, src, shape, dstr, sstr, doff, soff):
    out = dst.copy()
    out[offsets(doff, shape, dstr).reshape(-1)] = \
        src[offsets(soff, shape, sstr).reshape(-1)]
    return out


def combine(d, s, op):
    """dst OP src in the operands' own dtype (small integers wrap)."""
    dt = d.dtype
    if op == "add":
        r = d + s
    elif op == "mul":
        r = d * s
    elif op == "min":
        r = np.minimum(d, s)       # NaN from either side propagates
    elif op == "max":
        r = np.maximum(d, s)
    elif op == "land":
        r = (d != 0) & (s != 0)
    elif op == "lor":
        r = (d != 0) | (s != 0)
    else:
        raise ValueError(op)
    return r.astype(dt)


def combine_box(dst, src, shape, dstr, sstr, doff, soff, op):
    out = dst.copy()
    do = offsets(doff, shape, dstr).reshape(-1)
    so = offsets(soff, shape, sstr).reshape(-1)
    with np.errstate(all="ignore"):
        out[do] = combine(dst[do], src[so], op)
    return out


# -- rt_cumsum ----------------------------------------------------------------

def line(buf, off, stride, n):
    return buf[off + np.arange(n, dtype=np.int64) * stride]


def chunk_sums(x, chunk):
    """Phase 1: the sum of each `chunk`-sized piece of 1-D x, in x's dtype."""
    nb = -(-x.size // chunk)
    return np.array([x[c * chunk:(c + 1) * chunk].sum(dtype=x.dtype)
                     for c in range(nb)], dtype=x.dtype)


def exclusive_scan(b):
    """Phase 2: (exclusive prefixes of b, grand total), in b's dtype."""
    inc = np.cumsum(b.astype(np.float64 if b.dtype.kind == "f" else b.dtype))
    inc = inc.astype(b.dtype)
    excl = np.concatenate([np.zeros(1, dtype=b.dtype), inc[:-1]])
    return excl, inc[-1]


def cumsum_apply(x, excl, base, chunk):
    """Phase 3: out[i] = base + excl[i // chunk] + inclusive scan of x inside
    chunk i // chunk.  Floats accumulate in float64 and are cast (the test
    inputs keep every partial sum exactly representable)."""
    acc = np.float64 if x.dtype.kind == "f" else x.dtype.type
    out = np.empty(x.size, dtype=x.dtype)
    for c in range(-(-x.size // chunk)):
        seg = x[c * chunk:(c + 1) * chunk].astype(acc)
        out[c * chunk:(c + 1) * chunk] = \
            (np.cumsum(seg) + acc(excl[c]) + acc(base)).astype(x.dtype)
    return out


def cumsum_full(x, base):
    """What phases 1-3 compute together: base + cumsum(x)."""
    acc = np.float64 if x.dtype.kind == "f" else x.dtype.type
    return (np.cumsum(x.astype(acc)) + acc(base)).astype(x.dtype)


def exact_float_sums(x, dtype, base=0):
    """True when every partial sum of integer-valued x (plus base) along the
    LAST axis is exact in `dtype` whatever the summation order: all values
    are integers with |x| <= 8 and sum(|x|) + |base| of each line stays
    under 2^24 (float32) / 2^53 (float64)."""
    x = np.asarray(x, dtype=np.float64)
    lim = 2.0 ** (24 if np.dtype(dtype) == np.float32 else 53)
    return bool(np.all(x == np.round(x)) and np.all(np.abs(x) <= 8)
                and np.abs(x).sum(axis=-1).max() + abs(float(base)) < lim)


# -- rt_axis_scan -------------------------------------------------------------

def axis_scan(out, inp, shape, istr, ostr, ioff, ooff, axis):
    """(new out, dense C-order line totals)."""
    v = read(inp, ioff, shape, istr)
    acc = np.float64 if v.dtype.kind == "f" else v.dtype
    c = np.cumsum(v.astype(acc), axis=axis).astype(v.dtype)
    res = out.copy()
    res[offsets(ooff, shape, ostr).reshape(-1)] = c.reshape(-1)
    totals = np.take(c, shape[axis] - 1, axis=axis).reshape(-1)
    return res, totals


# -- rt_mask_compact ----------------------------------------------------------

def mask_counts(m, moff, shape, mstr, chunk):
    """Phase 1: selected count per `chunk` elements in C order (int64)."""
    sel = read(m, moff, shape, mstr).reshape(-1) != 0
    nb = -(-sel.size // chunk)
    return np.array([sel[c * chunk:(c + 1) * chunk].sum() for c in range(nb)],
                    dtype=np.int64)


def mask_compact(a, m, aoff, moff, shape, astr, mstr):
    """Phase 3: the selected values, C order."""
    sel = read(m, moff, shape, mstr).reshape(-1) != 0
    return read(a, aoff, shape, astr).reshape(-1)[sel]


# -- rt_flat_copy -------------------------------------------------------------

def flat_gather(boxed, off, shape, strides, flat0, n):
    return boxed[offsets(off, shape, strides).reshape(-1)[flat0:flat0 + n]]


def flat_scatter(boxed, dense, off, shape, strides, flat0, n):
    out = boxed.copy()
    out[offsets(off, shape, strides).reshape(-1)[flat0:flat0 + n]] = dense[:n]
    return out
