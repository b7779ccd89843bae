"""median / percentile / quantile: the canonical key on the host, and the
portable host hook of the radix select.

`runtime.select_op` finds order statistics with an MSD radix select over the
canonical sort key (include/ramba_sortkey.h).  It counts through one backend
hook:

    select_pass(source, shift, prefixes, collect) -> (counts, nan_count,
                                                      collected)
        source: a BoxSource (the rank's view-space box of the operand, read
            in place) or a KeySource (canonical keys collected earlier);
        shift: the bit position of this pass's 8-bit digit;
        prefixes: up to NQ_MAX distinct Python ints, the key bits above
            shift + 8 that are decided, in place;
        collect: None, or how many keys of this rank match a prefix: they are
            gathered, in any order, into the KeySource returned third;
        counts: a torch int64 tensor (len(prefixes), 256), counts[q][d] = how
            many keys match prefixes[q] and have digit d;
        nan_count: a 1-element torch int64 tensor, the NaNs of a BoxSource of
            floats (all of them, whatever the prefixes).

`HipBackend` implements it on the rt_select_pass kernel.  A backend without it
(the NumPy oracle backend, which is frozen test infrastructure) gets
`HostSelect`, built only on box_to_numpy and the NumPy restatement of the key
below.  The reference has no order statistics.
"""

import numpy as np

from .shardview import box_shape, c_strides

NQ_MAX = 8          # prefixes per launch (SELECT_NQ_MAX)
DIGIT_BITS = 8


class BoxSource:
    """The box `lb` of `view` that this rank owns of `bd`."""

    def __init__(self, bd, rt, view, lb):
        self.bd, self.rt, self.view, self.lb = bd, rt, view, lb


class KeySource:
    """Collected canonical keys (a dense 1-D backend buffer of the unsigned
    type of `dtype`'s width)."""

    def __init__(self, keys, dtype):
        self.keys, self.dtype = keys, np.dtype(dtype)


def key_dtype(dtype):
    return np.dtype(f"u{np.dtype(dtype).itemsize}")


def canon(x):
    """rt_sort_canon in NumPy: the unsigned keys of the 1-D array `x`."""
    x = np.ascontiguousarray(x)
    kind = "u" if x.dtype == np.bool_ else x.dtype.kind
    U = key_dtype(x.dtype)
    u = x.view(U)
    sign = U.type(1 << (8 * U.itemsize - 1))
    if kind == "i":
        return u ^ sign
    if kind != "f":
        return u
    mbits = 23 if U.itemsize == 4 else 52
    inf = U.type(((1 << (8 * U.itemsize - 1)) - 1) >> mbits << mbits)
    mag = u & U.type(sign - 1)
    k = np.where(u & sign != 0, ~u, u | sign)
    k[mag == 0] = sign
    k[mag > inf] = U.type(~U.type(0))
    return k


def decode(key, dtype):
    """rt_sort_decode in NumPy: the element of `dtype` (bool as uint8) that
    the canonical key `key`, a Python int, stands for.  A zero is +0.0 and a
    NaN the default quiet NaN."""
    dtype = np.dtype(np.uint8 if dtype == np.bool_ else dtype)
    U = key_dtype(dtype)
    bits = 8 * U.itemsize
    sign, ones = 1 << (bits - 1), (1 << bits) - 1
    if dtype.kind == "f":
        mbits = 23 if bits == 32 else 52
        if key == ones:
            raw = (sign - 1) >> (mbits - 1) << (mbits - 1)
        else:
            raw = key ^ sign if key & sign else ~key & ones
    else:
        raw = key ^ sign if dtype.kind == "i" else key
    return np.array([raw], dtype=U).view(dtype)[0]


def hooks_for(backend):
    """The object serving the hook for `backend`."""
    if hasattr(backend, "select_pass"):
        return backend
    return HostSelect(backend)


class HostSelect:
    """Portable host implementation of the select hook."""

    def __init__(self, backend):
        self.backend = backend

    def select_pass(self, source, shift, prefixes, collect):
        import torch
        nan = 0
        if isinstance(source, KeySource):
            keys = source.keys
            dtype = source.dtype
        else:
            bd, rt, view, lb = source.bd, source.rt, source.view, source.lb
            dtype = np.dtype(bd.dtype)
            core = rt.core_box(bd, rt.rank)
            local = self.backend.box_to_numpy(bd, rt, core)
            # the operand is read in place through the view's strides
            off0, strides = view.operand_addressing(
                lb[0], c_strides(local.shape), core[0], (0,) * local.ndim)
            flat = local.reshape(-1)
            x = np.lib.stride_tricks.as_strided(
                flat[off0:] if off0 else flat, shape=box_shape(lb),
                strides=tuple(s * local.itemsize for s in strides))
            keys = canon(x.reshape(-1))
            if dtype.kind == "f":
                nan = int(np.count_nonzero(keys == ~keys.dtype.type(0)))
        width = 8 * dtype.itemsize
        top = shift + DIGIT_BITS
        k64 = keys.astype(np.uint64)
        hi = k64 >> np.uint64(top) if top < 64 else np.zeros_like(k64)
        digit = ((k64 >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        counts = np.zeros((len(prefixes), 256), dtype=np.int64)
        taken = np.zeros(keys.shape, dtype=bool)
        for q, p in enumerate(prefixes):
            assert top <= width and p >> top << top == p, (p, shift)
            sel = hi == np.uint64(p >> top if top < 64 else 0)
            counts[q] = np.bincount(digit[sel], minlength=256)
            taken |= sel
        got = None
        if collect is not None:
            got = KeySource(keys[taken], dtype)
            assert got.keys.size == collect, (got.keys.size, collect)
        return (torch.from_numpy(counts),
                torch.tensor([nan], dtype=torch.int64), got)
