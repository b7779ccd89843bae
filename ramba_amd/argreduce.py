"""argmax / argmin / nanargmax / nanargmin: the pair order restated for the
host, and the portable host hooks.

`runtime.arg_reduce_op` carries a (value, index) pair per result element
through two backend hooks:

    arg_reduce_partial(bd, rt, view, lb, axis, mult, idx0, kind, skipna)
        -> (vals, idxs): the rank's pair partial over its view-space box
           `lb`, as two torch tensors (shape (1,) for axis=None, else the
           box's shape with `axis` at extent 1).  The reported index of an
           element at local coordinates i is idx0 + sum_d i_d * mult_d;
           -1 means "no candidate" (skipna and the line is all NaN).
    arg_combine_box(out_bd, rt, box, best, rel, src_vals, src_idx, kind,
                    skipna)
        -> merges the dense pair box (src_vals, src_idx) into the running
           pair: values in `best[rel]` (a message buffer shaped like the
           rank's core box of the int64 result `out_bd`), indices in the
           result's container at `box`.

`HipBackend` implements them on the rt_arg_* kernels.  A backend without
them (the NumPy oracle backend, which is frozen test infrastructure) gets
`HostArg`: the same hooks built only on calls every backend has
(box_to_numpy / write_core_from_numpy), for host-memory backends whose
message buffers wrap NumPy arrays.

The merge rule (`better`) is the NumPy restatement of rt_arg_better in
include/ramba_argcmp.h; the flat cross-rank merge in the runtime uses it
too.  The reference has no counterpart (ramba/ramba.py:10288 lists argmin /
argmax as to-do).
"""

import numpy as np

from .shardview import box_shape, box_slices, c_strides


def hooks_for(backend):
    """The object serving the two hooks for `backend`."""
    if hasattr(backend, "arg_reduce_partial"):
        return backend
    return HostArg(backend)


def better(pv, pi, qv, qi, kind, skipna):
    """Elementwise: does pair p = (pv, pi) replace pair q = (qv, qi)?

    idx < 0 always loses; unless skipna a NaN beats every number and the
    lower-index NaN beats the other; otherwise > (max) / < (min), and on
    equal values the lower index."""
    pv, qv = np.asarray(pv), np.asarray(qv)
    pi, qi = np.asarray(pi), np.asarray(qi)
    if pv.dtype.kind == "f":
        pn, qn = np.isnan(pv), np.isnan(qv)
    else:
        pn = np.zeros(pv.shape, dtype=bool)
        qn = np.zeros(qv.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        strict = (pv > qv) if kind == "max" else (pv < qv)
        tie = (pv == qv) & (pi < qi)
    if skipna:
        return (pi >= 0) & ~pn & ((qi < 0) | qn | strict | tie)
    nan_rule = pn & (~qn | (pi < qi))
    return (pi >= 0) & ((qi < 0)
                        | np.where(pn | qn, nan_rule, strict | tie))


def local_pairs(x, gidx, axis, kind, skipna):
    """(vals, idxs) of a host box `x` whose elements carry the global
    indices `gidx` (same shape, increasing along C order / the axis):
    keepdims along `axis`, or shape (1,) for axis None."""
    if axis is None:
        x, gidx, axis = x.reshape(-1), gidx.reshape(-1), 0
    fn = np.argmax if kind == "max" else np.argmin
    if skipna and x.dtype.kind == "f":
        nan = np.isnan(x)
        fill = -np.inf if kind == "max" else np.inf
        pos = np.expand_dims(fn(np.where(nan, fill, x), axis=axis), axis)
        dead = np.all(nan, axis=axis, keepdims=True)
    else:
        pos = np.expand_dims(fn(x, axis=axis), axis)
        dead = None
    vals = np.take_along_axis(x, pos, axis)
    idxs = np.take_along_axis(gidx, pos, axis).astype(np.int64)
    if dead is not None:
        # the fill ties with a genuine -inf (+inf) standing after a NaN: a
        # NaN is ignored, so such a line's answer is its first real
        # infinity, as in the kernels
        fix = np.take_along_axis(nan, pos, axis) & ~dead
        if np.any(fix):
            first = np.expand_dims(np.argmax(x == fill, axis=axis), axis)
            pos = np.where(fix, first, pos)
            vals = np.take_along_axis(x, pos, axis)
            idxs = np.take_along_axis(gidx, pos, axis).astype(np.int64)
        idxs = np.where(dead, np.int64(-1), idxs)
    return np.ascontiguousarray(vals), np.ascontiguousarray(idxs)


class HostArg:
    """Portable host implementation of the arg-reduction hooks."""

    def __init__(self, backend):
        self.backend = backend

    def arg_reduce_partial(self, bd, rt, view, lb, axis, mult, idx0, kind,
                           skipna):
        import torch
        core = rt.core_box(bd, rt.rank)
        local = self.backend.box_to_numpy(bd, rt, core)
        # the operand is read in place through the view's strides
        off0, strides = view.operand_addressing(
            lb[0], c_strides(local.shape), core[0], (0,) * local.ndim)
        shape = box_shape(lb)
        flat = local.reshape(-1)
        x = np.lib.stride_tricks.as_strided(
            flat[off0:] if off0 else flat, shape=shape,
            strides=tuple(s * local.itemsize for s in strides))
        gidx = np.full(shape, idx0, dtype=np.int64)
        for d, m in enumerate(mult):
            if m:
                sh = [1] * len(shape)
                sh[d] = shape[d]
                gidx = gidx + (np.arange(shape[d], dtype=np.int64)
                               * m).reshape(sh)
        vals, idxs = local_pairs(x, gidx, axis, kind, skipna)
        if axis is None:
            vals, idxs = vals.reshape(1), idxs.reshape(1)
        return torch.from_numpy(vals), torch.from_numpy(idxs)

    def arg_combine_box(self, out_bd, rt, box, best, rel, src_vals, src_idx,
                        kind, skipna):
        core = rt.core_box(out_bd, rt.rank)
        cur = self.backend.box_to_numpy(out_bd, rt, core).copy()
        sl_i = box_slices(box, core[0])
        bv = best.numpy()[box_slices(rel)]   # shares memory with `best`
        sv = src_vals.numpy().reshape(bv.shape)
        si = src_idx.numpy().reshape(bv.shape)
        take = better(sv, si, bv, cur[sl_i], kind, skipna)
        bv[take] = sv[take]
        cur[sl_i][take] = si[take]
        self.backend.write_core_from_numpy(out_bd, rt, cur)
