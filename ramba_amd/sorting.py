"""sort / argsort: the backend hooks, and the portable host implementation.

`runtime.sort_op` orders data through four backend hooks.  Keys travel as
dense torch tensors of the array's dtype (bool as uint8) on the backend's
own device, payloads and positions as int64:

    sort_lines(bd, rt, out_bd, want_index)
        `bd` is a constructed 2-D array (nlines, len) on axis-0 divisions;
        every line of the rank's core is sorted into the core of `out_bd`
        (same divisions): the sorted keys, or with want_index the int64
        positions 0 .. len-1 (argsort along the line).
    local_run(bd, rt) -> keys
        the rank's core of a constructed 1-D array (empty when it has none).
    sort_run(keys, vals, val0, want_keys, want_vals) -> (keys, vals)
        a stable sort of one dense run; the payload of key i is vals[i], or
        val0 + i when vals is None.  Results not asked for are None.
    sort_bounds(run, splitters) -> int64 NumPy array
        for each splitter (a NumPy array of the keys' dtype) the number of
        keys of the sorted `run` that sort strictly before it.
    split_run(keys, vals, val0, pivots, want_keys, want_vals,
              want_counts=True) -> (keys, vals, counts)
        the stable split of one dense run behind partition / argpartition:
        `pivots` are at most NPIV_MAX distinct ascending canonical keys
        (Python ints), the bucket of a key k is 2 * (pivots < canon(k)) +
        (canon(k) is a pivot), and the result is the buckets in ascending
        order, each in input order.  Payloads as in sort_run; counts is the
        int64 NumPy array of the 2 * len(pivots) + 1 bucket sizes, which a
        hook may leave out (None) when want_counts is false.

The order is NumPy's stable sort order (include/ramba_sortkey.h): floats
with -0.0 == +0.0 and every NaN equal and last, ties by position.
`HipBackend` implements the hooks on the rt_sort kernels.  A backend without
them (the NumPy oracle backend, which is frozen test infrastructure) gets
`HostSort`, built only on box_to_numpy / write_core_from_numpy and
np.argsort(kind="stable").  The reference has no sort.
"""

import numpy as np

NPIV_MAX = 8        # pivots per split (PART_NPIV_MAX = SELECT_NQ_MAX)


def hooks_for(backend):
    """The object serving the hooks for `backend`."""
    if hasattr(backend, "sort_lines"):
        return backend
    return HostSort(backend)


def _keys(a):
    return a.view(np.uint8) if a.dtype == np.bool_ else a


def splitter_bounds(run, splitters):
    """Host statement of sort_bounds: searchsorted(side="left") in NumPy's
    sort order (np.searchsorted compares as np.sort does, NaN last)."""
    return np.searchsorted(run, splitters, side="left").astype(np.int64)


class HostSort:
    """Portable host implementation of the sort hooks."""

    def __init__(self, backend):
        self.backend = backend

    def sort_lines(self, bd, rt, out_bd, want_index):
        core = rt.core_box(bd, rt.rank)
        if core is None:
            return
        local = _keys(self.backend.box_to_numpy(bd, rt, core))
        order = np.argsort(local, axis=1, kind="stable")
        res = order.astype(np.int64) if want_index else \
            np.take_along_axis(local, order, axis=1)
        self.backend.write_core_from_numpy(out_bd, rt, res)

    def local_run(self, bd, rt):
        import torch
        core = rt.core_box(bd, rt.rank)
        if core is None:
            return torch.from_numpy(
                np.empty(0, dtype=_keys(np.empty(0, bd.dtype)).dtype))
        return torch.from_numpy(np.ascontiguousarray(
            _keys(self.backend.box_to_numpy(bd, rt, core))))

    def sort_run(self, keys, vals, val0, want_keys, want_vals):
        import torch
        k = keys.numpy()
        order = np.argsort(k, kind="stable")
        out_k = torch.from_numpy(k[order]) if want_keys else None
        out_v = None
        if want_vals:
            out_v = torch.from_numpy(
                (order + np.int64(val0)) if vals is None
                else vals.numpy()[order])
        return out_k, out_v

    def sort_bounds(self, run, splitters):
        return splitter_bounds(run.numpy(), splitters)

    def split_run(self, keys, vals, val0, pivots, want_keys, want_vals,
                  want_counts=True):
        import torch
        from .selection import canon
        k = keys.numpy()
        c = canon(k)
        piv = np.array(pivots, dtype=c.dtype)
        bucket = 2 * np.searchsorted(piv, c, side="left") + np.isin(c, piv)
        order = np.argsort(bucket, kind="stable")
        out_k = torch.from_numpy(k[order]) if want_keys else None
        out_v = None
        if want_vals:
            out_v = torch.from_numpy(
                (order + np.int64(val0)) if vals is None
                else vals.numpy()[order])
        counts = np.bincount(bucket, minlength=2 * len(pivots) + 1)
        return out_k, out_v, counts.astype(np.int64)
