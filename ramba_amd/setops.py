"""unique / searchsorted: the backend hooks, and the portable host version.

`runtime.unique_op` and `runtime.searchsorted_op` work through two backend
hooks.  Keys travel as dense torch tensors of the array's dtype (bool as
uint8) on the backend's own device, positions and counts as int64:

    unique_run(keys, pos, want_first, want_counts) -> (ukeys, first, counts)
        `keys` is one dense SORTED run (what the sort hooks of
        ramba_amd/sorting.py leave), `pos` the int64 payloads that travelled
        with it or None.  ukeys: the first key of every run of equal keys,
        its raw bits; first: that key's payload; counts: the run lengths.
        Results not asked for are None.
    search_core(v, bd, rt, out_bd, side)
        `v` is the whole sorted key array, dense and the same on every rank;
        every element of the rank's core of the constructed array `bd`
        (same dtype) is searched in it and the int64 result lands in the core
        of `out_bd` (same shape and divisions).  side: "left" or "right".

Equality and order are those of include/ramba_sortkey.h: -0.0 == +0.0, every
NaN equals every NaN and sorts last, which is what NumPy's unique
(equal_nan=True) and searchsorted do.  `HipBackend` implements the hooks on
the rt_unique_* and rt_searchsorted kernels.  A backend without them (the
NumPy oracle backend, which is frozen test infrastructure) gets `HostUnique`,
built only on box_to_numpy / write_core_from_numpy and NumPy.  The reference
has neither operation.
"""

import numpy as np


def hooks_for(backend):
    """The object serving the hooks for `backend`."""
    if hasattr(backend, "unique_run"):
        return backend
    return HostUnique(backend)


class HostUnique:
    """Portable host implementation of the unique / searchsorted hooks."""

    def __init__(self, backend):
        self.backend = backend

    def unique_run(self, keys, pos, want_first, want_counts):
        import torch
        k = keys.numpy()
        n = k.shape[0]
        same = k[1:] == k[:-1]
        if k.dtype.kind == "f":
            same |= np.isnan(k[1:]) & np.isnan(k[:-1])
        heads = np.flatnonzero(np.concatenate([[True], ~same])[:n])
        first = counts = None
        if want_first:
            first = torch.from_numpy(
                heads.astype(np.int64) if pos is None else pos.numpy()[heads])
        if want_counts:
            counts = torch.from_numpy(
                np.diff(np.append(heads, n)).astype(np.int64))
        return torch.from_numpy(k[heads]), first, counts

    def search_core(self, v, bd, rt, out_bd, side):
        core = rt.core_box(bd, rt.rank)
        if core is None:
            return
        local = self.backend.box_to_numpy(bd, rt, core)
        keys = v.numpy()
        if local.dtype == np.bool_:
            keys = keys.astype(np.bool_)
        self.backend.write_core_from_numpy(
            out_bd, rt,
            np.searchsorted(keys, local, side=side).astype(np.int64))
