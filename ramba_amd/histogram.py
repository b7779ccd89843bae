"""histogram / bincount: the binning modes, and the portable host hook.

`runtime.hist_op` bins each rank's box through one backend hook:

    hist_partial(bd, rt, view, lb, mode, edges, nbins) -> (counts, bad)
        counts: the rank's partial counts over its view-space box `lb`, a
            torch int64 tensor of length nbins;
        bad: how many elements mode INDEX skipped (a 1-element tensor);
        mode: INDEX (the bin is the value), UNIFORM (`edges` are the
            nbins + 1 evenly spaced float32 / float64 edges NumPy computed)
            or EDGES (any non-decreasing float64 edges);
        edges: a host NumPy array, None in mode INDEX.

`HipBackend` implements it on the rt_hist kernel.  A backend without it (the
NumPy oracle backend, which is frozen test infrastructure) gets `HostHist`,
built only on box_to_numpy and NumPy.  In both modes with edges an element
lands in bin i iff edges[i] <= x < edges[i + 1] (the last bin closed), which
is what NumPy's own edge-array path computes; the kernel's UNIFORM mode
reaches the same bin through NumPy's index guess and its one-step
correction.  The reference has no histogram or bincount.

This module shares its name with the public function: once the package is
imported, `ramba_amd.histogram` is the function (ndarray.py), and this module
is reached with importlib.import_module("ramba_amd.histogram").
"""

import numpy as np

from .shardview import box_shape, c_strides

INDEX, UNIFORM, EDGES = 0, 1, 2


def hooks_for(backend):
    """The object serving the hook for `backend`."""
    if hasattr(backend, "hist_partial"):
        return backend
    return HostHist(backend)


class HostHist:
    """Portable host implementation of the histogram hook."""

    def __init__(self, backend):
        self.backend = backend

    def hist_partial(self, bd, rt, view, lb, mode, edges, nbins):
        import torch
        core = rt.core_box(bd, rt.rank)
        local = self.backend.box_to_numpy(bd, rt, core)
        # the operand is read in place through the view's strides
        off0, strides = view.operand_addressing(
            lb[0], c_strides(local.shape), core[0], (0,) * local.ndim)
        flat = local.reshape(-1)
        x = np.lib.stride_tricks.as_strided(
            flat[off0:] if off0 else flat, shape=box_shape(lb),
            strides=tuple(s * local.itemsize for s in strides)).reshape(-1)
        if x.dtype == np.bool_:
            x = x.view(np.uint8)
        if mode == INDEX:
            x = x.astype(np.int64)
            ok = (x >= 0) & (x < nbins)
            counts = np.bincount(x[ok], minlength=nbins)
            bad = int(x.size - np.count_nonzero(ok))
        else:
            counts = np.histogram(x, bins=edges)[0]
            bad = 0
        return (torch.from_numpy(counts.astype(np.int64)),
                torch.tensor([bad], dtype=torch.int32))
