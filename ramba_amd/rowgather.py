"""Indexed row gather: shared owner bucketing and the portable host hooks.

`runtime.take_op` moves rows through three backend hooks:

    take_index(idx_bd, rt)                 -> the rank's slice of the 1-D
                                              int64 index, a torch tensor
    gather_rows(src_bd, rt, rows, out=None, positions=None)
                                           -> dense (n,)+row_shape tensor of
                                              the selected LOCAL rows; with
                                              `out`, written into that
                                              array's core at positions[k]
                                              (rows 0..n-1 when None)
    place_rows(out_bd, rt, positions, dense)
                                           -> out[positions[k]] = dense[k]

`HipBackend` implements them on the rt_take_rows kernel.  A backend without
them (the NumPy oracle backend, which is frozen test infrastructure) gets
`HostTake`: the same hooks built only on calls every backend has
(box_to_numpy / write_core_from_numpy).  It works for host-memory backends
whose message buffers wrap NumPy arrays, and is strict where the kernel
counts: an out-of-range row raises at once.

Replaces the per-element index lists of the reference's all2all getitem
worker (ramba/ramba.py:3960) with whole-row requests.
"""

import numpy as np


def hooks_for(backend):
    """The object serving the three hooks for `backend`."""
    if hasattr(backend, "gather_rows"):
        return backend
    return HostTake(backend)


def bucket_rows(rows, starts, ranks, nrows, world):
    """Classify this rank's index entries by the rank owning the source row.

    rows   : 1-D int64 torch tensor (any device), negatives allowed
    starts : ascending axis-0 starts of the non-empty source shards
    ranks  : the rank owning each of those shards
    Returns (pos, lrows): per owner s, the positions of its entries in the
    local output (index order) and their row numbers local to s.
    """
    import torch
    rows = torch.where(rows < 0, rows + nrows, rows)
    bounds = torch.tensor(starts, dtype=torch.int64, device=rows.device)
    slot = torch.bucketize(rows, bounds, right=True) - 1
    pos = [rows.new_empty(0) for _ in range(world)]
    lrows = [rows.new_empty(0) for _ in range(world)]
    for j, s in enumerate(ranks):
        p = torch.nonzero(slot == j).reshape(-1)
        pos[s] = p
        lrows[s] = rows[p] - int(starts[j])
    return pos, lrows


class HostTake:
    """Portable host implementation of the take hooks (see module doc)."""

    def __init__(self, backend):
        self.backend = backend

    @staticmethod
    def _core(bd, rt):
        return rt.core_box(bd, rt.rank)

    def take_index(self, idx_bd, rt):
        import torch
        core = self._core(idx_bd, rt)
        if core is None:
            return torch.empty(0, dtype=torch.int64)
        return torch.from_numpy(np.ascontiguousarray(
            self.backend.box_to_numpy(idx_bd, rt, core), dtype=np.int64))

    @staticmethod
    def _checked(rows, nrows, wrap):
        rows = np.asarray(rows, dtype=np.int64)
        if wrap:
            rows = np.where(rows < 0, rows + nrows, rows)
        if rows.size and (rows.min() < 0 or rows.max() >= nrows):
            raise IndexError(f"take: row number out of range [0, {nrows})")
        return rows

    def gather_rows(self, src_bd, rt, rows, out=None, positions=None):
        import torch
        core = self._core(src_bd, rt)
        local = self.backend.box_to_numpy(src_bd, rt, core)
        sel = local[self._checked(rows.numpy(), local.shape[0], True)]
        if out is None:
            return torch.from_numpy(np.ascontiguousarray(sel))
        if positions is None:
            positions = torch.arange(sel.shape[0])
        self.place_rows(out, rt, positions, torch.from_numpy(sel))
        return None

    def place_rows(self, out_bd, rt, positions, dense):
        core = self._core(out_bd, rt)
        local = self.backend.box_to_numpy(out_bd, rt, core).copy()
        pos = self._checked(positions.numpy(), local.shape[0], False)
        local[pos] = dense.numpy().reshape((pos.size,) + local.shape[1:])
        self.backend.write_core_from_numpy(out_bd, rt, local)
