"""Dense float matmul: the backend hooks and their portable host version.

`runtime.matmul_op` multiplies through two backend hooks:

    gemm_panel(b_bd, rt)          -> the rank's core of B (its K rows) as a
                                     dense 2-D buffer `exchange` can send;
                                     shape (0, N) when the rank owns no rows
                                     (at world 1, where nothing is sent, it
                                     may be a strided view of the shard)
    gemm_local(c_bd, rt, a_bd, k0, k1, panel, accumulate)
                                  -> core(C) (+)= core(A)[:, k0:k1] @ panel

The 1-D and batched forms (`runtime.matvec_op`, `vecmat_op`, `bmm_op`) use

    gemv_vector(x_bd, rt)         -> the rank's piece of a 1-D array as a
                                     dense buffer (length 0 without one)
    gemv_local(y_bd, rt, a_bd, x) -> core(y) = core(A) @ x, x all of K
    gemv_t_local(a_bd, rt, x_bd)  -> core(x) @ core(A): a dense length-N
                                     buffer, None when the rank has no rows
    bgemm_local(c_bd, rt, a_bd, b_bd)
                                  -> core(C)[i] = core(A)[i] @ core(B)[i]

`HipBackend` implements them on the rt_gemm MFMA kernel (rt_gemm_batched for
the batch) and the rt_gemv kernels, straight on the shard containers.  A backend without them (the NumPy oracle backend, which
is frozen test infrastructure) gets `HostGemm`: the same hooks built only
on calls every backend has (box_to_numpy / write_core_from_numpy) and NumPy
matmul.  It works for host-memory backends whose message buffers wrap NumPy
arrays.

Replaces the np.dot of the reference's matmul workers (ramba/ramba.py:3056,
:6953-7040).
"""

import numpy as np


def hooks_for(backend):
    """The object serving the two hooks for `backend`."""
    if hasattr(backend, "gemm_local"):
        return backend
    return HostGemm(backend)


class HostGemm:
    """Portable host implementation of the GEMM hooks (see module doc)."""

    def __init__(self, backend):
        self.backend = backend

    def _local(self, bd, rt):
        core = rt.core_box(bd, rt.rank)
        if core is None:
            return None
        return self.backend.box_to_numpy(bd, rt, core)

    def gemm_panel(self, b_bd, rt):
        import torch
        local = self._local(b_bd, rt)
        if local is None:
            local = np.empty((0, b_bd.shape[1]), dtype=b_bd.dtype)
        return torch.from_numpy(np.ascontiguousarray(local))

    def gemm_local(self, c_bd, rt, a_bd, k0, k1, panel, accumulate):
        a = self._local(a_bd, rt)
        if a is None:
            return
        prod = np.matmul(a[:, k0:k1], panel.numpy())
        if accumulate:
            prod = self._local(c_bd, rt) + prod
        self.backend.write_core_from_numpy(c_bd, rt,
                                           prod.astype(c_bd.dtype, copy=False))

    def gemv_vector(self, x_bd, rt):
        import torch
        local = self._local(x_bd, rt)
        if local is None:
            local = np.empty((0,), dtype=x_bd.dtype)
        return torch.from_numpy(np.ascontiguousarray(local))

    def gemv_local(self, y_bd, rt, a_bd, x):
        a = self._local(a_bd, rt)
        if a is not None:
            self.backend.write_core_from_numpy(
                y_bd, rt, np.matmul(a, x.numpy()).astype(y_bd.dtype,
                                                         copy=False))

    def gemv_t_local(self, a_bd, rt, x_bd):
        import torch
        a = self._local(a_bd, rt)
        if a is None:
            return None
        return torch.from_numpy(np.ascontiguousarray(
            np.matmul(self._local(x_bd, rt), a)))

    def bgemm_local(self, c_bd, rt, a_bd, b_bd):
        a = self._local(a_bd, rt)
        if a is not None:
            self.backend.write_core_from_numpy(
                c_bd, rt, np.matmul(a, self._local(b_bd, rt)).astype(
                    c_bd.dtype, copy=False))
