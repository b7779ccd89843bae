"""Ahead-of-time kernel compilation (cache seeding).

Runs representative in-scope programs against a compile-only backend:
every fused group is lowered and compiled by hiprtc for gfx950 (no GPU
needed) and the code object lands in the content-addressed on-disk cache
(`ramba_amd/_kcache`, see csrc kcache_*).  The cache ships with the repo
snapshot, so GPU boxes load kernels instead of invoking hiprtc — this is
the build-time half of the JIT cache (the analog of the reference's
persistent Numba cache, ramba/ramba.py:177-232).

No array data exists here: launches compile and return reduction
identities.  Programs must therefore not branch on computed values.
"""

import ctypes
import os

import numpy as np

from . import codegen, ir


class AotCompileBackend:
    """Compile-only backend: plans are lowered + hiprtc-compiled, nothing
    executes.  Product tooling (no oracle involvement)."""

    name = "aot"

    def __init__(self):
        from .hip_backend import LIBPATH
        kc = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "_kcache")
        os.environ.setdefault("RAMBA_KCACHE", kc)
        os.makedirs(os.environ["RAMBA_KCACHE"], exist_ok=True)
        self.lib = ctypes.CDLL(LIBPATH)
        self.lib.rt_compile_check.argtypes = [ctypes.c_char_p]
        self.lib.rt_last_error.restype = ctypes.c_char_p
        self.rt = None
        self.compiled = 0

    def attach(self, rt):
        self.rt = rt

    def _cc(self, source):
        rc = self.lib.rt_compile_check(source.encode())
        if rc != 0:
            raise RuntimeError("aot compile failed:\n"
                               + self.lib.rt_last_error().decode())
        self.compiled += 1

    # -- memory: bookkeeping only -------------------------------------------

    def alloc_container(self, bd, rt):
        pass

    def free_container(self, bd):
        pass

    def alloc_temp(self, name, shape, dtype):
        pass

    def free_temps(self):
        pass

    def launch(self, plan, recipe=None):
        gk = codegen.generate(plan)
        self._cc(gk.source)
        if gk.finish_source:
            self._cc(gk.finish_source)
        # also precompile the LDS load-tiled stencil variant when the
        # plan qualifies (the HIP backend prefers it at runtime)
        if (not plan.reductions and len(plan.itershape) == 2
                and plan.itershape[0] * plan.itershape[1] >= (1 << 16)):
            fams = codegen.find_stencil_families(plan)
            if fams:
                self._cc(codegen.generate_load_tiled(plan, fams).source)
        return [ir.reduction_identity(s.kind, s.dtype)
                for s in plan.reductions]

    def axis_reduce_partial(self, bd, off0, strides, lb, axes, kind,
                            out_dtype):
        nd = lb.shape[1]
        gk = codegen.generate_axis_reduce(
            nd, tuple(sorted(axes)), bd.dtype, out_dtype, kind)
        self._cc(gk.source)
        if not gk.lane_split and len(axes) == 1:
            self._cc(codegen.generate_axis_reduce(
                nd, tuple(sorted(axes)), bd.dtype, out_dtype, kind,
                chunked=True).source)
            self._cc(codegen.generate_axis_reduce(
                2, (0,), out_dtype, out_dtype, kind).source)

    def fill_container(self, bd, rt, value):
        pass

    def pack_temp_box(self, vname, rel_box):
        return None

    def combine_box_into_container(self, bd, rt, box, buf, kind):
        pass

    def combine_temp_into_container(self, bd, rt, box, vname, rel_box,
                                    kind):
        pass

    def cumsum_local_phase12(self, bd, off0, stride, n, out_dtype):
        return np.asarray(0, dtype=out_dtype)[()]

    def cumsum_local_phase3(self, bd, off0, stride, n, out_bd, out_off,
                            offset, out_dtype):
        pass

    def allgather_scalars(self, val, dtype):
        return [val]

    def mask_compact(self, bd_a, bd_m, rt):
        return None, 0   # kernels live in libramba_rt.so (hipcc-built)

    def axis_scan_local(self, *a):
        pass

    def axcs_init_offsets(self, *a):
        pass

    def axcs_accumulate(self, *a):
        pass

    def axcs_apply(self, *a):
        pass

    def flat_gather(self, cont, off0, strides, shape, flat0, n):
        return None

    def flat_scatter(self, *a):
        pass

    def write_local_dense(self, out_bd, rt, local):
        pass

    def box_to_numpy(self, bd, rt, box):
        from .shardview import box_shape
        return np.zeros(box_shape(box), dtype=bd.dtype)

    def bcast_numpy(self, obj, root):
        return obj

    def allreduce(self, value, kind):
        return value

    def write_core_from_numpy(self, bd, rt, nparr):
        pass

    def sync(self):
        pass


def seed(fuzz_seeds=None):
    """Compile the kernels the bench/smoke programs need; optionally also
    every kernel the fuzz-parity sweep (tests/fuzz_programs.py) generates,
    so `pytest -m gpu` on a box loads code objects instead of invoking
    hiprtc (`RAMBA_AOT_FUZZ` seeds, default 240; 0 disables)."""
    import ramba_amd as ra
    if ra._initialized["done"]:
        ra.shutdown()
    be = AotCompileBackend()
    ra.init(backend=be)

    # smoke set + configs[1]/[2] (fp64 chain + fused reduction)
    A = ra.arange(1 << 16) / 1000.0
    B = ra.sin(A)
    C = ra.cos(A)
    D = B * B + C ** 2
    D.sum()
    ra.sync()
    # configs[3] stencil fp32 + smoke's f32 iota
    X = ra.fromfunction(lambda x, y: x + y, (128, 130), dtype=np.float32)
    Y = ra.zeros((128, 130), dtype=np.float32)
    Y[1:-1, 1:-1] = (X[:-2, 1:-1] + X[2:, 1:-1] + X[1:-1, :-2]
                     + X[1:-1, 2:] - 4.0 * X[1:-1, 1:-1])
    ra.sync()
    # configs[3] at the bench geometries so the adaptive LDS stencil
    # kernels land in the cache (tile geometry keys on the iteration
    # shape class; no data is allocated on the aot backend)
    for SS in (512, 4096, 30000):
        X2 = ra.fromfunction(lambda x, y: x + y, (SS, SS),
                             dtype=np.float32)
        Y2 = ra.zeros((SS, SS), dtype=np.float32)
        ra.sync()
        Y2[1:-1, 1:-1] = (X2[:-2, 1:-1] + X2[2:, 1:-1] + X2[1:-1, :-2]
                          + X2[1:-1, 2:] - 4.0 * X2[1:-1, 1:-1])
        ra.sync()
        del X2, Y2
        ra.sync()
    # configs[4] mixed fp64 (Z materialised first so the pair takes the
    # staged/tiled path, like the bench loop's steady state)
    Z = ra.zeros((64, 64), dtype=np.float64)
    ra.sync()
    src = ra.fromfunction(lambda x, y: (x * 64 + y) * 1e-6, (64, 64),
                          dtype=np.float64)
    ss = ra.sin(src)
    Z[1:-1, 1:-1] = (ss[:-2, 1:-1] + ss[2:, 1:-1] + ss[1:-1, :-2]
                     + ss[1:-1, 2:] - 4.0 * ss[1:-1, 1:-1])
    Z.sum()
    ra.sync()
    del A, B, C, D, X, Y, Z, src, ss
    ra.sync()
    # configs[1] exactly as bench.py runs it, at the bench size (nothing is
    # allocated here): A is materialised by its own flush, so the step
    # kernel either recomputes it from the index (common.remat, A is far
    # above remat_min_bytes) or reads it — seed both
    from . import common
    saved = common.remat
    try:
        for on in (1, 0):
            common.remat = on
            A = ra.arange(1_000_000_000) / 1000.0
            ra.sync()
            B = ra.sin(A)
            C = ra.cos(A)
            D = B * B + C ** 2
            ra.sync()      # B, C, D still referenced: live, like the bench
            del A, B, C, D
            ra.sync()
    finally:
        common.remat = saved
    if fuzz_seeds is None:
        fuzz_seeds = int(os.environ.get("RAMBA_AOT_FUZZ", "240"))
    if fuzz_seeds:
        import sys
        sys.path.insert(0, os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
            "tests"))
        from fuzz_programs import build_program
        from fuzz_staged import build_staged_program
        with np.errstate(all="ignore"):
            for sd in range(fuzz_seeds):
                impl, _ = build_program(sd, mode="numpy")
                impl(ra)
                impl, _ = build_program(sd, mode="oracle")
                impl(ra)
            # staged-fusion fuzz kernels (tiled producer/consumer pairs)
            for sd in range(min(fuzz_seeds, 200)):
                build_staged_program(sd)(ra)
    n = be.compiled
    ra.shutdown()
    return n


# -- cross-stage fusion: compile-only hooks (ramba_amd/staged.py) ------------

AotCompileBackend.supports_staged = True


def _aot_container_addr(self, bd):
    return 0


def _aot_tiled_kernel(self, desc):
    gk = codegen.generate_staged_tiled(desc)
    self._cc(gk.source)
    return gk


def _aot_tiled_launch(self, handle, vals, ntiles, red_dtypes=None,
                      rec=None):
    return [np.asarray(0, dtype=dt)[()] for dt in (red_dtypes or [])]


AotCompileBackend.container_addr = _aot_container_addr
AotCompileBackend.tiled_kernel = _aot_tiled_kernel
AotCompileBackend.tiled_launch = _aot_tiled_launch
