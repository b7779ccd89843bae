"""Host: the 3-D stencil family finder and the 'lt3' generator, no GPU.

The programs of tests/test_gpu_stencil3d.py run on the compile-only backend:
a qualifying update compiles two kernels for gfx950, the generic one and the
plane-marching one.  Four near misses must not qualify.
"""

import numpy as np
import pytest

from ramba_amd import aot, codegen

from test_gpu_stencil3d import CASES, program


class LoggingBackend(aot.AotCompileBackend):
    """Compile-only backend that keeps (plan, kernels compiled for it)."""

    def __init__(self):
        super().__init__()
        self.log = []

    def launch(self, plan, recipe=None):
        c0 = self.compiled
        out = super().launch(plan, recipe)
        self.log.append((plan, self.compiled - c0))
        return out


@pytest.fixture
def logged(monkeypatch):
    """(ramba_amd, backend): the logging backend swapped into the live
    runtime, with the runtime's recipe caches set aside meanwhile."""
    import ramba_amd as ra
    from ramba_amd import deferred
    from oracle.numpy_backend import NumpyBackend
    if not ra._initialized["done"]:
        ra.init(backend=NumpyBackend())
    deferred.flush()
    rt = deferred.get_runtime()
    old = rt.backend
    caches = {k: rt.__dict__.pop(k) for k in ("_recipe_cache", "_staged_cache")
              if k in rt.__dict__}
    be = LoggingBackend()
    rt.backend = be
    be.attach(rt)
    monkeypatch.setenv("RAMBA_LT3_MIN", "0")
    monkeypatch.setenv("RAMBA_LT3_SEG", "4")
    yield ra, be
    deferred.flush()
    rt.backend = old
    for k in ("_recipe_cache", "_staged_cache"):
        rt.__dict__.pop(k, None)
    rt.__dict__.update(caches)


@pytest.mark.parametrize("case", ["f32-7pt", "f64-star2", "f32-box27",
                                  "i32-7pt"])
def test_generic_and_lt3_kernels_compile(logged, case):
    ra, be = logged
    program(ra, *CASES[case], 1 if case == "i32-7pt" else 0.5)
    (grown,) = [g for (p, g) in be.log if p.itershape == CASES[case][1]]
    assert grown == 2


def _two_readers(A):
    return A[:-2, 1:-1, 1:-1] + 2.0 * A[2:, 1:-1, 1:-1]


def _delta_nine(A):
    return A[:-9, 1:-1, 1:-1] + 2.0 * A[9:, 1:-1, 1:-1] \
        + 3.0 * A[:-9, 2:, 1:-1]


def _inner_stride_two(A):
    return A[1:-1, 1:-1, 0:-2:2] + 2.0 * A[:-2, 1:-1, 0:-2:2] \
        + 3.0 * A[2:, 1:-1, 0:-2:2]


def _reduction(A):
    return (A[1:-1, 1:-1, 1:-1] + 2.0 * A[:-2, 1:-1, 1:-1]
            + 3.0 * A[2:, 1:-1, 1:-1]).sum()


@pytest.mark.parametrize("expr", [_two_readers, _delta_nine,
                                  _inner_stride_two, _reduction])
def test_near_misses_do_not_qualify(logged, expr):
    ra, be = logged
    A = ra.fromfunction(lambda x, y, z: x * x + y * z, (12, 20, 70),
                        dtype=np.float64)
    ra.sync()
    be.log.clear()
    r = expr(A)
    r.asarray() if hasattr(r, "asarray") else float(r)
    ra.sync()
    plans = [p for (p, _) in be.log if len(p.itershape) == 3]
    assert plans and all(
        codegen.find_stencil_families_3d(p) is None for p in plans)
