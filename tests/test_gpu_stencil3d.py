"""GPU: 3-D stencil updates on the plane-marching LDS kernel (kind 'lt3').

Each case runs with RAMBA_LT3_MIN=0, RAMBA_LT3_SEG=4 and RAMBA_LT3_NCH=64, so
its small shape spans several plane segments with a short last one, the ring
wraps, and the strip is 256 (4-byte) or 128 (8-byte) outputs wide.  The input
is not affine in the index (a symmetric stencil of an affine field hides a
swapped neighbour), the weights are distinct multiples of 0.5 and every
partial sum is exact in float32, so the checks need no tolerance:

(a) the result equals plain NumPy evaluated in float64 and cast back;
(b) it equals the result under RAMBA_STENCIL_LDS=0, bit for bit;
(c) the LDS run compiled an ("lt3", key) kernel and the =0 run did not.
"""

import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAR1 = [(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0),
         (1, 1, 2)]
STAR2 = [(2, 2, 2)] + [tuple(2 + s * r * (a == d) for a in range(3))
                       for d in range(3) for r in (1, 2) for s in (-1, 1)]
BOX = list(itertools.product(range(3), repeat=3))
UPWIND = [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3), (3, 1, 2)]

# id: (dtype, interior shape, read offsets, offset of the written box,
#      extra operands in the statement, crop of larger arrays, steps)
CASES = {
    "f32-7pt": ("float32", (11, 19, 261), STAR1, (1, 1, 1), False, None, 1),
    "f64-star2": ("float64", (9, 18, 136), STAR2, (2, 2, 2), False, None, 1),
    "f32-box27": ("float32", (6, 17, 70), BOX, (1, 1, 1), False, None, 1),
    "f64-upwind": ("float64", (10, 9, 131), UPWIND, (0, 0, 0), False, None,
                   1),
    "f32-7pt-extras": ("float32", (7, 20, 260), STAR1, (1, 1, 1), True, None,
                       1),
    "i32-7pt": ("int32", (5, 16, 259), STAR1, (1, 1, 1), False, None, 1),
    "f64-7pt-subbox": ("float64", (8, 10, 129), STAR1, (1, 1, 1), False,
                       ((2, 3), (1, 2), (3, 1)), 1),
    "f32-7pt-pingpong": ("float32", (11, 19, 261), STAR1, (1, 1, 1), False,
                         None, 2),
}


def program(np_, dtype, n, offs, dst, extras, crop, steps, wstep):
    dt = np.dtype(dtype)
    ext = tuple(max(o[d] for o in offs) for d in range(3))
    crop = crop or ((0, 0),) * 3
    full = tuple(n[d] + ext[d] + sum(crop[d]) for d in range(3))
    inner = tuple(slice(lo, s - hi) for (lo, hi), s in zip(crop, full))

    def box(off):
        return tuple(slice(o, o + m) for o, m in zip(off, n))

    def sync():
        if np_ is not np:
            np_.sync()

    A0 = np_.fromfunction(
        lambda x, y, z: (x * x * 3 + y * y * 5 + z * z * 7 + x * y * z) % 61,
        full, dtype=dt)
    B0 = np_.zeros(full, dtype=dt)
    W = np_.fromfunction(lambda x, y, z: (x * 7 + y * y + z * 3) % 13,
                         full, dtype=dt)
    sync()
    A, B = A0[inner], B0[inner]
    for _ in range(steps):
        # weights wstep, 2 * wstep, ...: 0.5 apart (1 for integers)
        acc = None
        for k, off in enumerate(offs):
            w = wstep * (k + 1)
            acc = w * A[box(off)] if acc is None else acc + w * A[box(off)]
        if extras:
            acc = acc + 2.0 * W[inner][box(dst)] + 1.5 + np_.fromfunction(
                lambda x, y, z: x * 4 + y * 2 + z, n, dtype=dt)
        B[box(dst)] = acc
        sync()
        if steps > 1:
            A[box(dst)] = 0.5 * B[box(dst)]
            sync()
    out = B0 if np_ is np else B0.asarray()
    return out if steps == 1 else (out, A0 if np_ is np else A0.asarray())


@pytest.mark.parametrize("case", list(CASES))
def test_lt3_equals_numpy_and_the_vectorized_route(ra_gpu, monkeypatch, case):
    from ramba_amd import deferred
    dtype, n, offs, dst, extras, crop, steps = CASES[case]
    rt = deferred.get_runtime()
    be = rt.backend
    wstep = 1 if dtype == "int32" else 0.5
    monkeypatch.setenv("RAMBA_LT3_MIN", "0")
    monkeypatch.setenv("RAMBA_LT3_SEG", "4")
    monkeypatch.setenv("RAMBA_LT3_NCH", "64")
    got = {}
    for lds in ("1", "0"):
        monkeypatch.setenv("RAMBA_STENCIL_LDS", lds)
        # kernels are kept per structure: set both caches aside
        rt.__dict__.pop("_recipe_cache", None)
        for k in [k for k in be.kernels if k[0] == "lt3"]:
            del be.kernels[k]
        got[lds] = np.stack(program(ra_gpu, *CASES[case], wstep))
        assert any(k[0] == "lt3" for k in be.kernels) == (lds == "1")
    rt.__dict__.pop("_recipe_cache", None)
    ref = {w: np.stack(program(np, w, n, offs, dst, extras, crop, steps,
                                 wstep))
           for w in (dtype, "float64")}
    assert np.array_equal(ref[dtype], ref["float64"]), "case is not exact"
    assert got["1"].dtype == np.dtype(dtype)
    assert np.array_equal(got["1"], ref["float64"].astype(dtype))
    assert np.array_equal(got["1"], got["0"])
