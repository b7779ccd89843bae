"""GPU: index-pure rematerialisation (common.remat) on the HIP path.

Each case runs with the threshold at 0, compares remat on against remat off
with np.array_equal (same operations, same order: the bits must match) and
against NumPy at 1e-12 (1e-5 for float32), and asserts that a substitution
really happened.  The 1-D sizes cover the scalar-only kernel (n < vector
width), the vector loop with and without a tail, and more than one block.
The 2-D input is NOT affine in the index and the stencil weights are all
different, so a wrong offset, step, axis order or global start in the
composed recipe changes the result (a Laplacian of an affine input would be
zero whatever the recipe computes).
"""

import numpy as np
import pytest

from ramba_amd import common

pytestmark = pytest.mark.gpu

CHAIN_SIZES = (1, 2, 3, 511, 512, 513, 1027, (1 << 16) + 37)
SLICES = {"1:": slice(1, None), "::2": slice(None, None, 2),
          "::-1": slice(None, None, -1), "3:-5:3": slice(3, -5, 3)}
SLICED_N = 1027
SHAPE_2D = (67, 7)


def _sync(np_):
    if hasattr(np_, "sync"):
        np_.sync()


def chain(np_, n):
    A = np_.arange(n) / 1000.0
    _sync(np_)
    B = np_.sin(A)
    C = np_.cos(A)
    D = B * B + C ** 2
    return B, C, D


def sliced(np_, sl):
    A = np_.arange(SLICED_N) * 0.25 + 3.0
    _sync(np_)
    return (np_.sin(A[sl]) * 2.0 - A[sl],)


def shifted_2d(np_):
    # values are small integers and the weights multiples of 0.5: every
    # float32 operation is exact
    X = np_.fromfunction(lambda x, y: x * x + y * x, SHAPE_2D,
                         dtype=np.float32)
    _sync(np_)
    return (0.5 * X[:-2, 1:-1] + 2.0 * X[2:, 1:-1] + 3.0 * X[1:-1, :-2]
            - 1.5 * X[1:-1, 2:] - 4.0 * X[1:-1, 1:-1],
            X[::-1, ::2] - 2.0 * X[:, :4],
            X.T[1:, 3:] + 1.0)


PROGRAMS = [(f"chain-{n}", (lambda np_, n=n: chain(np_, n)))
            for n in CHAIN_SIZES]
PROGRAMS += [(f"sliced-{k}", (lambda np_, sl=sl: sliced(np_, sl)))
             for k, sl in SLICES.items()]
PROGRAMS.append(("shifted2d", shifted_2d))


@pytest.mark.parametrize("prog", [p for _, p in PROGRAMS],
                         ids=[i for i, _ in PROGRAMS])
def test_remat_on_off_numpy(ra_gpu, prog):
    saved = (common.remat, common.remat_min_bytes)
    try:
        common.remat_min_bytes = 0
        common.remat = 1
        c0 = common.remat_substitutions
        on = [x.asarray() for x in prog(ra_gpu)]
        assert common.remat_substitutions > c0, "no substitution happened"
        common.remat = 0
        c0 = common.remat_substitutions
        off = [x.asarray() for x in prog(ra_gpu)]
        assert common.remat_substitutions == c0
    finally:
        ra_gpu.sync()
        common.remat, common.remat_min_bytes = saved
    ref = [np.asarray(x) for x in prog(np)]
    for a, b, r in zip(on, off, ref):
        assert a.dtype == b.dtype == r.dtype and a.shape == b.shape == r.shape
        assert np.array_equal(a, b)
        # (sin(0) alone is the one legitimate all-zero reference)
        assert r.size == 1 or np.any(r != 0), "degenerate all-zero case"
        tol = 1e-5 if a.dtype == np.float32 else 1e-12
        np.testing.assert_allclose(a, r, rtol=tol, atol=tol)
