"""sort / argsort over CPU ranks (gloo, worlds 2 and 4): the sample sort of
runtime.sort_op and the line sort on a repartitioned array, on the oracle
backend.  The shared worker compares int64 results with array_equal, so
values are sorted as int64 and float order is checked through argsort."""

import pytest

from test_argreduce_gloo import run_spmd

WORLDS = pytest.mark.parametrize("world", [2, 4])


@WORLDS
def test_sample_sort_1d(world):
    # ties across rank boundaries, all-equal keys (one rank gets everything),
    # sorted and reversed input, fewer elements than ranks, NaN-heavy floats
    run_spmd("""
        rng = np.random.default_rng(0)
        k = rng.integers(-5, 6, size=1001)
        f = k.astype(np.float64)
        f[rng.random(1001) < 0.4] = np.nan
        f[::11] = -0.0
        up = np.arange(1001)
        out = []
        for h in (k, np.full(1001, 7), up, up[::-1].copy(), k[:3], k[:1]):
            a = np_.array(h)
            out += [np_.sort(a, kind="stable"), np_.argsort(a, kind="stable"),
                    np_.argsort(a[::-1], kind="stable"),
                    np_.sort(a[5::3], kind="stable"),
                    np_.argsort(a[5::3], kind="stable")]
        for h in (f, f.astype(np.float32), k.astype(np.int8), k > 0):
            out += [np_.argsort(np_.array(h), kind="stable")]
        return out
    """, world=world)


@WORLDS
def test_lines_of_a_2d_grid(world):
    # (40, 44) at world 4 is a 2 x 2 grid: either sorted axis is split
    run_spmd("""
        rng = np.random.default_rng(1)
        g = rng.integers(-3, 4, size=(40, 44))
        a = np_.array(g)
        out = []
        for x in (a, a.T, a[::-1, 3:]):
            for axis in (0, 1, None):
                out += [np_.sort(x, axis=axis, kind="stable"),
                        np_.argsort(x, axis=axis, kind="stable")]
        return out
    """, world=world)
