"""histogram / bincount over CPU ranks (gloo, worlds 2 and 4): the exchange
of runtime.hist_op on the oracle backend.  Counts equal NumPy's (the edges
are NumPy's own and are checked in test_hist_frontend.py)."""

import pytest

from test_argreduce_gloo import run_spmd

WORLDS = pytest.mark.parametrize("world", [2, 4])


@WORLDS
def test_uneven_divisions_and_views(world):
    # 1001 elements do not divide evenly; a short view leaves ranks without
    # a box, and so does a 3-element array at world 4
    run_spmd("""
        rng = np.random.default_rng(0)
        h = rng.normal(size=1001)
        k = rng.integers(0, 300, size=1001)
        a, b = np_.array(h), np_.array(k)
        out = []
        for x in (a, a[::-1], a[5::3], a[:7], np_.array(h[:3])):
            out += [np_.histogram(x, bins=13, range=(-2, 2))[0],
                    np_.histogram(x, bins=[-3, -1, -1, 0.5, 4])[0],
                    np_.histogram(x)[0]]
        for x in (b, b[::-2], b[990:], np_.array(k[:3])):
            out += [np_.bincount(x), np_.bincount(x, minlength=400)]
        return out
    """, world=world)


@WORLDS
def test_2d_split_on_both_axes_and_fewer_bins_than_ranks(world):
    # (40, 44) at world 4 is a 2 x 2 grid; 1..3 bins leave ranks that own no
    # result element
    run_spmd("""
        rng = np.random.default_rng(1)
        g = rng.integers(0, 3, size=(40, 44))
        a = np_.array(g.astype(np.float32))
        out = []
        for x in (a, a.T, a[::-1, 3:]):
            for bins in (1, 2, 3, 50):
                out += [np_.histogram(x, bins=bins)[0]]
        out += [np_.bincount(np_.array(g.reshape(-1))),
                np_.bincount(np_.array(np.zeros(1001, dtype=np.int8)))]
        return out
    """, world=world)
