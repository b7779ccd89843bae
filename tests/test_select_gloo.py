"""median / percentile over CPU ranks (gloo, worlds 2 and 4): the pass
protocol of runtime.select_op on the oracle backend.  The shared worker
compares int64 results with array_equal, so every result travels as the bits
of its float64 value."""

import pytest

from test_argreduce_gloo import run_spmd

WORLDS = pytest.mark.parametrize("world", [2, 4])

BITS = """
        def bits(x):
            return np.asarray(x, dtype=np.float64).reshape(-1).view(np.int64)
        def stats():
            return ra.deferred.get_runtime().last_select if np_ is ra else None
"""


@WORLDS
def test_uneven_boxes_views_and_ranks_without_a_box(world):
    # 1001 elements do not divide evenly; a short view and a 3-element array
    # leave ranks with nothing; (40, 44) at world 4 is a 2 x 2 grid
    run_spmd(BITS + """
        rng = np.random.default_rng(0)
        h = rng.normal(size=1001)
        g = rng.integers(-9, 9, size=(40, 44)).astype(np.int8)
        a, b = np_.array(h), np_.array(g)
        out = []
        for x in (a, a[::-1], a[5::3], a[:7], np_.array(h[:3]), b, b.T,
                  b[::-1, 3:], np_.array(h.astype(np.float32))):
            out += [bits(np_.median(x)), bits(np_.percentile(x, [1, 50, 99])),
                    bits(np_.quantile(x, 0.3, method="nearest"))]
        return out
    """, world=world)


@WORLDS
def test_collecting_and_not_and_a_locally_empty_bin(world):
    # sorted input: the median's bins are empty on every rank but one.  The
    # spread keys narrow below n / 8 and collect; equal keys never do
    run_spmd(BITS + """
        spread = np_.array(np.arange(4001, dtype=np.int64) << 20)
        out = [bits(np_.median(spread))]
        assert stats() is None or stats()["collected"], stats()
        out += [bits(np_.median(np_.array(np.full(4001, 7.5))))]
        assert stats() is None or not stats()["collected"], stats()
        return out + [bits(np_.percentile(spread, [0, 12.5, 100]))]
    """, world=world)


@WORLDS
def test_nans_are_counted_across_ranks(world):
    run_spmd(BITS + """
        h = np.arange(1001, dtype=np.float64) % 13
        h[[3, 999]] = np.nan            # first and last rank
        a = np_.array(h)
        return [bits(np_.median(a)), bits(np_.nanmedian(a)),
                bits(np_.nanpercentile(a, [0, 50, 100])),
                bits(np_.percentile(a, 50)), bits(np_.nanmedian(a[:500]))]
    """, world=world)
