"""partition / argpartition over CPU ranks (gloo, worlds 2 and 4): the
select, split and exchange of runtime.partition_op on the oracle backend,
against the stable split restated in NumPy.  The shared worker compares int64
results with array_equal, so values travel as int64 and float order is
checked through argpartition."""

import pytest

from test_argreduce_gloo import run_spmd

WORLDS = pytest.mark.parametrize("world", [2, 4])


@WORLDS
def test_split_and_exchange(world):
    # ties across rank boundaries; sorted input, whose every rank falls into
    # one bucket; all-equal keys; fewer elements than ranks; NaN-heavy floats
    # with kth 700 and -1 past the numbers, so that the pivot is the NaN key
    run_spmd("""
        import sys
        sys.path.insert(0, os.path.join(sys.path[0], "tests"))
        from test_partition_frontend import expected_argpartition

        def arg(h, kth):
            if np_ is np:
                return expected_argpartition(h, kth)
            return np_.argpartition(np_.array(h), kth)

        def val(h, kth):
            if np_ is np:
                return h[expected_argpartition(h, kth)]
            return np_.partition(np_.array(h), kth)

        rng = np.random.default_rng(0)
        k = rng.integers(-5, 6, size=1001)
        f = k.astype(np.float64)
        f[rng.random(1001) < 0.4] = np.nan
        f[::11] = -0.0
        out = []
        for h in (k, np.arange(1001), np.full(1001, 7), k[:3], k[:1]):
            for kth in (0, h.size // 2, -1, [0, h.size // 3, -1]):
                out += [arg(h, kth), val(h, kth)]
        for h in (f, f.astype(np.float32), k.astype(np.int8), k > 0):
            for kth in (500, 700, [100, 500, -1]):
                out += [arg(h, kth)]
        out += [arg(k[5::3].copy(), 17)]
        return out
    """, world=world)
