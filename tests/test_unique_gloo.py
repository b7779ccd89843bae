"""unique / searchsorted over CPU ranks (gloo, worlds 2 and 3) on the oracle
backend: the exchange-free compaction after the sample sort, and the
replicated keys of searchsorted.  The shared worker compares int64 results
with array_equal, so values are int64 and float data is checked through its
index, inverse and counts."""

import pytest

from test_argreduce_gloo import run_spmd

WORLDS = pytest.mark.parametrize("world", [2, 3])


@WORLDS
def test_unique_runs_across_cuts_empty_ranks_and_distinct(world):
    # k: runs that cross the input's rank cuts; two values: a rank is left
    # empty; a permutation: all distinct; floats with NaN and signed zeros
    run_spmd("""
        k = np.arange(1001) // 97 * 3 - 7
        f = (k[::-1] % 5).astype(np.float64)
        f[::4] = np.nan
        f[1::7] = -0.0
        perm = np.arange(1001) * 7 % 1001
        out = []
        for h in (k, k[::-1].copy(), np.arange(1001) % 2 * 5, perm, k[:2]):
            a = np_.array(h)
            res = np_.unique(a, return_index=True, return_inverse=True,
                             return_counts=True)
            out += list(res) + [np_.unique(a[3::2])]
            if np_ is not np:       # the results' divisions sum to U
                bd = res[0].bdarray
                ext = bd.divisions[:, 1, 0] - bd.divisions[:, 0, 0] + 1
                assert ext.clip(0).sum() == bd.shape[0] == res[3].shape[0]
        out += list(np_.unique(np_.array(f), return_index=True,
                               return_inverse=True, return_counts=True)[1:])
        return out
    """, world=world)


@WORLDS
def test_searchsorted_with_distributed_needles(world):
    run_spmd("""
        v = np.arange(700) // 3 * 2 - 100
        x = (np.arange(41 * 23) * 13 % 600 - 150).reshape(41, 23)
        a, rx = np_.array(v), np_.array(x)
        out = []
        for side in ("left", "right"):
            out += [np_.searchsorted(a, rx, side=side),
                    np_.searchsorted(a, rx.T[::2], side=side),
                    np_.searchsorted(a, rx[0] + 0.5, side=side),
                    np_.searchsorted(v, rx, side=side),
                    np_.array([np_.searchsorted(a, 7, side=side)])]
        return out
    """, world=world)
