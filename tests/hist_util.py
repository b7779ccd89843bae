"""Shared by the histogram tests: one call on both sides, compared exactly."""

import numpy as np


def same(got, ref, what=""):
    got = got if isinstance(got, tuple) else (got,)
    ref = ref if isinstance(ref, tuple) else (ref,)
    for g, r in zip(got, ref):
        g = np.asarray(g.asarray() if hasattr(g, "asarray") else g)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, g.dtype)
        np.testing.assert_array_equal(g, r, err_msg=str(what))


def both(ra, fn, host, view=lambda np_, x: x, **kw):
    same(getattr(ra, fn)(view(ra, ra.fromarray(host)), **kw),
         getattr(np, fn)(view(np, host), **kw), (fn, host.dtype, kw))
