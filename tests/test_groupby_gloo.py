"""groupby over CPU ranks (gloo, worlds 2 and 3): the exchange of
runtime.group_op on the oracle backend.  The data are small integers stored
as floats, so the one-rank result is the np.<ufunc>.at model bit for bit, and
the merge in ascending source-rank order must reproduce it."""

import pytest

from test_take_gloo import run_spmd

BODY = """
    rng = np.random.default_rng(2)
    h = rng.integers(-4, 5, size={shape}).astype(np.float32)
    lab = rng.integers(0, 6, size=h{view}.shape[{dim}])
    lab[lab == 2] = 5                       # an empty group
    ufunc, ident = {{"sum": (np.add, 0), "min": (np.minimum, np.inf)}}["{op}"]
    if np_ is np:
        x = np.moveaxis(h{view}, {dim}, 0)
        out = np.full((7,) + x.shape[1:], ident, np.float32)
        ufunc.at(out, lab, x)
        return np.moveaxis(out, 0, {dim})
    return np_.array(h){view}.groupby({dim}, lab, 7).{op}()
"""


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("op", ["sum", "min"])
@pytest.mark.parametrize("shape,view,dim", [
    ((41, 6), "", 0),           # split along dim: every rank holds part of
                                # each group
    ((4, 41), "", 1),           # split along the other axis
    ((41, 6), "[:5, ::-1]", 0),  # the later ranks own no row of the view
])
def test_result_equals_the_one_rank_model(world, op, shape, view, dim):
    run_spmd(BODY.format(shape=shape, view=view, dim=dim, op=op), world=world)
