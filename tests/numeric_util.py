"""Comparators and exact references shared by the numeric-edge tests
(test_preamble_host.py on the CPU, test_gpu_numeric_edges.py on the GPU).

Everything here is plain NumPy / Python integers: the correctly rounded
function values come from the committed fixtures in golden/numeric/
(tests/golden/generate.py writes them with mpmath), so the tests
themselves need no multiprecision library.
"""

import functools
import math
import os
from fractions import Fraction

import numpy as np

NUMERIC = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "golden", "numeric")

# unit roundoff per float format
U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(NUMERIC, name + ".npz")) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def spacings(got, want):
    """|got - want| in spacings of the correctly rounded `want`.  Where the
    two agree exactly (same value, or NaN in both) the distance is 0; a NaN
    or an infinity on one side only is an infinite distance."""
    got = np.asarray(got)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) \
            / np.spacing(np.abs(want)).astype(np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    d[same] = 0.0
    d[~same & ~(np.isfinite(got) & np.isfinite(want))] = np.inf
    return d


def assert_signs(got, want):
    """Same sign bit wherever the expected value is not NaN (this is what
    sees -0.0 against +0.0; == cannot)."""
    ok = ~np.isnan(want)
    bad = ok & (np.signbit(got) != np.signbit(want))
    assert not bad.any(), (np.flatnonzero(bad)[:8], np.asarray(got)[bad][:8],
                           want[bad][:8])


def assert_exact(got, want):
    """Same dtype and shape, NaN in exactly the same places, every other
    value equal (so infinities match exactly) with the same sign bit."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.dtype.kind != "f":
        bad = got != want
        assert not bad.any(), (np.flatnonzero(bad)[:8], got[bad][:8],
                               want[bad][:8])
        return
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (got != want)) \
        | (~nan & (np.signbit(got) != np.signbit(want)))
    assert not bad.any(), (np.flatnonzero(bad)[:8], got[bad][:8],
                           want[bad][:8])


def assert_within(got, want, bound, what=""):
    """Every element within `bound` spacings of the fixture value, NaN and
    inf positions exact, sign bits equal.  Prints the measured maximum so a
    run with -s records it."""
    d = spacings(got, want)
    worst = int(np.argmax(d))
    print(f"{what}: max {d.max():.3g} spacings (bound {bound}) "
          f"at index {worst}")
    assert d.max() <= bound, (what, d.max(), worst, np.asarray(got)[worst],
                              want[worst])
    assert_signs(np.asarray(got), want)
    return float(d.max())


# -- exact references for reductions ----------------------------------------

def exact_sum(x):
    """(exact sum rounded once, sum of magnitudes) with math.fsum; NaN or
    inf inputs follow IEEE (fsum raises on inf - inf, which is NaN)."""
    xs = [float(v) for v in np.asarray(x).ravel()]
    if any(math.isnan(v) for v in xs):
        return math.nan, math.nan
    pinf = any(v == math.inf for v in xs)
    ninf = any(v == -math.inf for v in xs)
    if pinf or ninf:
        return (math.nan if pinf and ninf else
                (math.inf if pinf else -math.inf)), math.inf
    return math.fsum(xs), math.fsum(abs(v) for v in xs)


def exact_prod(x):
    """Product of finite floats, exact to better than 2^-230 and then
    rounded once to a float.  Each value is a 53-bit integer times a power
    of two; the integer product is cut back to 256 bits whenever it passes
    512, a relative error below 2^-255 per cut -- against bounds of
    (n - 1) * 2^-53 the reference's own error is nothing.  Up to 9 factors
    are never cut, so short products are exact."""
    man, exp = 1, 0
    for v in np.asarray(x, dtype=np.float64).ravel().tolist():
        m, e = math.frexp(v)
        man *= int(m * 9007199254740992.0)        # m * 2^53, exact
        exp += e - 53
        excess = man.bit_length() - 512
        if excess > 0:
            man >>= excess + 256
            exp += excess + 256
    # int / int and float(int) are correctly rounded in Python
    return float(man << exp) if exp >= 0 else man / (1 << -exp)


def exact_prefix_sums(x):
    """(correctly rounded prefix sums, prefix sums of magnitudes) of a
    finite 1-D array, accumulated exactly in rationals."""
    run, mag = Fraction(0), Fraction(0)
    sums, mags = [], []
    for v in np.asarray(x).ravel():
        f = Fraction(float(v))
        run += f
        mag += abs(f)
        sums.append(float(run))
        mags.append(float(mag))
    return np.array(sums), np.array(mags)
