"""Float kernels on hostile values: NaN, +-inf, +-0, subnormals, huge
arguments, arguments on a range-reduction boundary, sums that cancel.

Host data goes in through `fromarray`; results are compared with the
correctly rounded fixtures in golden/numeric/ (written by
golden/generate.py with mpmath) or with NumPy directly -- never with the
oracle backend.  NaN positions, infinities and the sign of zero are exact
everywhere; accuracy bounds are the caps of DESIGN.md §6 (OpenCL
full-profile for ocml, fdlibm's 1 ulp for rt_sincos), not figures tuned to
the kernels.  Reductions use the order-independent bound
|got - exact| <= (n - 1) * u * sum|x_i| with `exact` from math.fsum.

Run with -s to see the measured maximum of every accuracy case.
"""

import functools

import numpy as np
import pytest

from numeric_util import (U, assert_exact, assert_within, exact_prefix_sums,
                          exact_prod, exact_sum, fixture)

pytestmark = pytest.mark.gpu

TAGS = [("64", np.float64), ("32", np.float32)]

# caps in spacings of the correctly rounded value
UNARY_BOUND = {"sqrt": 0, "exp": 3, "log": 3, "tan": 5, "tanh": 5,
               "arctan": 5, "sinh": 4, "cosh": 4, "arcsin": 4, "arccos": 4}
OCML_SINCOS = 4      # ocml sin/cos, including rt_sincos' |x| >= 1e6 hand-off
RT_SINCOS = 1        # rt_sincos fast path, |x| < 1e6
POW_BOUND = 16


@pytest.fixture(autouse=True)
def quiet_numpy():
    with np.errstate(all="ignore"):
        yield


# ---------------------------------------------------------------------------
# sin / cos
# ---------------------------------------------------------------------------

def _odd(*arrs):
    """Make the common length odd (no multiple of any vector width) by
    repeating the first element at the end; nothing is dropped."""
    if arrs[0].size % 2:
        return arrs if len(arrs) > 1 else arrs[0]
    out = tuple(np.concatenate([a, a[:1]]) for a in arrs)
    return out if len(out) > 1 else out[0]


@functools.lru_cache(maxsize=None)
def _sincos(tag):
    z = fixture("sincos")
    return _odd(z["x" + tag], z["sin" + tag], z["cos" + tag])


def _check_sincos64(got, want, x, what):
    fast = np.abs(x) < 1.0e6
    assert_within(got[fast], want[fast], RT_SINCOS, what + " |x|<1e6")
    assert_within(got[~fast], want[~fast], OCML_SINCOS, what + " fallback")


def test_sin_solo_fp64(ra_gpu):
    x, s_ref, _ = _sincos("64")
    got = ra_gpu.sin(ra_gpu.fromarray(x)).asarray()
    _check_sincos64(got, s_ref, x, "sin fp64 solo")
    s0 = ra_gpu.sin(ra_gpu.fromarray(np.array([-0.0, 0.0, -0.0]))).asarray()
    assert list(np.signbit(s0)) == [True, False, True]


def test_cos_solo_fp64(ra_gpu):
    x, _, c_ref = _sincos("64")
    got = ra_gpu.cos(ra_gpu.fromarray(x)).asarray()
    _check_sincos64(got, c_ref, x, "cos fp64 solo")


def test_sincos_paired_fp64(ra_gpu):
    """sin and cos of one operand in one fused kernel share a single
    rt_sincos call.  Both results are checked on their own, and so is
    sin(x) * 2 + cos(x), in which a quadrant swap cannot cancel."""
    x, s_ref, c_ref = _sincos("64")
    X = ra_gpu.fromarray(x)
    S = ra_gpu.sin(X)
    C = ra_gpu.cos(X)
    E = S * 2 + C
    ra_gpu.sync()
    _check_sincos64(S.asarray(), s_ref, x, "sin fp64 paired")
    _check_sincos64(C.asarray(), c_ref, x, "cos fp64 paired")
    got = E.asarray()
    ref = s_ref * 2 + c_ref
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    # got = fl(2 s' + c') with s', c' within b spacings of s, c (b = 4 covers
    # both paths); the doubling is exact, the add rounds once on each side
    # (at most one spacing of 2|s| + |c| together)
    b = OCML_SINCOS
    tol = 2 * b * np.spacing(np.abs(s_ref[ok])) \
        + b * np.spacing(np.abs(c_ref[ok])) \
        + np.spacing(2 * np.abs(s_ref[ok]) + np.abs(c_ref[ok]))
    err = np.abs(got[ok] - ref[ok])
    assert (err <= tol).all(), (np.flatnonzero(err > tol)[:8],)


def test_sincos_paired_expression_only_fp64(ra_gpu):
    """The same expression with the intermediates dead (registers only)."""
    x, s_ref, c_ref = _sincos("64")
    X = ra_gpu.fromarray(x)
    got = (ra_gpu.sin(X) * 2 + ra_gpu.cos(X)).asarray()
    ref = s_ref * 2 + c_ref
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    b = OCML_SINCOS
    tol = 2 * b * np.spacing(np.abs(s_ref[ok])) \
        + b * np.spacing(np.abs(c_ref[ok])) \
        + np.spacing(2 * np.abs(s_ref[ok]) + np.abs(c_ref[ok]))
    err = np.abs(got[ok] - ref[ok])
    assert (err <= tol).all(), (np.flatnonzero(err > tol)[:8],)


def test_sincos_fp32(ra_gpu):
    x, s_ref, c_ref = _sincos("32")
    got = ra_gpu.sin(ra_gpu.fromarray(x)).asarray()
    assert_within(got, s_ref, OCML_SINCOS, "sin fp32 solo")
    got = ra_gpu.cos(ra_gpu.fromarray(x)).asarray()
    assert_within(got, c_ref, OCML_SINCOS, "cos fp32 solo")
    X = ra_gpu.fromarray(x)
    S = ra_gpu.sin(X)
    C = ra_gpu.cos(X)
    ra_gpu.sync()
    assert_within(S.asarray(), s_ref, OCML_SINCOS, "sin fp32 paired")
    assert_within(C.asarray(), c_ref, OCML_SINCOS, "cos fp32 paired")


# ---------------------------------------------------------------------------
# other unaries: one fused kernel per (op, dtype)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tag,dtype", TAGS)
@pytest.mark.parametrize("op", sorted(UNARY_BOUND))
def test_unary(ra_gpu, op, tag, dtype):
    z = fixture("unary")
    x, want = _odd(z[f"{op}_x{tag}"], z[f"{op}_y{tag}"])
    assert x.dtype == dtype and x.size % 2 == 1 and x.size > 256
    got = getattr(ra_gpu, op)(ra_gpu.fromarray(x)).asarray()
    assert_within(got, want, UNARY_BOUND[op], f"{op} fp{tag}")


# ---------------------------------------------------------------------------
# binaries
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tag,dtype", TAGS)
@pytest.mark.parametrize("op", ["floordiv", "mod", "minimum", "maximum"])
def test_binary_exact_array_array(ra_gpu, op, tag, dtype):
    z = fixture("binary")
    a, b, want = _odd(z["a" + tag], z["b" + tag], z[op + tag])
    A, B = ra_gpu.fromarray(a), ra_gpu.fromarray(b)
    got = {"floordiv": lambda: A // B, "mod": lambda: A % B,
           "minimum": lambda: ra_gpu.minimum(A, B),
           "maximum": lambda: ra_gpu.maximum(A, B)}[op]().asarray()
    assert_exact(got, want)


@pytest.mark.parametrize("tag,dtype", TAGS)
def test_floordiv_mod_array_scalar(ra_gpu, tag, dtype):
    """k*d // d and k // d against NumPy, divisor as a scalar (both signs,
    zero and inf included)."""
    z = fixture("binary")
    a = _odd(z["a" + tag])
    A = ra_gpu.fromarray(a)
    for d in list(z["decimals"]) + [-0.3, 0.0, -0.0, np.inf, -np.inf, 7.0]:
        d = float(d)
        assert_exact((A // d).asarray(), a // d)
        assert_exact((A % d).asarray(), a % d)
        assert_exact((d // A).asarray(), d // a)
        assert_exact((d % A).asarray(), d % a)


@pytest.mark.parametrize("tag,dtype", TAGS)
def test_pow_array_array(ra_gpu, tag, dtype):
    z = fixture("binary")
    a, b, want = _odd(z["pow_a" + tag], z["pow_b" + tag], z["pow_y" + tag])
    got = (ra_gpu.fromarray(a) ** ra_gpu.fromarray(b)).asarray()
    assert_within(got, want, POW_BOUND, f"pow fp{tag} array**array")


@pytest.mark.parametrize("tag,dtype", TAGS)
def test_pow_array_scalar(ra_gpu, tag, dtype):
    """Integer exponents 0..8 take the multiply chain, 0.5 the pow call."""
    z = fixture("binary")
    base, want = z["pow_sbase" + tag], z["pow_sy" + tag]
    A = ra_gpu.fromarray(base)
    for i, e in enumerate(z["pow_exponents"]):
        e = int(e) if float(e).is_integer() else float(e)
        got = (A ** e).asarray()
        assert_within(got, want[i], POW_BOUND, f"pow fp{tag} **{e}")


# ---------------------------------------------------------------------------
# predicates, sign, abs, where on the special-value grid
# ---------------------------------------------------------------------------

def _grid(tag):
    z = fixture("binary")
    a, b = z["a" + tag], z["b" + tag]
    # the special-value grid is stored after the decimal pairs: 17 x 17
    special = np.isnan(a) | np.isinf(a) | (a == 0) | np.isnan(b) \
        | np.isinf(b) | (b == 0)
    first = int(np.flatnonzero(special)[0])
    return a[first:first + 289], b[first:first + 289]


@pytest.mark.parametrize("tag,dtype", TAGS)
def test_predicates_sign_abs_where(ra_gpu, tag, dtype):
    a, b = _grid(tag)
    assert np.isnan(a).any() and np.isinf(a).any() and (a == 0).any() \
        and np.signbit(a[a == 0]).any() and a.size == 289
    A, B = ra_gpu.fromarray(a), ra_gpu.fromarray(b)
    for name in ("isnan", "isinf", "isfinite"):
        got = getattr(ra_gpu, name)(A).asarray()
        assert got.dtype == np.bool_
        assert np.array_equal(got, getattr(np, name)(a)), name
    assert_exact(ra_gpu.sign(A).asarray(), np.sign(a))
    assert_exact(ra_gpu.absolute(A).asarray(), np.abs(a))
    assert_exact((-A).asarray(), -a)
    assert_exact(ra_gpu.where(A < B, A, B).asarray(), np.where(a < b, a, b))
    assert_exact(ra_gpu.where(ra_gpu.isnan(A), B, A).asarray(),
                 np.where(np.isnan(a), b, a))
    for cmp in ("__lt__", "__le__", "__gt__", "__ge__", "__eq__", "__ne__"):
        got = getattr(A, cmp)(B).asarray()
        assert np.array_equal(got, getattr(a, cmp)(b)), cmp


# ---------------------------------------------------------------------------
# integer // and % : zero divisors, INT_MIN // -1
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int64, np.int32])
def test_int_floordiv_mod_zero_and_overflow(ra_gpu, dtype):
    ii = np.iinfo(dtype)
    v = np.array([0, 1, -1, 2, -2, 7, -7, 10, ii.min, ii.min + 1, ii.max],
                 dtype=dtype)
    a, b = [m.ravel().copy() for m in np.meshgrid(v, v, indexing="ij")]
    A, B = ra_gpu.fromarray(a), ra_gpu.fromarray(b)
    q, r = (A // B).asarray(), (A % B).asarray()
    assert_exact(q, a // b)
    assert_exact(r, a % b)
    assert not q[b == 0].any() and not r[b == 0].any()
    m1 = (a == ii.min) & (b == -1)
    assert q[m1][0] == ii.min and r[m1][0] == 0
    for d in (0, -1, 3):
        assert_exact((A // d).asarray(), a // d)
        assert_exact((A % d).asarray(), a % d)


# ---------------------------------------------------------------------------
# full reductions over host data
# ---------------------------------------------------------------------------
# A fused reduction kernel runs 256 threads x V lanes per block (V = 2 for
# fp64, 4 for fp32: codegen.decide_vec), so one block's tile is 512 fp64 /
# 1024 fp32 elements and TILE + 1 needs a second block.  The finish kernel
# is one block whose 256 threads stride over the partials (gen_finish:
# `for i = threadIdx.x; i < npartials; i += 256`); more than 256 partials,
# i.e. n > 256 * TILE, sends it round that loop a second time.

TILE = {"64": 256 * 2, "32": 256 * 4}


def _lengths(tag):
    return [1, 63, 64, 65, 255, 256, 257, TILE[tag] + 1,
            256 * TILE[tag] + 1]


PATTERNS = ["cancel", "mixed", "nan_first", "nan_last", "nan_seam", "inf_pm",
            "equal"]


@functools.lru_cache(maxsize=None)
def _red_data(pattern, n, tag, for_prod):
    dtype = dict(TAGS)[tag]
    rng = np.random.default_rng(n * 7 + len(pattern))
    if for_prod:
        # factors near 1 so that the exact product stays in the normal
        # range, where a relative bound means something
        w = 1.0 / 8 if n < 100000 else 1.0 / 64
        x = np.exp2(rng.uniform(-w, w, n)) * rng.choice([-1.0, 1.0], n)
        if pattern == "equal":
            x = np.full(n, 1 + 2.0 ** -12)
    elif pattern == "cancel":
        big = 1e16 if tag == "64" else 1e8
        x = np.resize(np.array([big, 1.0, -big, 1.0, 3.0, big, -3.0, -big]),
                      n)
    elif pattern == "equal":
        x = np.full(n, 0.1)
    else:
        x = np.exp(rng.uniform(np.log(1e-10), np.log(1e10), n)) \
            * rng.choice([-1.0, 1.0], n)
    x = x.astype(dtype)
    if pattern == "nan_first":
        x[0] = np.nan
    elif pattern == "nan_last":
        x[-1] = np.nan
    elif pattern == "nan_seam":
        # last lane of a wave / first of the next / block or tile seam
        seams = [s for s in (63, 64, 255, 256, TILE[tag] - 1, TILE[tag],
                             256 * TILE[tag]) if s < n]
        x[seams[-1] if seams else n // 2] = np.nan
    elif pattern == "inf_pm":
        x[n // 3] = np.inf
        if n > 1:
            x[(2 * n) // 3] = -np.inf
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _red_ref(pattern, n, tag, for_prod):
    """Exact references, computed once per data set."""
    x = _red_data(pattern, n, tag, for_prod)
    if for_prod:
        if not np.isfinite(x).all():
            return float(np.prod(x.astype(np.float64)))   # nan / +-inf
        return exact_prod(x)
    return exact_sum(x)


@pytest.mark.parametrize("tag,dtype", TAGS)
@pytest.mark.parametrize("op", ["sum", "mean", "min", "max", "prod"])
def test_full_reduction(ra_gpu, op, tag, dtype):
    u = U[np.dtype(dtype)]
    for n in _lengths(tag):
        for pattern in PATTERNS:
            if op == "prod" and pattern == "cancel":
                continue          # a property of sums; prod has its own data
            x = _red_data(pattern, n, tag, op == "prod")
            got = getattr(ra_gpu.fromarray(x), op)()
            got = float(got)
            where = (op, tag, n, pattern)
            if op in ("min", "max"):
                want = float(getattr(np, op)(x))
                assert (np.isnan(got) and np.isnan(want)) or got == want, \
                    (where, got, want)
            elif op == "prod":
                want = _red_ref(pattern, n, tag, True)
                if not np.isfinite(want):
                    assert (np.isnan(got) and np.isnan(want)) \
                        or got == want, (where, got, want)
                else:
                    assert abs(got - want) <= (n - 1) * u * abs(want), \
                        (where, got, want)
            else:
                exact, mag = _red_ref(pattern, n, tag, False)
                if not np.isfinite(exact):
                    assert (np.isnan(got) and np.isnan(exact)) \
                        or got == exact, (where, got, exact)
                elif op == "sum":
                    assert abs(got - exact) <= (n - 1) * u * mag, \
                        (where, got, exact)
                else:
                    # mean = fl(sum / n): the sum's bound over n plus one
                    # rounding of the quotient, |mean| <= mag / n
                    assert abs(got - exact / n) <= u * mag, \
                        (where, got, exact / n)


# ---------------------------------------------------------------------------
# axis reductions: exactly the lines that hold a NaN come back NaN
# ---------------------------------------------------------------------------

def _axis_data(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-100, 100, shape).astype(dtype)
    # a NaN in a few known places: first and last element, and inside
    flat = x.reshape(-1)
    for pos in (0, flat.size - 1, flat.size // 2 + 3, flat.size // 3):
        flat[pos] = np.nan
    return x


AXIS_CASES = [
    # 2-D: axis 0 (thread per column), axis 1 (lane-split), both
    ((70, 130), 0), ((70, 130), 1), ((70, 130), (0, 1)),
    # 3-D: every single axis and every pair
    ((9, 33, 70), 0), ((9, 33, 70), 1), ((9, 33, 70), 2),
    ((9, 33, 70), (0, 1)), ((9, 33, 70), (0, 2)), ((9, 33, 70), (1, 2)),
    # chunked two-stage path: reduced extent >= 2048, 8 outputs
    ((2100, 8), 0),
]


@pytest.mark.parametrize("tag,dtype", TAGS)
@pytest.mark.parametrize("shape,axis", AXIS_CASES)
def test_axis_reduction_nan_lines(ra_gpu, shape, axis, tag, dtype):
    x = _axis_data(shape, dtype, seed=len(shape) * 100 + sum(shape))
    nan_lines = np.isnan(x).any(axis=axis)
    # (all axes of the 2-D case reduce to the single, NaN, line)
    assert nan_lines.any() and (nan_lines.size == 1 or not nan_lines.all())
    X = ra_gpu.fromarray(x)
    u = U[np.dtype(dtype)]
    for op in ("min", "max", "sum"):
        r = getattr(X, op)(axis=axis)
        got = np.asarray(r.asarray() if hasattr(r, "asarray") else r)
        assert got.shape == nan_lines.shape and got.dtype == dtype
        assert np.array_equal(np.isnan(got), nan_lines), (op, axis)
        clean = ~nan_lines
        if op in ("min", "max"):
            want = getattr(np, op)(x, axis=axis)
            assert np.array_equal(got[clean], want[clean]), (op, axis)
        elif got.ndim:
            ax = (axis,) if isinstance(axis, int) else axis
            n = int(np.prod([shape[a] for a in ax]))
            lines = np.moveaxis(x, ax, range(-len(ax), 0)).reshape(
                nan_lines.shape + (n,))
            for idx in zip(*np.nonzero(clean)):
                exact, mag = exact_sum(lines[idx])
                assert abs(float(got[idx]) - exact) <= (n - 1) * u * mag, \
                    (op, axis, idx)


# ---------------------------------------------------------------------------
# cumsum: a NaN (or +inf ... -inf) poisons its suffix, never its prefix
# ---------------------------------------------------------------------------

SCAN_CHUNK = 4096        # elements per block of the flat scan kernels


@functools.lru_cache(maxsize=None)
def _scan_data(n, tag):
    dtype = dict(TAGS)[tag]
    x = np.random.default_rng(n).uniform(-1, 1, n).astype(dtype)
    sums, mags = exact_prefix_sums(x)
    x.setflags(write=False)
    return x, sums, mags


def _check_prefix(got, sums, mags, stop, u, where):
    k = np.arange(stop)
    err = np.abs(got[:stop].astype(np.float64) - sums[:stop])
    bad = err > k * u * mags[:stop]
    assert not bad.any(), (where, np.flatnonzero(bad)[:8])


@pytest.mark.parametrize("tag,dtype", TAGS)
@pytest.mark.parametrize("n", [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1,
                               3 * SCAN_CHUNK + 5])
def test_cumsum_flat_nan_suffix(ra_gpu, n, tag, dtype):
    x, sums, mags = _scan_data(n, tag)
    u = U[np.dtype(dtype)]
    got = ra_gpu.fromarray(x).cumsum().asarray()
    assert got.dtype == dtype
    _check_prefix(got, sums, mags, n, u, ("clean", n))
    # first, second, inside a thread's 16 items, wave seam, chunk seam, last
    for p in sorted({0, 1, 23, 1024 + 7, SCAN_CHUNK - 1, n // 2, n - 2,
                     n - 1} | ({SCAN_CHUNK, 2 * SCAN_CHUNK + 100}
                               if n > 2 * SCAN_CHUNK + 100 else set())):
        if not 0 <= p < n:
            continue
        y = x.copy()
        y[p] = np.nan
        got = ra_gpu.fromarray(y).cumsum().asarray()
        _check_prefix(got, sums, mags, p, u, ("nan", n, p))
        assert np.isnan(got[p:]).all(), ("nan", n, p)
        if p >= 1:
            q = p // 2                      # +inf at q, -inf later at p
            y = x.copy()
            y[q], y[p] = np.inf, -np.inf
            got = ra_gpu.fromarray(y).cumsum().asarray()
            _check_prefix(got, sums, mags, q, u, ("inf", n, q, p))
            assert (got[q:p] == np.inf).all(), ("inf", n, q, p)
            assert np.isnan(got[p:]).all(), ("inf", n, q, p)


# (shape, axis): 130 long on axis 0 takes the chunked 3-pass variant, 40 the
# thread-per-line walk, and the last axis the wave scan (130 > one wave)
@pytest.mark.parametrize("tag,dtype", TAGS)
@pytest.mark.parametrize("shape,axis", [((130, 37), 0), ((40, 37), 0),
                                        ((37, 130), 1)])
def test_cumsum_axis_nan_suffix(ra_gpu, shape, axis, tag, dtype):
    rng = np.random.default_rng(shape[0])
    x = rng.uniform(-1, 1, shape).astype(dtype)
    u = U[np.dtype(dtype)]
    length = shape[axis]
    nlines = shape[1 - axis]
    # line -> position of the event; the other lines stay clean
    events = {0: 0, 1: length - 1, 5: length // 2, nlines - 1: 33,
              7: 64 if length > 64 else 3}
    for kind in ("nan", "inf"):
        y = x.copy()
        lines = np.moveaxis(y, axis, -1)           # view: (nlines, length)
        for line, p in events.items():
            if kind == "nan":
                lines[line, p] = np.nan
            elif p >= 1:
                lines[line, p // 2], lines[line, p] = np.inf, -np.inf
        got = np.moveaxis(ra_gpu.fromarray(y).cumsum(axis=axis).asarray(),
                          axis, -1)
        assert got.dtype == dtype
        clean = np.moveaxis(x, axis, -1)
        for line in range(nlines):
            sums, mags = exact_prefix_sums(clean[line])
            p = events.get(line, length)
            if kind == "inf" and line in events and p >= 1:
                q = p // 2
                _check_prefix(got[line], sums, mags, q, u, (kind, line))
                assert (got[line, q:p] == np.inf).all(), (kind, line)
            elif kind == "inf" and line in events:
                p = length                  # p == 0: no event was placed
                _check_prefix(got[line], sums, mags, p, u, (kind, line))
            else:
                _check_prefix(got[line], sums, mags, p, u, (kind, line))
            assert np.isnan(got[line, p:]).all(), (kind, line)
