"""Generate the committed golden fixtures.

Two families:

* `tests/golden/*.npz` -- whole programs from `golden_cases.py`, evaluated
  by the NumPy oracle (the same executable oracle the reference's own CI
  compares against: run_both, ramba/tests/test_distributed_array.py:240-259).
* `tests/golden/numeric/*.npz` -- hostile inputs for the float kernels
  (NaN, +-inf, +-0, subnormals, range-reduction boundaries, overflow
  thresholds) with CORRECTLY ROUNDED expected outputs, fp64 and fp32,
  computed with mpmath at 256 bits and rounded once to the target format
  with integer arithmetic.  The tests that read them need no mpmath; this
  generator does.  They live in a subfolder because test_golden_fixtures
  globs `golden/*.npz` and looks every name up in CASES.

Run from the repo root:  python tests/golden/generate.py [--numeric-only]
"""

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from golden_cases import CASES_TOL  # noqa: E402

NUMERIC = os.path.join(HERE, "numeric")
PREC = 256          # working bits; >= 200 so one rounding decides the result


# ---------------------------------------------------------------------------
# correct rounding of an mpmath value to binary64 / binary32
# ---------------------------------------------------------------------------

_FMT = {np.dtype(np.float64): (53, -1074, 1024),
        np.dtype(np.float32): (24, -149, 128)}


def round_mpf(v, dt):
    """mpf -> nearest value of float format `dt` (ties to even, gradual
    underflow, overflow to inf), returned as a Python float that is exactly
    representable in `dt`.  One rounding, done on integers."""
    import mpmath
    if mpmath.isnan(v):
        return math.nan
    if mpmath.isinf(v):
        return math.inf if v > 0 else -math.inf
    p, qmin, emax = _FMT[np.dtype(dt)]
    sign, man, exp, _ = v._mpf_
    man = int(man)
    if man == 0:
        return 0.0
    e = man.bit_length() + exp          # |v| in [2^(e-1), 2^e)
    q = max(e - p, qmin)                # exponent of the result's quantum
    sh = exp - q
    if e > emax:
        n, q = 1, emax                  # overflow
    elif e < qmin - 1:
        n = 0                           # below half the smallest subnormal
    elif sh >= 0:
        n = man << sh
    else:
        n, rem = divmod(man, 1 << -sh)
        half = 1 << (-sh - 1)
        if rem > half or (rem == half and (n & 1)):
            n += 1
    if n.bit_length() + q > emax:
        r = math.inf
    else:
        r = math.ldexp(float(n), q)     # n <= 2^p: exact
    return -r if sign else r


# ---------------------------------------------------------------------------
# unary functions: value of f at the EXACT input, correctly rounded
# ---------------------------------------------------------------------------

_PIO2 = "pi/2"     # marker: atan(+-inf), acos(0)


def _mp_fn(op):
    import mpmath as mp
    return {"sin": mp.sin, "cos": mp.cos, "tan": mp.tan, "exp": mp.exp,
            "log": mp.log, "sqrt": mp.sqrt, "tanh": mp.tanh,
            "arctan": mp.atan, "sinh": mp.sinh, "cosh": mp.cosh,
            "arcsin": mp.asin, "arccos": mp.acos}[op]


# value at +inf / -inf (C99 Annex F)
_AT_INF = {
    "sin": (math.nan, math.nan), "cos": (math.nan, math.nan),
    "tan": (math.nan, math.nan), "exp": (math.inf, 0.0),
    "log": (math.inf, math.nan), "sqrt": (math.inf, math.nan),
    "tanh": (1.0, -1.0), "arctan": (_PIO2, _PIO2),
    "sinh": (math.inf, -math.inf), "cosh": (math.inf, math.inf),
    "arcsin": (math.nan, math.nan), "arccos": (math.nan, math.nan),
}
# functions with f(+-0) = +-0
_ODD_AT_ZERO = {"sin", "tan", "sqrt", "tanh", "arctan", "sinh", "arcsin"}


def exact_unary(op, x, dt):
    """Correctly rounded f(x) in format dt for one Python-float input."""
    import mpmath as mp
    if math.isnan(x):
        return math.nan
    if math.isinf(x):
        r = _AT_INF[op][0 if x > 0 else 1]
        if r is _PIO2:
            r = round_mpf(mp.pi / 2, dt)
            return r if x > 0 else -r
        return r
    if x == 0.0:
        if op in _ODD_AT_ZERO:
            return x                     # keeps the sign of zero
        if op == "log":
            return -math.inf
    if op == "log" and x < 0:
        return math.nan
    if op == "sqrt" and x < 0:
        return math.nan
    if op in ("arcsin", "arccos") and abs(x) > 1:
        return math.nan
    return round_mpf(_mp_fn(op)(mp.mpf(x)), dt)


def eval_unary(op, xs, dt):
    return np.array([exact_unary(op, float(x), dt) for x in xs], dtype=dt)


# ---------------------------------------------------------------------------
# input sets
# ---------------------------------------------------------------------------

def _with_neighbours(x, dt):
    x = np.asarray(x, dtype=dt)
    inf = np.asarray(np.inf, dtype=dt)
    return np.concatenate([np.nextafter(x, -inf), x, np.nextafter(x, inf)])


def _log_uniform(rng, lo, hi, n, dt, signed=True):
    mag = np.exp(rng.uniform(math.log(lo), math.log(hi), n))
    if signed:
        mag = mag * rng.choice([-1.0, 1.0], n)
    with np.errstate(over="ignore", under="ignore"):
        return mag.astype(dt)


def _specials(dt):
    fi = np.finfo(dt)
    return np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal,
                     fi.tiny, -fi.tiny, fi.tiny * 0.37, fi.max, -fi.max,
                     np.inf, -np.inf, np.nan], dtype=dt)


def sincos_inputs(dt):
    """Arguments for sin/cos: the floats nearest to k*pi/2 (range-reduction
    boundaries, where the reduced argument cancels) with both neighbours
    and both signs, random arguments, and the special values."""
    import mpmath as mp
    dt = np.dtype(dt)
    rng = np.random.default_rng(20240607 + dt.itemsize)
    f64 = dt == np.float64
    nk, nrand = (2000, 2000) if f64 else (600, 600)
    ks = list(range(1, nk + 1))
    ks += [int(k) for k in rng.integers(nk + 1, 636619, nrand)]
    ks += [636618, 636619]
    near = np.array([round_mpf(k * mp.pi / 2, dt) for k in ks], dtype=dt)
    near = _with_neighbours(near, dt)
    near = np.concatenate([near, -near])
    fi = np.finfo(dt)
    one_e6 = np.asarray(1e6, dtype=dt)
    inf = np.asarray(np.inf, dtype=dt)
    nu = 2000 if f64 else 800
    edges = np.array([0.0, -0.0, fi.smallest_subnormal,
                      -fi.smallest_subnormal,
                      1e-310 if f64 else 1e-40,
                      np.nextafter(one_e6, dt.type(0)), one_e6,
                      np.nextafter(one_e6, inf),
                      1e22, -1e22, fi.max, np.inf, -np.inf, np.nan],
                     dtype=dt)
    return np.concatenate([
        near,
        rng.uniform(-1e6, 1e6, nu).astype(dt),
        _log_uniform(rng, 1e-300 if f64 else 1e-44, 1e6, nu, dt),
        edges])


def unary_inputs(op, dt):
    """Log-uniform sweep of the function's domain plus its own edges."""
    dt = np.dtype(dt)
    f64 = dt == np.float64
    fi = np.finfo(dt)
    rng = np.random.default_rng(sum(map(ord, op)) * 1000 + dt.itemsize)
    tiny_lo = 1e-300 if f64 else 1e-44
    huge = 1e300 if f64 else 1e38
    N = 1200
    one = dt.type(1)
    inf = dt.type(np.inf)
    log_max = math.log(float(fi.max))                       # exp overflow
    log_sub = math.log(float(fi.smallest_subnormal))        # exp -> 0
    log_tiny = math.log(float(fi.tiny))                     # exp subnormal
    parts = [_specials(dt)]
    if op == "exp":
        parts += [_log_uniform(rng, tiny_lo, log_max, N, dt),
                  rng.uniform(log_sub - 2, log_max + 1, N).astype(dt),
                  _with_neighbours([log_max, log_sub, log_sub - math.log(2),
                                    log_tiny, 1.0, -1.0], dt),
                  np.array([log_max + 1, log_sub - 2, 1000, -1000], dt)]
    elif op == "log":
        parts += [_log_uniform(rng, tiny_lo, huge, N, dt, signed=False),
                  rng.uniform(0.5, 2.0, N // 2).astype(dt),
                  _with_neighbours([1.0, 2.0, 0.5, math.e], dt),
                  np.array([1e-310 if f64 else 1e-40, -1.0, -fi.tiny], dt)]
    elif op == "sqrt":
        parts += [_log_uniform(rng, tiny_lo, huge, N, dt, signed=False),
                  (rng.integers(1, 4096, 200).astype(dt)) ** 2,
                  _with_neighbours([1.0, 2.0, 4.0, 0.25], dt),
                  np.array([1e-310 if f64 else 1e-40, -1.0, -fi.tiny], dt)]
    elif op == "tanh":
        parts += [_log_uniform(rng, tiny_lo, 1e3, N, dt),
                  rng.uniform(-25, 25, N // 2).astype(dt),
                  _with_neighbours([19.0615474653984, 9.010913, 0.5493061,
                                    22.0, 1.0], dt)]
    elif op == "arctan":
        parts += [_log_uniform(rng, tiny_lo, huge, N, dt),
                  rng.uniform(-4, 4, N // 2).astype(dt),
                  _with_neighbours([1.0, -1.0, 0.4375, 0.6875, 1.1875,
                                    2.4375], dt)]
    elif op == "tan":
        import mpmath as mp
        odd = np.array([round_mpf((2 * k + 1) * mp.pi / 2, dt)
                        for k in range(0, 150)], dtype=dt)
        parts += [_log_uniform(rng, tiny_lo, 1e6, N, dt),
                  rng.uniform(-1e6, 1e6, N // 2).astype(dt),
                  _with_neighbours(odd, dt), -odd,
                  np.array([1e22, -1e22], dt)]
    elif op in ("sinh", "cosh"):
        ovf = log_max + math.log(2)          # sinh/cosh overflow threshold
        parts += [_log_uniform(rng, tiny_lo, ovf, N, dt),
                  rng.uniform(-ovf - 1, ovf + 1, N // 2).astype(dt),
                  _with_neighbours([ovf, -ovf, log_max, 1.0, 22.0], dt),
                  np.array([ovf + 1, -ovf - 1], dt)]
    elif op in ("arcsin", "arccos"):
        parts += [_log_uniform(rng, tiny_lo, 1.0, N, dt),
                  rng.uniform(-1, 1, N // 2).astype(dt),
                  (1 - _log_uniform(rng, float(fi.eps), 0.5, 200, dt,
                                    signed=False)).astype(dt),
                  np.array([1.0, -1.0, np.nextafter(one, dt.type(0)),
                            -np.nextafter(one, dt.type(0)),
                            np.nextafter(one, inf), -np.nextafter(one, inf),
                            2.0, -2.0, 0.5, -0.5], dt)]
    else:
        raise KeyError(op)
    with np.errstate(all="ignore"):
        return np.concatenate([np.asarray(p, dtype=dt) for p in parts])


UNARY_OPS = ["exp", "log", "sqrt", "tanh", "arctan", "tan", "sinh", "cosh",
             "arcsin", "arccos"]
POW_EXPONENTS = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 0.5]
DECIMALS = [0.1, 0.2, 0.3, 0.7, 0.01]


def special_grid(dt):
    """Every sign combination of {0, finite, inf, nan} (finite covers a
    non-integer ratio, a subnormal and a huge value)."""
    fi = np.finfo(dt)
    v = np.array([0.0, -0.0, 1.5, -1.5, 7.0, -7.0, 0.1, -0.1, 1.0, -1.0,
                  fi.smallest_subnormal, -fi.smallest_subnormal,
                  fi.max, -fi.max, np.inf, -np.inf, np.nan], dtype=dt)
    a, b = np.meshgrid(v, v, indexing="ij")
    return a.ravel().copy(), b.ravel().copy()


def divmod_inputs(dt):
    """Pairs for // % minimum maximum: decimal multiples k*d // d and
    k // d (where floor(a / b) is wrong), with every sign pattern, plus the
    special-value grid (zero divisors included)."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(77 + dt.itemsize)
    A, B = [], []
    for d in DECIMALS:
        k = rng.integers(1, 1000, 240).astype(np.float64)
        dd = dt.type(d)
        kd = (k.astype(dt) * dd).astype(dt)
        for sa, sb in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            # all 240 with both positive, the last 60 for each other sign
            q = slice(0 if (sa, sb) == (1, 1) else 180, None)
            A += [sa * kd[q], sa * k.astype(dt)[q]]
            B += [np.full(kd[q].shape, sb * dd, dt)] * 2
    ga, gb = special_grid(dt)
    A.append(ga)
    B.append(gb)
    A.append(rng.uniform(-100, 100, 301).astype(dt))
    B.append(rng.uniform(-10, 10, 301).astype(dt))
    return np.concatenate(A).astype(dt), np.concatenate(B).astype(dt)


def exact_pow(a, b, dt):
    """Correctly rounded a**b; every C99 special case (zero, inf or nan
    operand, negative base with a non-integer exponent) is taken from
    NumPy's float64 libm pow, which implements Annex F exactly."""
    import mpmath as mp
    if (not math.isfinite(a)) or (not math.isfinite(b)) or a == 0.0 \
            or b == 0.0 or (a < 0 and b != math.floor(b)):
        with np.errstate(all="ignore"):
            return float(np.power(np.float64(a), np.float64(b)))
    mag = mp.power(mp.mpf(abs(a)), mp.mpf(b))
    if a < 0 and int(b) % 2:
        mag = -mag                       # negative base, odd integer power
    return round_mpf(mag, dt)


def pow_inputs(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(99 + dt.itemsize)
    n = 1500
    base = np.concatenate([
        _log_uniform(rng, 1e-3, 1e3, n, dt, signed=False),
        -_log_uniform(rng, 1e-2, 1e2, 300, dt, signed=False)])
    expo = np.concatenate([
        rng.uniform(-8, 8, n),
        rng.integers(-9, 10, 300).astype(np.float64)]).astype(dt)
    # exponents 0..8 and 0.5 as ARRAY operands (the general pow call)
    b2 = np.concatenate([_log_uniform(rng, 1e-3, 1e3, 40, dt),
                         np.array([0.0, -0.0, 1.0, -1.0], dt)])
    eb, ee = np.meshgrid(b2, np.array(POW_EXPONENTS, dt), indexing="ij")
    ga, gb = special_grid(dt)
    a = np.concatenate([base, eb.ravel(), ga]).astype(dt)
    b = np.concatenate([expo, ee.ravel(), gb]).astype(dt)
    # bases for the SCALAR-exponent (multiply chain) path
    sb = np.concatenate([_log_uniform(rng, 1e-3, 1e3, 700, dt),
                         np.array([0.0, -0.0, np.inf, -np.inf, np.nan,
                                   1.0, -1.0], dt)]).astype(dt)
    return a, b, sb


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------

def _save(name, **arrs):
    os.makedirs(NUMERIC, exist_ok=True)
    path = os.path.join(NUMERIC, f"{name}.npz")
    np.savez_compressed(path, **arrs)
    print(f"numeric/{name}: {sum(a.size for a in arrs.values())} values, "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def generate_numeric():
    import mpmath as mp
    mp.mp.prec = PREC
    tags = (("64", np.float64), ("32", np.float32))

    out = {}
    for tag, dt in tags:
        x = sincos_inputs(dt)
        out[f"x{tag}"] = x
        out[f"sin{tag}"] = eval_unary("sin", x, dt)
        out[f"cos{tag}"] = eval_unary("cos", x, dt)
    _save("sincos", **out)

    out = {}
    for op in UNARY_OPS:
        for tag, dt in tags:
            x = unary_inputs(op, dt)
            out[f"{op}_x{tag}"] = x
            out[f"{op}_y{tag}"] = eval_unary(op, x, dt)
    _save("unary", **out)

    # //, %, minimum, maximum are exact operations whose definition IS
    # NumPy's (npy_divmod); their expected values are NumPy's own, recorded
    # here so the file also pins them across NumPy versions
    out = {"decimals": np.array(DECIMALS), "pow_exponents":
           np.array(POW_EXPONENTS)}
    with np.errstate(all="ignore"):
        for tag, dt in tags:
            a, b = divmod_inputs(dt)
            out[f"a{tag}"], out[f"b{tag}"] = a, b
            out[f"floordiv{tag}"] = np.floor_divide(a, b)
            out[f"mod{tag}"] = np.mod(a, b)
            out[f"minimum{tag}"] = np.minimum(a, b)
            out[f"maximum{tag}"] = np.maximum(a, b)
            pa, pb, sb = pow_inputs(dt)
            out[f"pow_a{tag}"], out[f"pow_b{tag}"] = pa, pb
            out[f"pow_y{tag}"] = np.array(
                [exact_pow(float(u), float(v), dt) for u, v in zip(pa, pb)],
                dtype=dt)
            out[f"pow_sbase{tag}"] = sb
            out[f"pow_sy{tag}"] = np.array(
                [[exact_pow(float(u), e, dt) for u in sb]
                 for e in POW_EXPONENTS], dtype=dt)
    _save("binary", **out)


def main():
    if "--numeric-only" not in sys.argv:
        for name, (fn, tol) in CASES_TOL.items():
            out = fn(np)
            path = os.path.join(HERE, f"{name}.npz")
            np.savez_compressed(path, out=np.asarray(out),
                                tol=np.float64(tol))
            print(f"{name}: shape={np.asarray(out).shape} tol={tol} "
                  f"-> {path}")
    generate_numeric()


if __name__ == "__main__":
    main()
