"""Case tables and input generators of tests/test_gpu_rt_kernels.py.

They live here, without any GPU dependency, so tests/test_rt_ref_host.py
can assert on the CPU that the float inputs the GPU suite really feeds the
scans keep every partial sum exact (integers, |x| <= 8, sums under 2^24 /
2^53): the GPU comparisons are then bit-exact whatever the summation
order."""

import numpy as np

F_BASE, I_BASE = 1000.0, 1000      # the nonzero cross-rank base of phase 3


def _seed(*key):
    h = 17
    for k in key:
        for ch in str(k):
            h = (h * 131 + ord(ch)) % (1 << 31)
    return h


def small_ints(shape, dtype, *key):
    """Integer values in [-8, 8] (uint8: [0, 8]) stored as `dtype`."""
    rng = np.random.default_rng(_seed(dtype, shape, *key))
    lo = 0 if np.dtype(dtype).kind == "u" else -8
    return rng.integers(lo, 9, size=shape).astype(dtype)


def base_of(dtype):
    return F_BASE if np.dtype(dtype).kind == "f" else I_BASE


# -- rt_cumsum ----------------------------------------------------------------

def cumsum_ns(C):
    return [1, 15, 16, 17, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5]


CUMSUM_STRIDES = [1, 3, -1]
PHASE2_LENGTHS = [1, 255, 256, 257, 1000]


def cumsum_trips_n(C):
    """13 chunks, the last one partial: 3 blocks take 5, 4 and 4 of them."""
    return 12 * C + 77


def cumsum_input(dtype, n):
    return small_ints((n,), dtype, "cumsum")


def phase2_input(dtype, n):
    return small_ints((n,), dtype, "bsums")


# -- rt_axis_scan -------------------------------------------------------------

AXIS_SHAPES = {2: (11, 65), 3: (5, 11, 13), 4: (5, 11, 5, 13)}
AXIS_CHUNKS = [2, 3, 7]     # never divide: 11 -> 6+5, 4+4+3, 5x2+1+empty
WAVE_LENGTHS = [1, 63, 64, 65, 130]
EMPTY_TAIL = ((9, 5), 0, 6)         # length 9 in 6 chunks of 2: the 6th empty
# (name, shape, axis, nchunks, dtype): each takes a second grid-stride trip
AXIS_BIG = [
    ("waves", (16390, 3), 1, 1, "int64"),       # > 4096 blocks x 4 waves
    ("lines", (3, 1048700), 0, 1, "float32"),   # > 4096 x 256 threads
    ("chunked", (1000, 2110), 0, 500, "int32"),  # 2110 x 499 > 4096 x 256
]


def axis_input(dtype, shape):
    return small_ints(tuple(shape), dtype, "axis")


def float_scan_inputs(C):
    """(dtype, values with the scan axis last, base) of every float scan."""
    for dtype in ("float64", "float32"):
        for n in cumsum_ns(C) + [cumsum_trips_n(C)]:
            yield dtype, cumsum_input(dtype, n), base_of(dtype)
        for n in PHASE2_LENGTHS:
            yield dtype, phase2_input(dtype, n), 0
        shapes = [(s, ax) for s in AXIS_SHAPES.values()
                  for ax in range(len(s))]
        shapes += [((5, L), 1) for L in WAVE_LENGTHS]
        shapes += [((3, 4, L), 2) for L in WAVE_LENGTHS]
        shapes.append((EMPTY_TAIL[0], EMPTY_TAIL[1]))
        shapes += [(s, ax) for (_, s, ax, _, dt) in AXIS_BIG if dt == dtype]
        for shape, ax in shapes:
            yield dtype, np.moveaxis(axis_input(dtype, shape), ax, -1), 0


# -- rt_combine_box -----------------------------------------------------------

LOGICAL_VALUES = [0, 1, 2, -3, 7, 0, 100, -128]


def combine_inputs(dtype, op, n):
    """(dst values, src values), 1-D of n.  add / mul: floats and the wide
    integers get small integers (exact, in range); int16 / int8 / uint8
    take their whole range and wrap like NumPy's same-dtype arithmetic.
    Logical ops see values other than 0 and 1 (and -0.0, 0.5 for floats)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(_seed(dtype, op, n))
    if op in ("land", "lor"):
        vals = np.array(LOGICAL_VALUES)
        if dt.kind == "u":
            vals = np.abs(vals)
        d = rng.choice(vals, n).astype(dtype)
        s = rng.choice(vals, n).astype(dtype)
        if dt.kind == "f":
            d[::11], s[::13] = -0.0, 0.5
        return d, s
    if dt.kind == "f" or dt.itemsize >= 4:
        return (small_ints((n,), dtype, op, "d"),
                small_ints((n,), dtype, op, "s"))
    info = np.iinfo(dt)
    return (rng.integers(info.min, info.max, n, endpoint=True).astype(dtype),
            rng.integers(info.min, info.max, n, endpoint=True).astype(dtype))


COMBINE_SHAPES = [(5, 130), (3, 4, 5, 6)]
COMBINE_BIG = (2049, 257)           # > 2048 blocks x 256 threads
COMBINE_BIG_CASES = [("float32", "add"), ("int16", "max"), ("uint8", "lor"),
                     ("int64", "min")]


def float_combine_inputs():
    for dtype in ("float64", "float32"):
        for op in ("add", "mul"):
            sizes = [int(np.prod(s)) for s in COMBINE_SHAPES]
            if (dtype, op) in COMBINE_BIG_CASES:
                sizes.append(int(np.prod(COMBINE_BIG)))
            for n in sizes:
                d, s = combine_inputs(dtype, op, n)
                yield dtype, np.concatenate([d, s])

