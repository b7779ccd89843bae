"""The pair comparator of the arg-reduction kernels (rt_arg_better,
include/ramba_argcmp.h — the one function every kernel and the cross-rank
combine merge with), compiled for the HOST with a small stand-alone main
and run over a table of (value, index) pairs.  No GPU.

The same table also pins `ramba_amd.argreduce.better`, the NumPy
restatement the host merge uses, so the two cannot drift apart.
"""

import os
import subprocess

import numpy as np
import pytest

from test_preamble_host import _find_clangxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ramba_argcmp.h"
// stdin rows: type pv pi qv qi is_max skipna  ->  one 0/1 per row
int main() {
    char t[8], pv[64], qv[64];
    long long pi, qi;
    int mx, sk;
    while (scanf("%7s %63s %lld %63s %lld %d %d", t, pv, &pi, qv, &qi, &mx,
                 &sk) == 7) {
        bool r;
        if (!strcmp(t, "f64"))
            r = rt_arg_better<double>(strtod(pv, 0), pi, strtod(qv, 0), qi,
                                      mx, sk);
        else if (!strcmp(t, "f32"))
            r = rt_arg_better<float>(strtof(pv, 0), pi, strtof(qv, 0), qi,
                                     mx, sk);
        else if (!strcmp(t, "i64"))
            r = rt_arg_better<int64_t>(strtoll(pv, 0, 10), pi,
                                       strtoll(qv, 0, 10), qi, mx, sk);
        else
            r = rt_arg_better<uint8_t>((uint8_t)atoi(pv), pi,
                                       (uint8_t)atoi(qv), qi, mx, sk);
        printf("%d\n", (int)r);
    }
    return 0;
}
"""

# (type, pv, pi, qv, qi, is_max, skipna, p replaces q)
TABLE = [
    # strict order
    ("f64", "2", 5, "1", 0, 1, 0, True),
    ("f64", "1", 0, "2", 5, 1, 0, False),
    ("f64", "1", 5, "2", 0, 0, 0, True),
    ("f64", "2", 0, "1", 5, 0, 0, False),
    # equal values: the lower index wins, either way round, max and min
    ("f64", "3", 2, "3", 7, 1, 0, True),
    ("f64", "3", 7, "3", 2, 1, 0, False),
    ("f64", "3", 2, "3", 7, 0, 0, True),
    ("f64", "3", 7, "3", 2, 0, 0, False),
    ("f64", "3", 4, "3", 4, 1, 0, False),      # a pair never beats itself
    # signed zeros tie
    ("f64", "-0.0", 1, "0.0", 2, 1, 0, True),
    ("f64", "0.0", 2, "-0.0", 1, 1, 0, False),
    ("f32", "-0.0", 1, "0.0", 2, 0, 0, True),
    ("f32", "0.0", 2, "-0.0", 1, 0, 0, False),
    # NaN / number: NaN wins whatever its index, for max and for min
    ("f64", "nan", 9, "1e300", 0, 1, 0, True),
    ("f64", "1e300", 0, "nan", 9, 1, 0, False),
    ("f64", "nan", 9, "-1e300", 0, 0, 0, True),
    ("f32", "inf", 0, "nan", 9, 1, 0, False),
    ("f32", "nan", 9, "inf", 0, 1, 0, True),
    # NaN / NaN: the first NaN wins
    ("f64", "nan", 3, "nan", 8, 1, 0, True),
    ("f64", "nan", 8, "nan", 3, 1, 0, False),
    ("f64", "nan", 3, "nan", 8, 0, 0, True),
    ("f64", "nan", 3, "nan", 3, 1, 0, False),
    # skipna: a NaN never wins and always gives way
    ("f64", "nan", 0, "1", 5, 1, 1, False),
    ("f64", "1", 5, "nan", 0, 1, 1, True),
    ("f64", "nan", 0, "nan", 5, 1, 1, False),
    ("f64", "nan", 0, "0", -1, 1, 1, False),
    ("f64", "2", 5, "1", 0, 1, 1, True),
    ("f64", "3", 7, "3", 2, 0, 1, False),
    ("f32", "-inf", 4, "nan", 0, 1, 1, True),
    # the -1 sentinel always loses, whatever value rides with it
    ("f64", "1e300", -1, "-1e300", 0, 1, 0, False),
    ("f64", "-1e300", 0, "1e300", -1, 1, 0, True),
    ("f64", "nan", -1, "0", 0, 1, 0, False),
    ("f64", "0", 0, "nan", -1, 1, 0, True),
    ("f64", "0", -1, "0", -1, 1, 0, False),
    ("f64", "0", 0, "0", -1, 0, 1, True),
    ("i64", "5", -1, "5", 3, 0, 0, False),
    # int64 compared as integers: a double cannot tell these apart
    ("i64", "4611686018427387905", 1, "4611686018427387904", 0, 1, 0, True),
    ("i64", "4611686018427387904", 0, "4611686018427387905", 1, 1, 0, False),
    ("i64", "4611686018427387904", 0, "4611686018427387905", 1, 0, 0, True),
    ("i64", "-9223372036854775808", 6, "9223372036854775807", 0, 0, 0, True),
    # bool / uint8
    ("u8", "1", 9, "0", 0, 1, 0, True),
    ("u8", "0", 9, "1", 0, 0, 0, True),
    ("u8", "255", 9, "1", 0, 1, 0, True),
    ("u8", "1", 9, "1", 0, 1, 1, False),
]


@pytest.fixture(scope="module")
def cmp_prog(tmp_path_factory):
    cxx = _find_clangxx()
    if cxx is None:
        pytest.skip("no ROCm clang++ found")
    d = tmp_path_factory.mktemp("argcmp_host")
    src = d / "argcmp_main.cpp"
    src.write_text(MAIN)
    exe = d / "argcmp_main"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


def test_comparator_table_on_the_host(cmp_prog):
    rows = "".join(f"{t} {pv} {pi} {qv} {qi} {mx} {sk}\n"
                   for (t, pv, pi, qv, qi, mx, sk, _) in TABLE)
    out = subprocess.run([cmp_prog], input=rows.encode(), check=True,
                         stdout=subprocess.PIPE).stdout.decode().split()
    assert len(out) == len(TABLE)
    bad = [row for row, got in zip(TABLE, out) if bool(int(got)) != row[-1]]
    assert not bad, bad


def test_numpy_restatement_agrees_with_the_table():
    from ramba_amd.argreduce import better
    npdt = {"f64": np.float64, "f32": np.float32, "i64": np.int64,
            "u8": np.uint8}
    for (t, pv, pi, qv, qi, mx, sk, want) in TABLE:
        conv = float if t[0] == "f" else int
        p = np.asarray(conv(pv), dtype=npdt[t])
        q = np.asarray(conv(qv), dtype=npdt[t])
        got = bool(better(p, np.int64(pi), q, np.int64(qi),
                          "max" if mx else "min", bool(sk)))
        assert got == want, (t, pv, pi, qv, qi, mx, sk)


def test_merge_is_order_independent():
    """Folding any permutation of a pair list gives the same pair — what
    makes the parallel tree deterministic."""
    from itertools import permutations
    from ramba_amd.argreduce import better
    pairs = [(1.0, 4), (np.nan, 9), (3.0, 2), (3.0, 7), (np.nan, 5),
             (0.0, -1)]
    for kind in ("max", "min"):
        for skipna in (False, True):
            seen = set()
            for order in permutations(pairs):
                bv, bi = order[0]
                for (v, i) in order[1:]:
                    if bool(better(np.float64(v), np.int64(i),
                                   np.float64(bv), np.int64(bi), kind,
                                   skipna)):
                        bv, bi = v, i
                seen.add(bi)
            assert len(seen) == 1, (kind, skipna, seen)
            want = 2 if (skipna and kind == "max") else \
                4 if (skipna and kind == "min") else 5
            assert seen == {want}
