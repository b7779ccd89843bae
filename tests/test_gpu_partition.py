"""partition / argpartition on the HIP backend: rt_partition behind
runtime.partition_op, through the public functions, with the host fallback
taken away.  The flat path is compared exactly (values by their bits) with
the stable split restated in NumPy; the paths that sort are held to NumPy's
partition contract."""

import importlib

import numpy as np
import pytest

from test_gpu_sort import DTYPES, bits, hostile, ties
from test_partition_frontend import contract, expected_argpartition

pytestmark = pytest.mark.gpu

SIZES = ["1", "2", "63", "64", "65", "tile-1", "tile", "tile+1", "2*tile+3"]


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):      # reaching the host hooks is a TypeError
    for mod, cls, hooks in (("sorting", "HostSort", ("split_run", "local_run",
                                                     "sort_run", "sort_lines")),
                            ("selection", "HostSelect", ("select_pass",))):
        for hook in hooks:
            monkeypatch.setattr(
                getattr(importlib.import_module("ramba_amd." + mod), cls),
                hook, None)


@pytest.fixture(scope="module")
def geo():
    from ramba_amd import hip_backend as hb
    return hb.partition_geometry(hb._load_lib())


def check(ra, host, kth, view=lambda x: x, **kw):
    a, h = view(ra.fromarray(host)), view(host).reshape(-1)
    idx = expected_argpartition(h, kth)
    got = ra.partition(a, kth, **kw).asarray()
    assert got.dtype == h.dtype and got.shape == h.shape
    assert np.array_equal(bits(got), bits(h[idx])), (h.dtype, h.size, kth)
    got = ra.argpartition(a, kth, **kw).asarray()
    assert got.dtype == np.int64 and np.array_equal(got, idx), \
        (h.dtype, h.size, kth)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_dtypes_and_data(ra_gpu, geo, n, dtype):
    n = eval(n, {"tile": geo["tile"]})
    perm = np.random.default_rng(n).permutation(n)
    data = [ties(n, dtype), np.full(n, 1).astype(dtype),
            (perm % 2 if dtype == "bool" else perm % 251 - 125).astype(dtype)]
    if dtype != "bool":
        data.append(hostile(dtype, n))
    for host in data:
        for kth in sorted({0, n // 2, n - 1}) + [-1]:
            check(ra_gpu, host, kth)
        check(ra_gpu, host, [n // 3, -1, n // 2])


@pytest.mark.parametrize("npiv", [2, 4, 5, 8])
def test_every_packed_word_class(ra_gpu, geo, npiv):
    n = 2 * geo["tile"] + 3
    host = np.random.default_rng(npiv).permutation(n).astype(np.float32)
    host[::5] = np.nan              # the last pivot is the NaN key
    check(ra_gpu, host, [(i * n) // npiv + 7 for i in range(npiv - 1)] + [-1])


def test_three_tiles_per_block_and_a_ragged_tail(ra_gpu, geo):
    n = 2 * geo["grid_cap"] * geo["tile"] + 1
    check(ra_gpu, ties(n, "int32"), n // 2)


def test_views(ra_gpu):
    check(ra_gpu, ties((41, 67), "float64"), 1000, lambda x: x.T, axis=None)
    check(ra_gpu, ties(301, "int16"), [5, 150], lambda x: x[::-1])


@pytest.mark.parametrize("axis", [0, 1])
def test_lines_and_nine_kth_meet_numpys_contract(ra_gpu, axis):
    h = ties((41, 67), "float32")
    h[::7, ::3] = np.nan
    a = ra_gpu.fromarray(h)
    contract(ra_gpu.partition(a, [3, 20], axis=axis).asarray(), h, [3, 20],
             axis)
    idx = ra_gpu.argpartition(a, 11, axis=axis).asarray()
    contract(np.take_along_axis(h, idx, axis), h, [11], axis)
    nine, flat = list(range(0, 2700, 300)), ties(2747, "int16")
    contract(ra_gpu.partition(ra_gpu.fromarray(flat), nine).asarray(), flat,
             nine, 0)
