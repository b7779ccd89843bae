"""bench.py --dump-outputs / --full: the sampler on the CPU oracle backend,
and one small end-to-end run of the flagship on the HIP path."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

import bench  # noqa: E402  (conftest puts the repo root on sys.path)


def _rng():
    return np.random.default_rng(bench.DUMP_SEED)


def test_sample_small_array_is_whole(ra):
    x = ra.arange(1000) / 8.0
    got = bench.sample_output(x, 8000, _rng())
    assert got.dtype == np.float64
    assert np.array_equal(got, np.arange(1000) / 8.0)


def test_sample_scalar_and_int(ra):
    got = bench.sample_output(2.5, 100, _rng())
    assert got.dtype == np.float64 and got.shape == () and got == 2.5
    got = bench.sample_output(ra.arange(10), 1000, _rng())
    assert got.dtype == np.float64
    assert np.array_equal(got, np.arange(10.0))


@pytest.mark.parametrize("n", [1001, 4096, 100_003])
def test_sample_large_1d(ra, n):
    budget = 800                                  # 100 fp64 elements
    x = ra.arange(n) * 0.5
    got = bench.sample_output(x, budget, _rng())
    again = bench.sample_output(x, budget, _rng())
    assert np.array_equal(got, again)             # same elements every run
    assert got.nbytes <= budget
    # head, strided middle, tail -- rebuilt here from the documented rule
    ref = np.arange(n) * 0.5
    edge = 100 // 8
    stride = -(-n // (100 - 2 * edge))
    off = int(_rng().integers(stride))
    want = np.concatenate([ref[:edge], ref[off::stride], ref[n - edge:]])
    assert np.array_equal(got, want)


def test_sample_large_2d_rows(ra):
    x = ra.fromfunction(lambda i, j: i * 7 + j, (67, 7), dtype=np.float32)
    ref = np.fromfunction(lambda i, j: i * 7 + j, (67, 7), dtype=np.float32)
    budget = 24 * 7 * 4                           # 24 rows
    got = bench.sample_output(x, budget, _rng())
    assert got.dtype == np.float32 and got.shape[1] == 7
    assert got.nbytes <= budget
    edge = 3
    stride = -(-67 // (24 - 2 * edge))
    off = int(_rng().integers(stride))
    want = np.concatenate([ref[:edge], ref[off::stride], ref[67 - edge:]])
    assert np.array_equal(got, want)


def test_sample_row_over_budget_is_an_error(ra):
    x = ra.zeros((4, 100), dtype=np.float64)
    with pytest.raises(ValueError):
        bench.sample_output(x, 1600, _rng())


@pytest.mark.gpu
def test_bench_dump_outputs_flagship(tmp_path):
    n = (1 << 20) + 37
    env = dict(os.environ, RAMBA_WARMUP_FLOOR="0")
    p = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--elems", str(n),
         "--dump-outputs", str(tmp_path / "dump")],
        env=env, capture_output=True, timeout=240)
    out = p.stdout.decode()
    assert p.returncode == 0, out + p.stderr.decode()
    line = json.loads(out.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "GElem/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["ms_per_step"] > 0
    assert abs(line["value"] - n / line["ms_per_step"] / 1e6) \
        <= 1e-9 * line["value"]
    # the legs behind --full stay out of a plain run
    assert line["roofline"] is None and line["cpu_baseline"] is None
    a = np.arange(n, dtype=np.float64) / 1000.0
    want = {"B": np.sin(a), "C": np.cos(a)}
    want["D"] = want["B"] * want["B"] + want["C"] ** 2
    assert sorted(os.listdir(tmp_path / "dump")) == ["B.npy", "C.npy", "D.npy"]
    for name, ref in want.items():
        got = np.load(tmp_path / "dump" / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == (n,)
        # smoke()'s tolerance for the same chain
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
