"""Integer-array getitem / take on the HIP backend: every branch of the
rt_take_rows kernel (narrow / wide-vector / wide-scalar, 0..3 inner axes,
block boundaries) against NumPy with array_equal, with the host fallback
patched to raise so that the kernel is what ran.
"""

import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):
    from ramba_amd import rowgather

    def boom(*a, **k):
        raise AssertionError("host take fallback reached on the HIP backend")
    for name in ("take_index", "gather_rows", "place_rows"):
        monkeypatch.setattr(rowgather.HostTake, name, boom)


def _src(shape, dtype):
    n = int(np.prod(shape))
    if np.dtype(dtype) == np.bool_:
        return (np.arange(n) % 3 == 0).reshape(shape)
    return (np.arange(n) % 251).astype(dtype).reshape(shape)


def _idx(n_axis, m, seed=0):
    idx = np.random.default_rng(seed).integers(-n_axis, n_axis, size=m)
    if m >= 5:
        idx[1] = idx[0]                 # a duplicate
        idx[2], idx[3] = -1, n_axis - 1   # both ends, one negative
    return idx


def _check(ra, host, index_fn):
    got = index_fn(ra.fromarray(host)).asarray()
    ref = index_fn(host)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert np.array_equal(got, ref)


# -- narrow regime: one thread per element ----------------------------------

@pytest.mark.parametrize("m", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("dtype", ["float64", "int8", "bool"])
def test_narrow_1d(ra_gpu, dtype, m):
    idx = _idx(1000, m)
    _check(ra_gpu, _src((1000,), dtype), lambda a: a[idx])


def test_narrow_two_inner_axes_odd_extent(ra_gpu):
    idx = _idx(64, 40)
    _check(ra_gpu, _src((64, 3, 7), "int16"), lambda a: a[idx])


def test_narrow_three_inner_axes(ra_gpu):
    idx = _idx(5, 9)
    _check(ra_gpu, _src((5, 2, 3, 4), "float32"), lambda a: a[idx])


# -- wide regime ------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 5, 257])
def test_wide_vector_rows(ra_gpu, m):
    idx = _idx(300, m)
    _check(ra_gpu, _src((300, 128), "float64"), lambda a: a[idx])


def test_wide_vector_three_inner_axes(ra_gpu):
    idx = _idx(5, 9)
    _check(ra_gpu, _src((5, 2, 3, 16), "float64"), lambda a: a[idx])


@pytest.mark.parametrize("m", [1, 5, 257])
def test_wide_scalar_unaligned_rows(ra_gpu, m):
    idx = _idx(300, m)
    _check(ra_gpu, _src((300, 130), "float32"), lambda a: a[:, 1:][idx])


def test_wide_scalar_two_inner_axes(ra_gpu):
    idx = _idx(40, 21)
    _check(ra_gpu, _src((40, 3, 50), "int16"), lambda a: a[idx])


def test_indexed_axis_not_first(ra_gpu):
    idx = _idx(300, 77)
    _check(ra_gpu, _src((6, 300), "float64"), lambda a: a[:, idx])


def test_2d_index_and_take(ra_gpu):
    idx = _idx(300, 12).reshape(3, 4)
    _check(ra_gpu, _src((6, 300), "float64"),
           lambda a: a.take(idx, axis=1))


# -- the hooks with explicit position lists (the multi-rank data path) -------

@pytest.mark.parametrize("shape,dtype", [((1000,), "float64"),
                                         ((37, 6), "float64"),
                                         ((300, 128), "float64"),
                                         ((40, 3, 50), "int16")])
def test_gather_then_place_hooks(ra_gpu, shape, dtype):
    import torch
    from ramba_amd import deferred
    ra = ra_gpu
    host = _src(shape, dtype)
    a = ra.fromarray(host)
    out = ra.zeros((50,) + shape[1:], dtype=dtype)
    ra.sync()
    rt = deferred.get_runtime()
    rows = _idx(shape[0], 50, seed=1)
    perm = np.random.default_rng(2).permutation(50)
    dense = rt.backend.gather_rows(a.bdarray, rt,
                                   torch.from_numpy(rows).cuda())
    assert np.array_equal(dense.cpu().numpy(), host[rows])
    rt.backend.place_rows(out.bdarray, rt, torch.from_numpy(perm).cuda(),
                          dense)
    ref = np.zeros((50,) + shape[1:], dtype=dtype)
    ref[perm] = host[rows]
    assert np.array_equal(out.asarray(), ref)


# -- validation happens before any launch ------------------------------------

def test_out_of_range_raises_without_a_launch(ra_gpu, monkeypatch):
    from ramba_amd import deferred
    be = deferred.get_runtime().backend
    a = ra_gpu.fromarray(_src((1000,), "float64"))

    def boom(*args, **kw):
        raise AssertionError("gather launched for an invalid index")
    monkeypatch.setattr(be, "gather_rows", boom)
    monkeypatch.setattr(be, "place_rows", boom)
    with pytest.raises(IndexError) as e:
        a[np.array([0, 1000, 5])]
    assert str(e.value) == "index 1000 is out of bounds for axis 0 with size 1000"
    with pytest.raises(IndexError):
        a[np.array([-1001])]


# -- two ranks on one GPU over gloo -------------------------------------------

WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np
import ramba_amd as ra
from ramba_amd import rowgather

def boom(*a, **k):
    raise AssertionError("host take fallback reached on the HIP backend")
for name in ("take_index", "gather_rows", "place_rows"):
    setattr(rowgather.HostTake, name, boom)
ra.init()   # HIP product backend

def impl(np_):
{body}

res = impl(ra).asarray()
ref = impl(np)
assert res.shape == ref.shape and res.dtype == ref.dtype
assert np.array_equal(res, ref), f"rank {{os.environ['RANK']}}: mismatch"
print("RANK", os.environ["RANK"], "OK")
"""

_PORT_COUNTER = [0]


def run_spmd_gpu(body_src, world=2):
    body = textwrap.indent(textwrap.dedent(body_src).strip(), "    ")
    script = WORKER.format(root=ROOT, body=body)
    _PORT_COUNTER[0] += 1
    port = str(21000 + (os.getpid() * 7 + _PORT_COUNTER[0] * 13) % 2000)
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update({"RANK": str(r), "WORLD_SIZE": str(world),
                    "LOCAL_RANK": "0", "RAMBA_PG_BACKEND": "gloo",
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port,
                    "GLOO_SOCKET_IFNAME": env.get("GLOO_SOCKET_IFNAME",
                                                  "lo")})
        procs.append(subprocess.Popen(
            [sys.executable, "-c", script], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    ok = True
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
            ok = False
        outs.append(out.decode())
        ok = ok and p.returncode == 0
    assert ok, "\n==== rank outputs ====\n" + "\n----\n".join(outs)


def test_rows_2rank_gpu():
    run_spmd_gpu("""
        a = np_.arange(37 * 6).reshape(37, 6) * 1.5
        idx = np.random.default_rng(0).integers(-37, 37, size=50)
        return a[idx]
    """)
