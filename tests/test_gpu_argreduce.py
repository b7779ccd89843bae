"""argmax / argmin / nanargmax / nanargmin on the HIP backend: every regime
of the rt_arg_* kernels (flat 16-byte and scalar loads, one and several
grid-stride trips, wave-per-line, thread-per-output, chunked, pair combine)
against NumPy with array_equal, with the host fallback patched to raise so
that the kernels are what ran.  A second reference, the two-pass where/min
composition on the same device data, checks three float shapes, and two
ranks on one GPU exercise the cross-rank pair exchange.
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

PATCH = """
from ramba_amd import argreduce as _ar
def _boom(*a, **k):
    raise AssertionError("host arg-reduction fallback reached on HIP")
_ar.HostArg.arg_reduce_partial = _boom
_ar.HostArg.arg_combine_box = _boom
"""


@pytest.fixture(autouse=True)
def no_host_fallback(monkeypatch):
    from ramba_amd import argreduce

    def boom(*a, **k):
        raise AssertionError("host arg-reduction fallback reached on HIP")
    for name in ("arg_reduce_partial", "arg_combine_box"):
        monkeypatch.setattr(argreduce.HostArg, name, boom)


def _same(got, ref, what=""):
    if hasattr(got, "asarray"):
        got = got.asarray()
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.int64, (what, got.dtype, ref.dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, got, ref)


def _both(ra, host, fn, view=lambda x: x, what="", **kw):
    _same(getattr(ra, fn)(view(ra.fromarray(host)), **kw),
          getattr(np, fn)(view(host), **kw), (what, fn, kw))


def _grid_cap():
    from ramba_amd import hip_backend
    return hip_backend._load_lib().rt_arg_grid_cap()


def _two_trip_size(dtype):
    """Elements that give every stage-1 block of the 16-byte path two full
    grid-stride trips, half of them a third, and a scalar tail."""
    per = 16 // np.dtype(dtype).itemsize
    return _grid_cap() * 256 * per * 5 // 2 + per + 1


# -- flat ----------------------------------------------------------------------

def _base(n, dtype, kind):
    """A body of middling values with ties; (body, extreme value)."""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return (np.zeros(n, bool), True) if kind == "max" \
            else (np.ones(n, bool), False)
    body = (np.arange(n) * 7 % 5 + 1).astype(dt)
    return body, dt.type(9 if kind == "max" else -9)


def _flat_cases(n, dtype):
    """(name, host array, function names) for one size."""
    out = []
    for kind in ("max", "min"):
        fns = ("arg" + kind, "nanarg" + kind)
        body, ext = _base(n, dtype, kind)
        for name, pos in (("first", [0]), ("last", [n - 1]),
                          ("tie63/64", [63, 64]), ("tie255/256", [255, 256]),
                          ("tie-two-blocks", [7, n - 9]),
                          ("tie-mid", [n // 3, n // 3 + n // 2])):
            if max(pos) >= n or min(pos) < 0 or len(set(pos)) != len(pos):
                continue
            x = body.copy()
            x[pos] = ext
            out.append((f"{kind}-{name}", x, fns))
        out.append((f"{kind}-all-equal", np.full(n, ext, dtype=dtype), fns))
    if np.dtype(dtype).kind == "f":
        body, ext = _base(n, dtype, "max")
        if n >= 3:
            x = body.copy()
            x[0] = ext
            x[n - 1] = np.nan               # one NaN after the maximum
            out.append(("nan-after-max", x,
                        ("argmax", "argmin", "nanargmax", "nanargmin")))
        if n >= 20:
            x = body.copy()
            x[n // 2] = ext
            x[[n // 3, n - 2]] = np.nan     # two NaNs, far apart
            out.append(("two-nans", x,
                        ("argmax", "argmin", "nanargmax", "nanargmin")))
    return out


def _check_flat(ra, n, dtype, view=lambda a: a):
    for name, x, fns in _flat_cases(n, dtype):
        a = view(ra.fromarray(x))
        for fn in fns:
            _same(getattr(a, fn)(), getattr(np, fn)(view(x)),
                  (n, dtype, name, fn))


@pytest.mark.parametrize("dtype", ["float64", "int64", "bool"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_flat_sizes(ra_gpu, n, dtype):
    _check_flat(ra_gpu, n, dtype)
    for view in (lambda a: a[::-1], lambda a: a[::3]):
        _check_flat(ra_gpu, n, dtype, view)


@pytest.mark.parametrize("dtype", ["float64", "int64"])
def test_flat_two_grid_stride_trips_vector_path(ra_gpu, dtype):
    from ramba_amd import deferred, hip_backend
    n = _two_trip_size(dtype)
    assert n <= 4_000_000
    per = 16 // np.dtype(dtype).itemsize
    assert n // per >= 2 * _grid_cap() * 256 and n % per
    _check_flat(ra_gpu, n, dtype)
    # and the path taken really is the 16-byte one
    a = ra_gpu.fromarray(np.zeros(n, dtype=dtype))
    rt = deferred.get_runtime()
    cont = rt.backend._cont(a.bdarray)
    _, _, cstr, pads = rt.shard_geometry(a.bdarray)
    i64 = hip_backend._i64arr
    import ctypes
    assert rt.backend.lib.rt_arg_flat_regime(
        ctypes.c_void_p(cont.data_ptr()), pads[0], 1, i64([n]), i64([1]),
        hip_backend._DT_ENUM[dtype]) == 1


def test_flat_two_grid_stride_trips_scalar_path_bool(ra_gpu):
    # an offset view is not 16-byte aligned: one element per lane and trip
    n = _grid_cap() * 256 * 5 // 2 + 3
    assert n <= 4_000_000
    _check_flat(ra_gpu, n + 1, "bool", lambda a: a[1:])
    _check_flat(ra_gpu, n, "float64", lambda a: a[::-1])


@pytest.mark.parametrize("dtype", ["float64", "int64", "bool", "float32",
                                   "int8"])
def test_flat_views_of_2d(ra_gpu, dtype):
    rng = np.random.default_rng(3)
    if dtype == "bool":
        h = rng.integers(0, 2, size=(33, 65)).astype(bool)
    else:
        h = rng.integers(-3, 4, size=(33, 65)).astype(dtype)
    for fn in ("argmax", "argmin"):
        for view in (lambda a: a, lambda a: a.T, lambda a: a[::-1],
                     lambda a: a[:, ::3], lambda a: a[:, 1:]):
            _both(ra_gpu, h, fn, view)
    h = np.zeros((33, 65), dtype=dtype)
    h[20, 40] = 1                           # a unique extreme: view order
    _both(ra_gpu, h, "argmax", lambda a: a.T)
    _both(ra_gpu, h, "argmax", lambda a: a[::-1, ::-1])


def test_flat_vector_path_nd(ra_gpu):
    # innermost extent a whole number of 16-byte units: the N-D unit decode
    rng = np.random.default_rng(4)
    for shape, dtype in (((33, 64), "float64"), ((5, 6, 32), "float32"),
                         ((2, 3, 4, 48), "bool"), ((9, 16), "int8")):
        h = rng.integers(0, 2, size=shape).astype(dtype)
        for fn in ("argmax", "argmin"):
            _both(ra_gpu, h, fn)
        h = np.zeros(shape, dtype=dtype)
        h[tuple(s - 1 for s in shape)] = 1
        _both(ra_gpu, h, "argmax")
        h[tuple(s // 2 for s in shape)] = 1
        _both(ra_gpu, h, "argmax")


def test_int64_beyond_double_precision(ra_gpu):
    h = np.array([2**62, 2**62 + 1] * 40, dtype=np.int64)
    assert int(ra_gpu.argmax(ra_gpu.fromarray(h))) == 1
    assert int(ra_gpu.argmin(ra_gpu.fromarray(h[::-1].copy()))) == 1
    _both(ra_gpu, h.reshape(2, 40), "argmax", axis=0)
    _both(ra_gpu, h.reshape(40, 2), "argmax", axis=1)


# -- one axis --------------------------------------------------------------------

def _axis_data(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "bool":
        return rng.integers(0, 2, size=shape).astype(bool)
    h = rng.integers(-3, 4, size=shape).astype(dtype)
    if np.dtype(dtype).kind == "f":
        flat = h.reshape(-1)
        flat[rng.integers(0, flat.size, size=max(1, flat.size // 40))] = \
            np.nan
    return h


AXIS_CASES = [((7, 130), 1), ((130, 7), 0), ((3, 5, 4), 1),
              ((2, 3, 4, 5), 0), ((2, 3, 4, 5), 1), ((2, 3, 4, 5), 2),
              ((2, 3, 4, 5), 3), ((7, 130), 0), ((130, 7), 1)]


@pytest.mark.parametrize("dtype", ["float64", "float32", "int64", "int16",
                                   "bool"])
@pytest.mark.parametrize("shape,axis", AXIS_CASES)
def test_axis_shapes(ra_gpu, shape, axis, dtype):
    h = _axis_data(shape, dtype, seed=len(shape) * 10 + axis)
    for fn in ("argmax", "argmin"):
        _both(ra_gpu, h, fn, axis=axis)
    if np.dtype(dtype).kind == "f":
        g = np.where(np.isnan(h), 0.5, h)
        g.reshape(-1)[3] = np.nan           # NaN lines are never complete
        for fn in ("nanargmax", "nanargmin"):
            _both(ra_gpu, g.astype(dtype), fn, axis=axis)


@pytest.mark.parametrize("shape,dtype", [((5, 1103), "float64"),
                                         ((3, 2111), "float32"),
                                         ((4, 5003), "int8"),
                                         ((3, 1040), "bool"),
                                         ((2, 700), "int64")])
def test_axis_long_lines_wave_regime(ra_gpu, shape, dtype):
    # lines long enough for the four-loads-in-flight loop: 16-byte units
    # with a scalar tail on the whole array, single elements on an offset
    # or reversed view
    h = _axis_data(shape, dtype, seed=shape[1])
    h[1, shape[1] - 1] = np.nanmax(h)       # an extreme in the tail
    h[0, 300] = h[0, 17] = np.nanmax(h)     # a tie inside one line
    for fn in ("argmax", "argmin"):
        _both(ra_gpu, h, fn, axis=1)
        _both(ra_gpu, h, fn, lambda a: a[:, 1:], axis=1)
        _both(ra_gpu, h, fn, lambda a: a[:, ::-1], axis=1)
    if np.dtype(dtype).kind == "f":
        _both(ra_gpu, h, "nanargmax", axis=1)


def test_axis_keepdims_negative_axis_and_views(ra_gpu):
    h = _axis_data((7, 130), "float64", seed=1)
    _both(ra_gpu, h, "argmax", axis=1, keepdims=True)
    _both(ra_gpu, h, "argmin", axis=-2, keepdims=True)
    _both(ra_gpu, h, "argmax", lambda a: a.T, axis=0)
    _both(ra_gpu, h, "argmax", lambda a: a[::-1, ::2], axis=1)
    g = _axis_data((3, 5, 4), "int64", seed=2)
    _both(ra_gpu, g, "argmin", lambda a: a.transpose(2, 0, 1), axis=2)


def test_axis_chunked_regime_tie_and_nan_in_different_chunks(ra_gpu):
    from ramba_amd.hip_backend import _hb_arg_chunks
    assert _hb_arg_chunks(2, 0, 3, 5000) > 1      # the regime under test
    assert _hb_arg_chunks(2, 0, 7, 130) == 1
    h = (np.arange(15000) * 7 % 5 + 1.0).reshape(5000, 3)
    h[[10, 4000], 0] = 9.0          # a tie across chunks: 10 wins
    h[100, 1] = 9.0
    h[3000, 1] = np.nan             # a NaN in a later chunk beats it
    h[[4999, 2], 2] = -9.0
    for fn in ("argmax", "argmin", "nanargmax", "nanargmin"):
        _both(ra_gpu, h, fn, axis=0)
    assert ra_gpu.argmax(ra_gpu.fromarray(h), axis=0).asarray().tolist() \
        == [10, 3000, 0]
    _both(ra_gpu, np.nan_to_num(h).astype(np.int64), "argmax", axis=0)
    # one output element, K not a multiple of the chunk length
    _both(ra_gpu, h[:4099, :1].copy(), "argmin", axis=0)


def test_all_nan_line_raises_and_leaves_the_backend_usable(ra_gpu):
    h = np.ones((7, 130))
    h[4, :] = np.nan
    a = ra_gpu.fromarray(h)
    with pytest.raises(ValueError, match="All-NaN slice encountered"):
        ra_gpu.nanargmax(a, axis=1)
    with pytest.raises(ValueError, match="All-NaN slice encountered"):
        ra_gpu.nanargmin(ra_gpu.fromarray(np.full(300, np.nan)))
    _both(ra_gpu, h, "nanargmax", axis=0)
    _both(ra_gpu, h, "argmax", axis=1)


# -- second reference: the two-pass where/min composition -------------------------

def _composed_argmax(ra, a, axis):
    n = a.shape[axis]
    sh = [1] * a.ndim
    sh[axis] = n
    m = a.max(axis=axis, keepdims=True)
    j = ra.arange(n).reshape(tuple(sh))
    hit = (a == m) | (ra.isnan(a) & ra.isnan(m))
    return ra.where(hit, j, n).min(axis=axis)


@pytest.mark.parametrize("shape,axis", [((7, 130), 1), ((130, 7), 0),
                                        ((5000, 3), 0)])
def test_against_where_min_composition_on_device(ra_gpu, shape, axis):
    h = _axis_data(shape, "float64", seed=7)
    a = ra_gpu.fromarray(h)
    got = ra_gpu.argmax(a, axis=axis).asarray()
    comp = _composed_argmax(ra_gpu, a, axis).asarray()
    assert got.shape == comp.shape and np.array_equal(got, comp)
    assert np.array_equal(got, np.argmax(h, axis=axis))


# -- two ranks on one GPU (gloo transport) ------------------------------------------

WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np
import ramba_amd as ra
{patch}
ra.init()   # HIP product backend

def impl(np_):
{body}

got, ref = impl(ra), impl(np)
assert len(got) == len(ref)
for k, (g, r) in enumerate(zip(got, ref)):
    g = np.asarray(g.asarray() if hasattr(g, "asarray") else g)
    r = np.asarray(r)
    assert g.dtype == r.dtype == np.int64 and g.shape == r.shape, (k, g, r)
    assert np.array_equal(g, r), f"rank {{os.environ['RANK']}} #{{k}}: " \
        f"{{g}} != {{r}}"
print("RANK", os.environ["RANK"], "OK")
"""


def run_spmd_gpu(body_src, world=2):
    body = textwrap.indent(textwrap.dedent(body_src).strip(), "    ")
    script = WORKER.format(root=ROOT, body=body, patch=PATCH)
    port = str(29000 + (os.getpid() * 7) % 2000)
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
    for r, out in enumerate(outs):
        assert f"RANK {r} OK" in out, out


def test_two_ranks_one_gpu():
    run_spmd_gpu("""
        h = (np.arange(1001) * 7 % 5 + 1.0)
        h[10] = h[990] = 9.0             # a cross-rank tie: 10 wins
        h[995] = np.nan                  # ... unless a NaN is on rank 1
        g = (np.arange(53 * 71) * 7 % 5 + 1.0).reshape(53, 71)
        g[2, 1] = g[50, 1] = g[2, 60] = 9.0
        g[51, 5] = np.nan
        a, b = np_.array(h), np_.array(g)
        return [np_.argmax(a), np_.nanargmax(a), np_.argmin(a[::-1]),
                np_.argmax(b), np_.nanargmax(b.T),
                np_.argmax(b, axis=0), np_.argmax(b, axis=1),
                np_.nanargmax(b, axis=0), np_.argmin(b, axis=1,
                                                     keepdims=True),
                np_.argmax(np_.array(np.nan_to_num(g).astype(np.int64)),
                           axis=0)]
    """)
