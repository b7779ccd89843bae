"""argmax / argmin / nanargmax / nanargmin over several CPU ranks (gloo,
worlds 2 and 4): the pair exchange plan of runtime.arg_reduce_op on the
oracle backend with the portable host hooks.  Every comparison is
array_equal with equal dtype and shape.
"""

import os
import subprocess
import sys
import textwrap

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np
import ramba_amd as ra
from oracle.numpy_backend import NumpyBackend

ra.init(backend=NumpyBackend())

def impl(np_):
{body}

def as_list(res):
    res = res if isinstance(res, (list, tuple)) else [res]
    return [np.asarray(r.asarray() if hasattr(r, "asarray") else r)
            for r in res]

expect_error = {expect_error!r}
if expect_error:
    for leg in (ra, np):
        try:
            impl(leg)
        except ValueError as e:
            assert expect_error == str(e), str(e)
        else:
            raise AssertionError("no ValueError raised")
    # the ranks must still be in step after the collective decision
    assert int(ra.arange(10).sum()) == 45
else:
    got, ref = as_list(impl(ra)), as_list(impl(np))
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype == np.int64, \
            (k, g.shape, r.shape, g.dtype, r.dtype)
        assert np.array_equal(g, r), \
            f"rank {{os.environ['RANK']}} result {{k}}: {{g}} != {{r}}"
print("RANK", os.environ["RANK"], "OK")
"""

_PORT_COUNTER = [0]


def _next_port(base=25500):
    _PORT_COUNTER[0] += 1
    return str(base + (os.getpid() * 7 + _PORT_COUNTER[0] * 13) % 2000)


def run_spmd(body_src, world=2, expect_error=None):
    body = textwrap.indent(textwrap.dedent(body_src).strip(), "    ")
    script = WORKER.format(root=ROOT, body=body, expect_error=expect_error)
    port = _next_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update({"RANK": str(r), "WORLD_SIZE": str(world),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port,
                    "GLOO_SOCKET_IFNAME": env.get("GLOO_SOCKET_IFNAME", "lo")})
        procs.append(subprocess.Popen(
            [sys.executable, "-c", script], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    ok = True
    for p in procs:
        try:
            out, _ = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
            ok = False
        outs.append(out.decode())
        ok = ok and p.returncode == 0
    assert ok, "\n==== rank outputs ====\n" + "\n----\n".join(outs)
    for r, out in enumerate(outs):
        assert f"RANK {r} OK" in out, out


WORLDS = pytest.mark.parametrize("world", [2, 4])


@WORLDS
def test_flat_and_axis_1d_2d(world):
    # (40, 44) at world 4 is a 2x2 grid: either reduced axis is split
    run_spmd("""
        rng = np.random.default_rng(0)
        h1 = rng.integers(-3, 4, size=1001).astype(np.float64)
        h2 = rng.integers(-3, 4, size=(40, 44)).astype(np.float32)
        h2[7, 9] = np.nan
        a1, a2 = np_.array(h1), np_.array(h2)
        out = []
        for fn in ("argmax", "argmin", "nanargmax", "nanargmin"):
            f = getattr(np_, fn)
            out += [f(a1), f(a1[::-1]), f(a1[5::3]), f(a2), f(a2.T),
                    f(a2, axis=0), f(a2, axis=1), f(a2.T, axis=0),
                    f(a2, axis=1, keepdims=True), f(a2[::-1, 3:], axis=0)]
        return out
    """, world=world)


@WORLDS
def test_integer_dtypes_and_3d(world):
    run_spmd("""
        rng = np.random.default_rng(1)
        h = rng.integers(-100, 100, size=(6, 10, 12)).astype(np.int8)
        big = np.array([2**62, 2**62 + 1] * 50, dtype=np.int64)
        a, b = np_.array(h), np_.array(big)
        out = [np_.argmax(b), np_.argmin(b), np_.argmax(b[::-1])]
        for axis in (None, 0, 1, 2):
            out += [np_.argmax(a, axis=axis), np_.argmin(a, axis=axis),
                    np_.argmax(a.transpose(2, 0, 1), axis=axis)]
        m = np_.array(h > 50)
        return out + [np_.argmax(m), np_.argmin(m, axis=1)]
    """, world=world)


@WORLDS
def test_all_equal_gives_zero(world):
    # every rank holds the same extreme: rank 0's first element must win
    run_spmd("""
        a = np_.ones(1001)
        b = np_.ones((40, 44))
        return [np_.argmax(a), np_.argmin(a), np_.argmax(b),
                np_.argmax(b, axis=0), np_.argmin(b, axis=1)]
    """, world=world)


@WORLDS
def test_nan_on_last_rank_beats_max_on_rank_zero(world):
    run_spmd("""
        h = np.zeros(1001)
        h[3] = 1e300            # rank 0
        h[1000] = np.nan        # last rank
        a = np_.array(h)
        g = np.zeros((40, 44))
        g[0, :] = 9.0
        g[39, 5] = np.nan
        b = np_.array(g)
        return [np_.argmax(a), np_.argmin(a), np_.nanargmax(a),
                np_.nanargmin(a), np_.argmax(b), np_.argmax(b, axis=0),
                np_.nanargmax(b, axis=0)]
    """, world=world)


@WORLDS
def test_same_maximum_on_two_ranks_lower_index_wins(world):
    run_spmd("""
        h = np.zeros(1001)
        h[10] = h[990] = 5.0
        h[20] = h[980] = -5.0
        a = np_.array(h)
        g = np.zeros((40, 44))
        g[2, 1] = g[38, 1] = g[2, 40] = 7.0
        b = np_.array(g)
        return [np_.argmax(a), np_.argmin(a), np_.argmax(a[::-1]),
                np_.argmax(b), np_.argmax(b, axis=0), np_.argmax(b, axis=1),
                np_.argmax(b.T)]
    """, world=world)


def test_fewer_elements_than_ranks():
    # n = 3 at world 4: some ranks have empty shards
    run_spmd("""
        a = np_.array(np.array([2.0, 7.0, 7.0]))
        b = np_.array(np.array([[1, 5, 5], [9, 0, 9], [9, 5, 1]]))
        return [np_.argmax(a), np_.argmin(a), np_.argmax(b),
                np_.argmax(b, axis=0), np_.argmin(b, axis=1)]
    """, world=4)


@WORLDS
def test_all_nan_line_raises_on_every_rank(world):
    run_spmd("""
        g = np.ones((40, 44))
        g[:, 43] = np.nan        # one all-NaN column, on the last rank(s)
        return np_.nanargmax(np_.array(g), axis=0)
    """, world=world, expect_error="All-NaN slice encountered")


@WORLDS
def test_all_nan_flat_raises_on_every_rank(world):
    run_spmd("""
        return np_.nanargmin(np_.array(np.full(1001, np.nan)))
    """, world=world, expect_error="All-NaN slice encountered")
