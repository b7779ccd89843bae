"""Integer-array getitem / take over several CPU ranks (gloo, worlds 2 and
4): the request/reply row exchange of runtime.take_op on the oracle backend
with the portable host hooks.  Every comparison is array_equal.
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

expect_error = {expect_error!r}
if expect_error:
    for leg in (ra, np):
        try:
            impl(leg)
        except IndexError as e:
            assert expect_error in str(e), str(e)
        else:
            raise AssertionError("no IndexError raised")
    # the ranks must still be in step after the collective decision
    assert int(ra.arange(10).sum()) == 45
else:
    res = impl(ra)
    if hasattr(res, "asarray"):
        res = res.asarray()
    ref = impl(np)
    assert res.shape == ref.shape and res.dtype == ref.dtype, \
        (res.shape, ref.shape, res.dtype, ref.dtype)
    assert np.array_equal(res, ref), \
        f"rank {{os.environ['RANK']}}: {{res}} != {{ref}}"
print("RANK", os.environ["RANK"], "OK")
"""

_PORT_COUNTER = [0]


def _next_port(base=23500):
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
def test_permutation_1d(world):
    run_spmd("""
        a = np_.arange(1001) * 0.5
        perm = np.random.default_rng(0).permutation(1001)
        return a[perm]
    """, world=world)


@WORLDS
def test_all_indices_hit_one_rank(world):
    run_spmd("""
        a = np_.arange(1001) * 0.5
        idx = np.random.default_rng(0).integers(0, 100, size=333)
        return a[idx]
    """, world=world)


@WORLDS
def test_one_rank_never_requested(world):
    # the last rank's rows are never asked for: zero-length messages
    run_spmd("""
        a = np_.arange(1001) * 0.5
        idx = np.random.default_rng(0).integers(0, 1001 // 2 - 1, size=400)
        return a[idx]
    """, world=world)


@WORLDS
def test_rows_negatives_duplicates(world):
    run_spmd("""
        a = np_.arange(37 * 6).reshape(37, 6) * 1.5
        idx = np.random.default_rng(0).integers(-37, 37, size=50)
        return a[idx]
    """, world=world)


@WORLDS
def test_axis1_repartitions_source(world):
    run_spmd("""
        a = np_.fromfunction(lambda i, j: i * 10 + j, (9, 10),
                             dtype=np.int64)
        return a[:, [9, 0, 0, -2, 5]]
    """, world=world)


@WORLDS
def test_default_partition_2d_source(world):
    # a default (possibly 2-D block) partition is repartitioned first
    run_spmd("""
        a = np_.fromfunction(lambda i, j: i * 100 + j, (40, 44),
                             dtype=np.int64)
        return a[[39, 0, 17, 17, -1]]
    """, world=world)


@WORLDS
def test_2d_index(world):
    run_spmd("""
        a = np_.arange(37 * 6).reshape(37, 6)
        idx = np.random.default_rng(0).integers(-37, 37, size=(5, 4))
        return a[idx, 1:]
    """, world=world)


@WORLDS
def test_ramba_index_and_take(world):
    run_spmd("""
        a = np_.arange(300).reshape(50, 6) * 1.0
        idx = (np_.arange(21)[::-1] * 7) % 50
        return np_.take(a, idx.astype(np.int32), axis=0)
    """, world=world)


def test_fewer_rows_than_ranks():
    # shape (3, 4) at world 4 leaves an empty source shard; two indices
    # leave empty index/output shards
    run_spmd("""
        a = np_.arange(12).reshape(3, 4)
        return np_.concatenate([a[[2, 0]], a[[0, 1, 2, 2, 1, 0, -1]]])
    """, world=4)


@WORLDS
def test_out_of_range_raises_on_every_rank(world):
    run_spmd("""
        a = np_.arange(1001) * 0.5
        idx = np.arange(600)
        idx[599] = 1001
        return a[idx]
    """, world=world, expect_error="index 1001 is out of bounds for axis 0 "
                                   "with size 1001")
