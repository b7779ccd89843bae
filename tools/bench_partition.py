"""Time partition / argpartition on one MI355X (HIP events) and write one JSON
line per case to profiles/partition_bench.jsonl.

    python tools/bench_partition.py [--sizes 20,24,27] [--reps 3] [--out PATH]

Cases: n = 2^20, 2^24, 2^27 elements of float32 / float64 / int32, uniform
random and heavily duplicated (16 distinct values), kth = n // 2 and n - 100.
Per case, all on resident device data:
    split_ms         rt_partition alone (keys only) about the pivot that the
                     select found; split_arg_ms the same moving only the
                     generated int64 payload
    partition_ms /   the public ramba_amd calls: select_op, then the split
    argpartition_ms
    sort_ms /        ramba_amd.sort / argsort of the same array, the route a
    argsort_ms       user had before
    torch_ms         the outside yardstick: torch.kthvalue for kth = n // 2,
                     torch.topk(100) for kth = n - 100
    bytes            what the split moves, from the shapes: two reads of the
                     keys and one write; peak_frac = bytes over 8 TB/s over
                     split_ms
    vs_sort, vs_argsort   partition_ms / sort_ms, argpartition_ms / argsort_ms
A timed window holds as many calls as fill about 100 ms; each figure is the
per-call median of `reps` windows after two warm-up calls, and the windows of
the functions of one case alternate.
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sort import PEAK_BYTES_PER_S, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24,27")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "partition_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import ramba_amd as ra
    from ramba_amd import deferred
    ra.init()
    rt = deferred.get_runtime()
    be = rt.backend
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    for log2n in (int(s) for s in args.sizes.split(",")):
        n = 1 << log2n
        for dtype in ("float32", "float64", "int32"):
            tdt = getattr(torch, dtype)
            for dist in ("uniform", "dup16"):
                a = ra.zeros(n, dtype=dtype)
                ra.sync()
                pad = rt.lo_pads(a.bdarray)[0]
                core = be._cont(a.bdarray)[pad:pad + n]
                if dist == "dup16":
                    core.copy_(torch.randint(0, 16, (n,), device="cuda")
                               .to(tdt))
                elif dtype == "int32":
                    core.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (n,),
                                             dtype=tdt, device="cuda"))
                else:
                    core.copy_(torch.rand(n, dtype=tdt, device="cuda") - 0.5)
                a.bdarray.pure = None       # written behind the engine's back
                for kth in (n // 2, n - 100):
                    keys, _, _ = rt.select_op(a, [kth], True)
                    ks = a.dtype.itemsize
                    rec = dict(dtype=dtype, dist=dist, n=n, kth=kth,
                               itemsize=ks, bytes=3 * n * ks)
                    if kth == n // 2:
                        yard = lambda: torch.kthvalue(core, kth + 1)
                    else:
                        yard = lambda: torch.topk(core, n - kth)
                    fns = dict(
                        split_ms=lambda: be.split_run(core, None, 0, keys,
                                                      True, False, False),
                        split_arg_ms=lambda: be.split_run(core, None, 0, keys,
                                                          False, True, False),
                        partition_ms=lambda: ra.partition(a, kth),
                        argpartition_ms=lambda: ra.argpartition(a, kth),
                        sort_ms=lambda: ra.sort(a),
                        argsort_ms=lambda: ra.argsort(a),
                        torch_ms=yard)
                    ms, calls = timed_alternating(torch, list(fns.values()),
                                                  args.reps)
                    rec.update(zip(fns, ms))
                    rec["calls"] = dict(zip(fns, calls))
                    rec["peak_frac"] = rec["bytes"] / PEAK_BYTES_PER_S * 1e3 \
                        / rec["split_ms"]
                    rec["vs_sort"] = rec["partition_ms"] / rec["sort_ms"]
                    rec["vs_argsort"] = rec["argpartition_ms"] \
                        / rec["argsort_ms"]
                    print(json.dumps(rec), flush=True)
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
                del a, core
    out.close()


if __name__ == "__main__":
    main()
