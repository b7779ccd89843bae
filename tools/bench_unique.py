"""Time unique and searchsorted on one MI355X (HIP events) and write one JSON
line per case to profiles/unique_bench.jsonl.

    python tools/bench_unique.py [--sizes 1000000,10000000,100000000]
                                 [--needles 100000000] [--reps 3] [--out PATH]

unique cases: n elements of float64 / int32 with few (256), many (n / 16)
and all-distinct values.  Per case, RESIDENT-BUFFER times (HIP events
around the backend hook; NOT a kernel trace): `compact_ms`, the
rt_unique_count + rt_unique_write pair on the already sorted run with all
three outputs, which holds the pair's one stream synchronisation, its 8-byte
read-back and torch's allocation of the outputs besides the five kernels;
`sort_ms`, rt_sort of the same data, keys with the int64 payload; `torch_ms`,
torch.unique(sorted=True, return_counts=True) on the same device data.
Before timing, the pair's values and counts are compared with torch.unique's
at the timed size.
END-TO-END times through the public functions: `unique_call_ms`,
ramba_amd.unique(a, return_index=True, return_counts=True); `sort_call_ms`,
ramba_amd.argsort(a), the sort alone on the same data, so that their
difference is the compaction's added cost; `host_ms`, the round trip a user
had before (asarray -> np.unique -> fromarray), timed once.  `bytes`: what
the compaction must move (two reads of the keys, U payload reads, U writes
of key, first and start, and the in-place difference); `peak_frac` = bytes
over 8 TB/s over compact_ms.

searchsorted cases: `needles` float64 needles against m = 10^3, 10^5 and
10^7 sorted keys, side left.  KERNEL (one launch between HIP events, no
synchronisation or allocation inside): `kernel_ms`, rt_searchsorted alone;
`torch_ms`, torch.searchsorted on the same tensors; `roofline_ms`, the
needles' read plus the int64 results' write at 8 TB/s.  END TO END:
`call_ms`, ramba_amd.searchsorted.

A timed window holds as many calls as fill about 100 ms; the windows of the
figures compared alternate, and each figure is the per-call median of `reps`
windows after two warm-up calls.
"""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sort import PEAK_BYTES_PER_S, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000,100000000")
    ap.add_argument("--needles", type=int, default=10 ** 8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "unique_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import ramba_amd as ra
    from ramba_amd import deferred
    from ramba_amd.hip_backend import RT_DTYPE, _i64arr
    ra.init()
    rt = deferred.get_runtime()
    be = rt.backend
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def device_array(n, dtype, fill):
        """A 1-D ramba array whose container core is filled on the device."""
        a = ra.zeros(n, dtype=dtype)
        ra.sync()
        pad = rt.lo_pads(a.bdarray)[0]
        core = be._cont(a.bdarray)[pad:pad + n]
        core.copy_(fill)
        a.bdarray.pure = None       # no longer the zeros a kernel may recompute
        return a, core

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    def run_unique(n, dtype, dist):
        k = {"few": lambda: torch.randint(0, 256, (n,), device="cuda"),
             "many": lambda: torch.randint(0, max(n // 16, 1), (n,),
                                           device="cuda"),
             "distinct": lambda: torch.randperm(n, device="cuda")}[dist]()
        a, core = device_array(n, dtype, k.to(getattr(torch, dtype)))
        del k
        skeys, spos = be.sort_run(core, None, 0, True, True)
        rec = dict(op="unique", dtype=dtype, dist=dist, n=n,
                   itemsize=a.dtype.itemsize)
        got = be.unique_run(skeys, spos, True, True)
        ref = torch.unique(core, sorted=True, return_counts=True)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[1])
        assert torch.equal(core[got[1]], got[0])    # first indices point home
        rec["n_unique"] = int(got[0].numel())
        del got, ref
        (rec["compact_ms"], rec["sort_ms"], rec["torch_ms"]), c1 = \
            timed_alternating(torch, (
                lambda: be.unique_run(skeys, spos, True, True),
                lambda: be.sort_run(core, None, 0, True, True),
                lambda: torch.unique(core, sorted=True, return_counts=True)),
                args.reps)
        (rec["unique_call_ms"], rec["sort_call_ms"]), c2 = timed_alternating(
            torch, (lambda: ra.unique(a, return_index=True,
                                      return_counts=True),
                    lambda: ra.argsort(a)), args.reps)
        rec["calls"] = c1 + c2
        ra.sync()
        t0 = time.perf_counter()
        res = np.unique(a.asarray(), return_index=True, return_counts=True)
        [ra.fromarray(r) for r in res]
        ra.sync()
        rec["host_ms"] = (time.perf_counter() - t0) * 1e3
        u, ks = rec["n_unique"], rec["itemsize"]
        rec["bytes"] = 2 * n * ks + u * (8 + ks + 8 + 8 + 16)
        rec["peak_frac"] = rec["bytes"] / PEAK_BYTES_PER_S * 1e3 \
            / rec["compact_ms"]
        rec["added_cost"] = rec["unique_call_ms"] / rec["sort_call_ms"]
        rec["vs_torch"] = (rec["sort_ms"] + rec["compact_ms"]) \
            / rec["torch_ms"]
        rec["vs_host"] = rec["unique_call_ms"] / rec["host_ms"]
        emit(rec)

    def run_search(n, m):
        a, core = device_array(
            n, "float64", torch.rand(n, dtype=torch.float64, device="cuda"))
        v = torch.sort(torch.rand(m, dtype=torch.float64, device="cuda"))[0]
        rv = ra.fromarray(v.cpu().numpy())
        res = torch.empty(n, dtype=torch.int64, device="cuda")
        rec = dict(op="searchsorted", dtype="float64", n=n, m=m, side="left")

        def kernel():
            be._check(be.lib.rt_searchsorted(
                be._stream(), ctypes.c_void_p(v.data_ptr()), m,
                ctypes.c_void_p(core.data_ptr()), 0, 1, _i64arr((n,)),
                _i64arr((1,)), RT_DTYPE["float64"], 0,
                ctypes.c_void_p(res.data_ptr())), "rt_searchsorted")

        (rec["kernel_ms"], rec["torch_ms"]), c1 = timed_alternating(
            torch, (kernel, lambda: torch.searchsorted(v, core)), args.reps)
        (rec["call_ms"],), c2 = timed_alternating(
            torch, (lambda: ra.searchsorted(rv, a),), args.reps)
        rec["calls"] = c1 + c2
        assert torch.equal(res, torch.searchsorted(v, core))
        rec["roofline_ms"] = n * 16 / PEAK_BYTES_PER_S * 1e3
        rec["peak_frac"] = rec["roofline_ms"] / rec["kernel_ms"]
        rec["vs_torch"] = rec["kernel_ms"] / rec["torch_ms"]
        emit(rec)

    for n in (int(s) for s in args.sizes.split(",")):
        for dtype in ("float64", "int32"):
            for dist in ("few", "many", "distinct"):
                run_unique(n, dtype, dist)
    for m in (10 ** 3, 10 ** 5, 10 ** 7):
        run_search(args.needles, m)
    out.close()


if __name__ == "__main__":
    main()
