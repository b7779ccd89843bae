"""Time sort / argsort on one MI355X (HIP events) and write one JSON line per
case to profiles/sort_bench.jsonl.

    python tools/bench_sort.py [--n 67108864] [--reps 3] [--out PATH]

Cases: n elements of float32 / float64 / int32 / int64, uniform random and
already sorted, and int64 in [0, 1000) (pass skipping), each keys-only
(`sort`) and with the int64 payload (`argsort`); line sorts of (2^20, 64) and
(2^14, 4096).  Per case: `kernel_ms`, rt_sort / rt_sort_lines alone on
resident buffers (scratch from torch's caching allocator); `call_ms`, the
public ramba_amd call; `host_ms`, the round trip a user had before
(asarray -> numpy stable sort -> fromarray), timed once; `torch_ms`,
torch.sort(stable=True) on the same device data, which always produces the
indices too; `passes`, the radix passes that ran; `bytes`, what those passes
move, from shapes and `passes`: one histogram read, per pass one count read
and one read and one write of the keys (and of the payloads, generated in
the first pass), or for lines two reads and one write; `peak_frac` = bytes
over 8 TB/s over kernel_ms; `vs_torch` = kernel_ms / torch_ms; `vs_host` =
call_ms / host_ms.  A timed window holds as many calls as fill about 100 ms;
kernel and torch windows alternate, and each figure is the per-call median
of `reps` windows after two warm-up calls.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12
WINDOW_MS = 100.0


def window(torch, fn, calls):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / calls


def timed_alternating(torch, fns, reps):
    """Per-call median ms of each fn; their windows alternate."""
    calls = []
    for fn in fns:
        window(torch, fn, 1)
        first = window(torch, fn, 1)
        calls.append(max(1, min(500, int(WINDOW_MS / max(first, 1e-3)))))
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(window(torch, fn, calls[k]))
    return [float(np.median(m)) for m in ms], calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "sort_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import ramba_amd as ra
    from ramba_amd import deferred
    ra.init()
    rt = deferred.get_runtime()
    be = rt.backend
    geo = be.sort_geometry()
    n = args.n
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def device_array(shape, dtype, fill):
        """A ramba array whose container core is filled on the device."""
        a = ra.zeros(shape, dtype=dtype)
        ra.sync()
        pads = rt.lo_pads(a.bdarray)
        core = be._cont(a.bdarray)[tuple(
            slice(p, p + s) for p, s in zip(pads, a.shape))]
        core.copy_(fill())
        # written behind the engine's back: no longer the zeros that a fused
        # kernel may recompute in place of reading them
        a.bdarray.pure = None
        return a, core

    def finish(rec, a, kernel, ref, call, host, nbytes):
        (rec["kernel_ms"], rec["torch_ms"]), calls = timed_alternating(
            torch, (kernel, ref), args.reps)
        (rec["call_ms"],), c2 = timed_alternating(torch, (call,), args.reps)
        rec["calls"] = {"kernel_ms": calls[0], "torch_ms": calls[1],
                        "call_ms": c2[0]}
        ra.sync()
        t0 = time.perf_counter()
        host()
        ra.sync()
        rec["host_ms"] = (time.perf_counter() - t0) * 1e3
        rec["bytes"] = nbytes(rec)
        rec["peak_frac"] = rec["bytes"] / PEAK_BYTES_PER_S * 1e3 \
            / rec["kernel_ms"]
        rec["vs_torch"] = rec["kernel_ms"] / rec["torch_ms"]
        rec["vs_host"] = rec["call_ms"] / rec["host_ms"]
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    def run_1d(dtype, dist, fill):
        a, core = device_array(n, dtype, fill)
        ks = a.dtype.itemsize
        okeys = torch.empty_like(core)
        ovals = torch.empty(n, dtype=torch.int64, device="cuda")
        for op, pay in (("sort", False), ("argsort", True)):
            rec = dict(op=op, dtype=dtype, dist=dist, n=n, itemsize=ks,
                       keys_per_lane=geo["keys_per_lane"])

            def kernel():
                rec["passes"] = be._sort_long(core, okeys, None, 0,
                                              ovals if pay else None)

            def nbytes(r):
                p = r["passes"]
                if p == 0:
                    return n * (2 * ks + (8 if pay else 0))
                return n * (ks + p * 3 * ks + (8 * (2 * p - 1) if pay else 0))

            finish(rec, a, kernel, lambda: torch.sort(core, stable=True),
                   (lambda: ra.argsort(a)) if pay else (lambda: ra.sort(a)),
                   lambda: ra.fromarray((np.argsort if pay else np.sort)(
                       a.asarray(), kind="stable")), nbytes)

    def run_lines(shape, dtype):
        a, core = device_array(
            shape, dtype, lambda: torch.rand(shape, device="cuda",
                                             dtype=getattr(torch, dtype)))
        dense = core.contiguous()
        ks = a.dtype.itemsize
        okeys = torch.empty_like(dense)
        rec = dict(op="sort", dtype=dtype, dist="uniform-lines",
                   n=list(shape), itemsize=ks, passes=None)
        finish(rec, a,
               lambda: be._sort_lines(dense, 0, shape[0], shape[1], shape[1],
                                      1, okeys, None),
               lambda: torch.sort(dense, dim=1, stable=True),
               lambda: ra.sort(a, axis=1),
               lambda: ra.fromarray(np.sort(a.asarray(), axis=1,
                                            kind="stable")),
               lambda r: 3 * ks * shape[0] * shape[1])

    for dtype in ("float32", "float64", "int32", "int64"):
        tdt = getattr(torch, dtype)
        if dtype.startswith("float"):
            uniform = lambda: torch.rand(n, dtype=tdt, device="cuda") - 0.5
        else:
            info = torch.iinfo(tdt)
            uniform = lambda: torch.randint(info.min, info.max, (n,),
                                            dtype=tdt, device="cuda")
        run_1d(dtype, "uniform", uniform)
        run_1d(dtype, "sorted", lambda: torch.sort(uniform())[0])
    run_1d("int64", "range-1000", lambda: torch.randint(
        0, 1000, (n,), dtype=torch.int64, device="cuda"))
    for shape in ((1 << 20, 64), (1 << 14, 4096)):
        for dtype in ("float32", "float64"):
            run_lines(shape, dtype)
    out.close()


if __name__ == "__main__":
    main()
