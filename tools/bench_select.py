"""Time median / percentile on one MI355X (HIP events) and write one JSON line
per case to profiles/select_bench.jsonl.

    python tools/bench_select.py [--n 67108864] [--reps 3] [--out PATH]

Cases: n elements of float32 / float64 / int32 / int64, uniform random and
already sorted, and int64 in [0, 1000); `median`, and `percentile` with q =
[1, 50, 99].  Per case: `kernel_ms`, every rt_select_pass launch of the call
replayed back to back on resident buffers with no read-back between them
(the schedule is recorded from one real call); `call_ms`, the public
ramba_amd call, which reads the counts back after every pass; `sort_ms`, the
public ramba_amd.sort of the same array in the same run; `host_ms`, the round
trip a user had before (np.median(asarray())), timed once; `torch_ms`,
torch.median (torch.quantile refuses inputs this long, so percentile is
three torch.kthvalue calls) on the same device data; `full_passes`, the
passes over the original data, `collected`, whether the candidates were
gathered, `launches`; `bytes`, what the launches move, from those: a read of
the box per full-pass launch, a write and per later launch a read of the
collected keys; `peak_frac` = bytes over 8 TB/s over kernel_ms; `vs_sort` =
call_ms / sort_ms, the bar (below 1 on uniform and sorted input).  A timed
window holds as many calls as fill about 100 ms; kernel and torch windows
alternate, as do call and sort windows, and each figure is the per-call
median of `reps` windows after two warm-up calls.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sort import PEAK_BYTES_PER_S, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "select_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import ramba_amd as ra
    from ramba_amd import deferred
    from ramba_amd.selection import KeySource
    ra.init()
    rt = deferred.get_runtime()
    be = rt.backend
    n = args.n
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def device_array(dtype, fill):
        """A ramba array whose container core is filled on the device."""
        a = ra.zeros(n, dtype=dtype)
        ra.sync()
        pads = rt.lo_pads(a.bdarray)
        core = be._cont(a.bdarray)[pads[0]:pads[0] + n]
        core.copy_(fill())
        # written behind the engine's back: no longer the zeros that a fused
        # kernel may recompute in place of reading them
        a.bdarray.pure = None
        return a, core

    def schedule(call):
        """The select_pass launches of one real call: [(source, shift,
        prefixes, collect)], a KeySource standing for 'what was collected'."""
        log = []
        real = be.select_pass

        def spy(source, shift, prefixes, collect):
            log.append((source, shift, list(prefixes), collect))
            return real(source, shift, prefixes, collect)
        be.select_pass = spy
        try:
            call()
        finally:
            del be.select_pass
        return log

    def run(dtype, dist, fill):
        a, core = device_array(dtype, fill)
        ks = a.dtype.itemsize
        k = [n // 100, n // 2, n - n // 100]
        for op, call, ref in (
                ("median", lambda: ra.median(a), lambda: torch.median(core)),
                ("percentile", lambda: ra.percentile(a, [1, 50, 99]),
                 lambda: [torch.kthvalue(core, i) for i in k])):
            log = schedule(call)
            stats = dict(rt.last_select)
            rec = dict(op=op, dtype=dtype, dist=dist, n=n, itemsize=ks,
                       **stats)

            def kernel():
                got = None
                for source, shift, prefixes, collect in log:
                    src = got if isinstance(source, KeySource) else source
                    _, _, new = be.select_pass(src, shift, prefixes, collect)
                    got = new if new is not None else got

            held = sum(c for _, _, _, c in log if c is not None)
            later = sum(isinstance(s, KeySource) for s, _, _, _ in log)
            rec["bytes"] = ks * (n * (len(log) - later) + held * (1 + later))
            (rec["kernel_ms"], rec["torch_ms"]), c1 = timed_alternating(
                torch, (kernel, ref), args.reps)
            (rec["call_ms"], rec["sort_ms"]), c2 = timed_alternating(
                torch, (call, lambda: ra.sort(a)), args.reps)
            rec["calls"] = dict(zip(("kernel_ms", "torch_ms", "call_ms",
                                     "sort_ms"), c1 + c2))
            ra.sync()
            t0 = time.perf_counter()
            np.median(a.asarray()) if op == "median" else \
                np.percentile(a.asarray(), [1, 50, 99])
            rec["host_ms"] = (time.perf_counter() - t0) * 1e3
            rec["peak_frac"] = rec["bytes"] / PEAK_BYTES_PER_S * 1e3 \
                / rec["kernel_ms"]
            rec["vs_sort"] = rec["call_ms"] / rec["sort_ms"]
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()

    for dtype in ("float32", "float64", "int32", "int64"):
        tdt = getattr(torch, dtype)
        if dtype.startswith("float"):
            uniform = lambda: torch.rand(n, dtype=tdt, device="cuda") - 0.5
        else:
            info = torch.iinfo(tdt)
            uniform = lambda: torch.randint(info.min, info.max, (n,),
                                            dtype=tdt, device="cuda")
        run(dtype, "uniform", uniform)
        run(dtype, "sorted", lambda: torch.sort(uniform())[0])
    run("int64", "range-1000", lambda: torch.randint(
        0, 1000, (n,), dtype=torch.int64, device="cuda"))
    out.close()


if __name__ == "__main__":
    main()
