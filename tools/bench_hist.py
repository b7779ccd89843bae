"""Time histogram / bincount on one MI355X (HIP events) and write one JSON
line per case to profiles/hist_bench.jsonl.

    python tools/bench_hist.py [--n 134217728] [--reps 5] [--out PATH]
                               [--lib PATH --variant NAME]

Per case: `kernel_ms`, rt_hist alone on resident edges and counts;
`call_ms`, the public ramba_amd call; `sum_ms`, this project's sum() of the
same array (the same read with no binning); `torch_ms`, torch.histc /
torch.bincount on the same device data (null where not timed);
`roofline_ms`, n x itemsize bytes over 8 TB/s; `peak_frac` = roofline_ms /
kernel_ms; `vs_sum` = kernel_ms / sum_ms.  A timed window holds as many calls
as fill about 50 ms (`calls`); each figure is the per-call median of `reps`
windows after two warm-up calls; a call slower than 100 ms is timed once.
`--lib` times another build of the runtime library (one compiled with
-DHIST_PREAGG=0, say) and `--variant` names it in the rows.
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12


WINDOW_MS = 50.0


def timed(torch, fn, reps):
    """(ms per call, calls per timed window)."""
    def window(calls):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls
    window(1)
    first = window(1)
    if first > 100.0:       # a call this slow is timed once, not `reps` times
        return first, 1
    calls = max(1, min(500, int(WINDOW_MS / max(first, 1e-3))))
    return float(np.median([window(calls) for _ in range(reps)])), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "hist_bench.jsonl"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--variant", default="shipped")
    args = ap.parse_args()

    import torch
    import ramba_amd as ra
    from ramba_amd import deferred, hip_backend
    from ramba_amd.hip_backend import RT_DTYPE, _i64arr
    if args.lib:
        hip_backend.LIBPATH = os.path.abspath(args.lib)
    ra.init()
    rt = deferred.get_runtime()
    be = rt.backend
    geo = be.hist_geometry()
    n = args.n

    def device_array(dtype, fill):
        """A ramba array whose container core is filled on the device."""
        a = ra.zeros(n, dtype=dtype)
        ra.sync()
        pad = rt.lo_pads(a.bdarray)[0]
        core = be._cont(a.bdarray)[pad:pad + n]
        core.copy_(fill())
        # written behind the engine's back: the array is no longer the zeros
        # that a fused kernel may recompute in place of reading them
        a.bdarray.pure = None
        return a, core, pad

    def run_case(name, a, core, pad, mode, nbins, edges, call, ref):
        cont = be._cont(a.bdarray)
        counts = torch.zeros(nbins, dtype=torch.int64, device="cuda")
        dev_edges = None if edges is None else \
            torch.from_numpy(edges).to("cuda")

        def kernel():
            be._check(be.lib.rt_hist(
                be._stream(), ctypes.c_void_p(cont.data_ptr()), pad, 1,
                _i64arr([n]), _i64arr([1]), RT_DTYPE[str(a.dtype)], mode,
                None if dev_edges is None
                else ctypes.c_void_p(dev_edges.data_ptr()),
                0 if edges is None else RT_DTYPE[str(edges.dtype)], nbins,
                ctypes.c_void_p(counts.data_ptr()), None), "rt_hist")

        rec = dict(name, variant=args.variant, n=n, nbins=nbins,
                   regime=be.lib.rt_hist_regime(nbins),
                   itemsize=a.dtype.itemsize, calls={})
        for key, fn in (("kernel_ms", kernel), ("call_ms", call),
                        ("sum_ms", lambda: a.sum()), ("torch_ms", ref)):
            rec[key] = None
            # sum() and torch do not depend on the library under --lib
            if fn is not None and not (args.lib and key[0] in "st"):
                rec[key], rec["calls"][key] = timed(torch, fn, args.reps)
            print("#", name, nbins, key, rec[key], flush=True)
        rec["roofline_ms"] = n * a.dtype.itemsize / PEAK_BYTES_PER_S * 1e3
        rec["peak_frac"] = rec["roofline_ms"] / rec["kernel_ms"]
        rec["vs_sum"] = rec["sum_ms"] and rec["kernel_ms"] / rec["sum_ms"]
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    bins_list = (64, 4096, geo["block_max_bins"], geo["block_max_bins"] + 1,
                 10 ** 6)
    for dtype, tdt in (("float64", torch.float64), ("float32", torch.float32)):
        fills = {
            "uniform": lambda: torch.rand(n, dtype=tdt, device="cuda"),
            "sorted": lambda: torch.sort(
                torch.rand(n, dtype=tdt, device="cuda"))[0],
            "equal": lambda: torch.full((n,), 0.5, dtype=tdt, device="cuda"),
        }
        for dist, fill in fills.items():
            a, core, pad = device_array(dtype, fill)
            for nbins in bins_list:
                edges = np.histogram_bin_edges(np.empty(0, dtype), nbins,
                                               (0, 1))
                run_case(dict(op="histogram", dtype=dtype, dist=dist), a,
                         core, pad, 1, nbins, edges,
                         lambda: ra.histogram(a, bins=nbins, range=(0, 1)),
                         # torch.histc needs seconds to minutes per call on
                         # sorted / constant input with many bins: not timed
                         (lambda: torch.histc(core, bins=nbins, min=0, max=1))
                         if dist == "uniform" or nbins <= 4096 else None)
            del a, core
    for dtype, tdt in (("int32", torch.int32), ("int64", torch.int64)):
        for nbins in (256, 10 ** 7):
            a, core, pad = device_array(
                dtype, lambda: torch.randint(0, nbins, (n,), dtype=tdt,
                                             device="cuda"))
            run_case(dict(op="bincount", dtype=dtype, dist="uniform"), a,
                     core, pad, 0, nbins, None,
                     lambda: ra.bincount(a, minlength=nbins),
                     lambda: torch.bincount(core, minlength=nbins))
            del a, core
    out.close()


if __name__ == "__main__":
    main()
