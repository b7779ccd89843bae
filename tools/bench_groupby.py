"""Time groupby(...).sum() on one MI355X (HIP events) and write one JSON line
per case to profiles/groupby_bench.jsonl.

    python tools/bench_groupby.py [--rows 1460] [--log2n 27] [--reps 5]

Case 1, regime ROWS: a (rows, 721, 1440) float32 array grouped on axis 0 into
rows / 4 groups (day-of-year labels, k % ngroups), and float64 at half the
rows.  Yardstick: a.sum(axis=0) of the same array in the same run, which
moves the same bytes.  The routes a user had before are timed too: the loop
of masked sums, (a * mask_g).sum(axis=0) for MASKED_GROUPS of the groups,
scaled to all of them; and the host round trip's copy alone, asarray() of the
input (np.add.at on the host comes on top and is not timed).
Case 2, regimes LINE_SELECT and LINE_GATHER: a 1-D float64 array of 2^log2n
elements with 12 and with 4096 groups (random labels).  Yardstick: a.sum().

Every timed call ends in a device synchronise.  A window holds as many calls
as fill about 200 ms; each figure is the per-call median of `reps` windows
after two warm-up calls, with the lowest and highest window, and the windows
of the functions of one case alternate.  gbps = input bytes / median time;
`kernels` is the backend hook on a CSR already on the device, `hook` the same
with the CSR uploaded, `public` the whole call (CSR built on the host too)."""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sort import window  # noqa: E402

WINDOW_MS = 200.0
MASKED_GROUPS = 3


def timed(torch, fns, reps):
    """{name: (median, min, max) ms per call}; the windows alternate."""
    calls = {}
    for name, fn in fns.items():
        window(torch, fn, 1)
        first = window(torch, fn, 1)
        calls[name] = max(1, min(200, int(WINDOW_MS / max(first, 1e-3))))
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ms[name].append(window(torch, fn, calls[name]))
    return {name: (float(np.median(m)), float(min(m)), float(max(m)))
            for name, m in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1460)
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "groupby_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import ramba_amd as ra
    from ramba_amd import deferred, groupby as gb
    from ramba_amd.shardview import exec_boxes
    ra.init()
    rt = deferred.get_runtime()
    be = rt.backend
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def device_array(shape, dtype):
        a = ra.zeros(shape, dtype=dtype)
        ra.sync()
        pads = rt.lo_pads(a.bdarray)
        core = be._cont(a.bdarray)[tuple(
            slice(p, p + s) for p, s in zip(pads, a.shape))]
        core.copy_(torch.rand(shape, dtype=getattr(torch, dtype),
                              device="cuda") - 0.5)
        a.bdarray.pure = None       # written behind the engine's back
        return a

    def case(name, a, dim, lab, ng, yard, extra):
        lb = exec_boxes(a.view, a.bdarray.divisions)[0]
        csr = gb.build_csr(lab, ng)

        def public():
            a.groupby(dim, lab, ng).sum()
            ra.sync()

        def hook():
            be.group_partial(a.bdarray, rt, a.view, lb, dim, *csr, ng,
                             gb.SUM, False)
            ra.sync()

        dev_csr = [torch.from_numpy(t).to("cuda") for t in csr]

        def kernels():
            be.group_partial(a.bdarray, rt, a.view, lb, dim, *dev_csr, ng,
                             gb.SUM, False)
            ra.sync()

        def yardstick():
            yard()
            ra.sync()

        ms = timed(torch, dict(public=public, hook=hook, kernels=kernels,
                               yardstick=yardstick, **extra), args.reps)
        nbytes = a.size * a.dtype.itemsize
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        strides = (ctypes.c_int64 * a.ndim)(
            *[int(np.prod(a.shape[d + 1:])) for d in range(a.ndim)])
        rec = dict(case=name, dtype=str(a.dtype), shape=list(a.shape),
                   ngroups=ng, input_bytes=nbytes,
                   regime=be.lib.rt_group_regime(
                       a.ndim, shape, strides, dim,
                       {"float64": 0, "float32": 1}[str(a.dtype)], ng),
                   ms={k: dict(median=v[0], min=v[1], max=v[2])
                       for k, v in ms.items()})
        for k in ("public", "hook", "kernels", "yardstick"):
            rec[k + "_gbps"] = nbytes / ms[k][0] / 1e6
        rec["kernels_vs_yardstick"] = ms["kernels"][0] / ms["yardstick"][0]
        rec["hook_vs_yardstick"] = ms["hook"][0] / ms["yardstick"][0]
        rec["public_vs_yardstick"] = ms["public"][0] / ms["yardstick"][0]
        if "masked_sums" in ms:
            rec["masked_loop_ms_scaled"] = ms["masked_sums"][0] * ng \
                / MASKED_GROUPS
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    for dtype, rows in (("float32", args.rows), ("float64", args.rows // 2)):
        a = device_array((rows, 721, 1440), dtype)
        ng = max(1, rows // 4)
        lab = np.arange(rows) % ng
        masks = [ra.fromarray((lab == g).astype(dtype).reshape(-1, 1, 1))
                 for g in range(MASKED_GROUPS)]

        def masked_sums():
            for m in masks:
                (a * m).sum(axis=0)
            ra.sync()

        def host_copy():
            a.asarray()

        case("climatology", a, 0, lab, ng, lambda: a.sum(axis=0),
             dict(masked_sums=masked_sums, host_copy=host_copy))
        del a, masks

    n = 1 << args.log2n
    a = device_array((n,), "float64")
    for ng in (12, 4096):
        lab = np.random.default_rng(ng).integers(0, ng, size=n)
        case("flat", a, 0, lab, ng, lambda: a.sum(), {})
    out.close()


if __name__ == "__main__":
    main()
