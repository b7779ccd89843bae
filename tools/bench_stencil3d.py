"""Time 3-D stencil updates on one MI355X (HIP events), the plane-marching
LDS kernel ('lt3') against the vectorized kernel on the same arrays in the
same process, and write one JSON line per case to
profiles/stencil3d_bench.jsonl.

    python tools/bench_stencil3d.py [--reps 5] [--cases 7pt-f32-512,...]
                                    [--routes lds,vec] [--out PATH]

Cases: a 7-point float32 update at 128^3, 256^3, 512^3 and 768^3 (interior
shapes), 7-point float64, a radius-4 star (25 points) and a 27-point box at
512^3.  The input holds random data, so nothing is recomputed from the index.
A step is the update's flush; a window holds as many steps as fill about
200 ms and ends in a device synchronise.  Each figure is the per-step median
of `reps` windows after two warm-up steps, with the lowest and highest
window; the windows of the two routes alternate.  The route is switched with
RAMBA_STENCIL_LDS, with the runtime's recipe cache dropped at every switch
(it keeps the kernel).  `kernel_ms` is the median of 20 single launches, each
between its own event pair, with the lowest and highest: where a step is
host-bound (the small cases) it is the figure that tells the routes apart.
RAMBA_LT3_TH / _NCH / _SEG apply as usual and are recorded, so a geometry
sweep is this tool run under different settings.
gelem_s = outputs / median; tbyte_s counts 2 x itemsize per output, and
`of_achievable` is that over 6.3 TB/s."""

import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sort import window  # noqa: E402

WINDOW_MS = 200.0
ACHIEVABLE = 6.3e12


def star(r):
    return [(r, r, r)] + [tuple(r + s * k * (a == d) for a in range(3))
                          for d in range(3) for k in range(1, r + 1)
                          for s in (-1, 1)]


CASES = {f"7pt-f32-{n}": ("float32", n, star(1)) for n in (128, 256, 512, 768)}
CASES["7pt-f64-512"] = ("float64", 512, star(1))
CASES["star4-f32-512"] = ("float32", 512, star(4))
CASES["box27-f32-512"] = ("float32", 512,
                          list(itertools.product(range(3), repeat=3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--routes", default="lds,vec")
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "stencil3d_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import ramba_amd as ra
    from ramba_amd import deferred
    ra.init()
    rt = deferred.get_runtime()
    be = rt.backend
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    routes = args.routes.split(",")

    def device_array(shape, dtype, rand):
        a = ra.zeros(shape, dtype=dtype)
        ra.sync()
        if rand:
            pads = rt.lo_pads(a.bdarray)
            core = be._cont(a.bdarray)[tuple(
                slice(p, p + s) for p, s in zip(pads, shape))]
            core.copy_(torch.rand(shape, dtype=getattr(torch, dtype),
                                  device="cuda") - 0.5)
        a.bdarray.pure = None       # user data, not a fill
        return a

    for name in args.cases.split(","):
        dtype, n, offs = CASES[name]
        ext = max(max(o) for o in offs)
        c = ext // 2
        A = device_array((n + ext,) * 3, dtype, True)
        B = device_array((n + ext,) * 3, dtype, False)

        def step():
            acc = None
            for k, o in enumerate(offs):
                t = (0.5 + 0.125 * k) * A[tuple(slice(x, x + n) for x in o)]
                acc = t if acc is None else acc + t
            B[c:c + n, c:c + n, c:c + n] = acc
            del acc, t
            deferred.flush()

        def switch(route):
            os.environ["RAMBA_STENCIL_LDS"] = "1" if route == "lds" else "0"
            rt.__dict__.pop("_recipe_cache", None)
            step()
            ra.sync()

        calls, kinds, kern = {}, {}, {}
        for route in routes:
            for k in [k for k in be.kernels if k[0] == "lt3"]:
                del be.kernels[k]
            switch(route)
            kinds[route] = "lt3" if any(k[0] == "lt3"
                                        for k in be.kernels) else "fused"
            # the kernel alone: an event pair around each of 20 launches
            be.time_kernels, be.kernel_times_ms = True, []
            for _ in range(20):
                step()
            be.time_kernels = False
            kt = be.kernel_times_ms
            kern[route] = [float(np.median(kt)), float(min(kt)),
                           float(max(kt))]
            window(torch, step, 1)
            first = window(torch, step, 1)
            calls[route] = max(1, min(2000, int(WINDOW_MS / max(first, 1e-3))))
        ms = {route: [] for route in routes}
        for _ in range(args.reps):
            for route in routes:
                switch(route)
                ms[route].append(window(torch, step, calls[route]))
        rec = dict(case=name, dtype=dtype, interior=[n] * 3, points=len(offs),
                   geometry={k: os.environ.get(k) for k in (
                       "RAMBA_LT3_TH", "RAMBA_LT3_NCH", "RAMBA_LT3_SEG")})
        for route in routes:
            med = float(np.median(ms[route]))
            rec[route] = dict(
                kernel=kinds[route], kernel_ms=kern[route][0],
                kernel_ms_min=kern[route][1], kernel_ms_max=kern[route][2],
                steps_per_window=calls[route],
                ms=med, ms_min=float(min(ms[route])),
                ms_max=float(max(ms[route])), gelem_s=n ** 3 / med / 1e6,
                tbyte_s=2 * np.dtype(dtype).itemsize * n ** 3 / med / 1e9,
                of_achievable=2 * np.dtype(dtype).itemsize * n ** 3
                / (med * 1e-3) / ACHIEVABLE)
        if len(routes) == 2:
            a, b = (rec[r] for r in routes)
            rec["lds_over_vec"] = rec["lds"]["ms"] / rec["vec"]["ms"]
            rec["windows_overlap"] = not (a["ms_max"] < b["ms_min"]
                                          or b["ms_max"] < a["ms_min"])
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        del A, B
        ra.sync()
    out.close()


if __name__ == "__main__":
    main()
