"""Timings for the round-1 extension kernels at streaming scale
(axis cumsum / mask-getitem / reshape), for the indexed row gather
(`python tools/bench_extras.py take` runs that leg alone) and for the
arg-reduction kernels (`... argreduce`, likewise).  Not the judged
bench line — evidence for DESIGN.md §9's extra rows; run under rocprofv3
--stats for the per-kernel summary committed to profiles/."""

import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import ramba_amd as ra  # noqa: E402


def timed(label, fn, algo_bytes, iters=3):
    import torch
    fn()                      # warmup (compile, allocate)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    print(f"{label}: {dt*1e3:.2f} ms/iter, algorithmic "
          f"{algo_bytes/dt/1e12:.2f} TB/s", flush=True)
    return r


def take_leg(repeats=5, inner=10):
    """rt_take_rows on one GPU against torch.index_select on the same
    tensors (an independent yardstick).  Per case: `repeats` windows of
    `inner` launches each, the two implementations alternating, timed with
    rt_event_*; effective GB/s = (index bytes + 2 x gathered bytes) / time.
    (a) 1e8 random int64 indices into a 1e8-element fp64 vector (narrow
    regime); (b) 4e6 random rows of a (4e6, 128) fp64 table: 1 KiB rows,
    4 GB table, far past the Infinity Cache (wide 16-byte regime)."""
    import torch
    from ramba_amd import deferred
    rt = deferred.get_runtime()
    be = rt.backend
    lib = be.lib
    lib.rt_event_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    lib.rt_event_record.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.rt_event_elapsed.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_float)]
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    be._check(lib.rt_event_create(ctypes.byref(ev0)), "rt_event_create")
    be._check(lib.rt_event_create(ctypes.byref(ev1)), "rt_event_create")

    def window(fn):
        ms = ctypes.c_float()
        be._check(lib.rt_event_record(ev0, be._stream()), "rt_event_record")
        for _ in range(inner):
            fn()
        be._check(lib.rt_event_record(ev1, be._stream()), "rt_event_record")
        be._check(lib.rt_event_elapsed(ev0, ev1, ctypes.byref(ms)),
                  "rt_event_elapsed")
        return ms.value / inner

    def core(arr):
        bd = arr.bdarray
        _, _, _, pads = rt.shard_geometry(bd)
        sl = tuple(slice(p, p + s) for p, s in zip(pads, bd.shape))
        return be._cont(bd)[sl]

    cases = [("take_1d_1e8_fp64", (100_000_000,), 100_000_000),
             ("take_rows_4e6x128_fp64", (4_000_000, 128), 4_000_000)]
    for name, shape, m in cases:
        if len(shape) == 1:
            table = ra.arange(shape[0]) * 1.0
        else:
            table = ra.fromfunction(lambda i, j: i * 128.0 + j, shape)
        idx = ra.zeros(m, dtype=np.int64)
        out = ra.zeros((m,) + shape[1:])
        ra.sync()
        rows = be.take_index(idx.bdarray, rt)
        rows.copy_(torch.randint(0, shape[0], (m,), device="cuda"))
        t_core, o_core = core(table), core(out)
        ref = torch.empty((m,) + shape[1:], dtype=torch.float64,
                          device="cuda")

        def hand():
            be.gather_rows(table.bdarray, rt, rows, out=out.bdarray)

        def yard():
            torch.index_select(t_core, 0, rows, out=ref)

        hand(), yard()                      # warm-up of both shapes
        torch.cuda.synchronize()
        assert torch.equal(o_core, ref), name
        t_hand, t_yard = [], []
        for _ in range(repeats):            # alternate the two
            t_hand.append(window(hand))
            t_yard.append(window(yard))
        row_bytes = 8 * int(np.prod(shape[1:], dtype=np.int64))
        nbytes = m * 8 + 2 * m * row_bytes

        def gbs(ms):
            return nbytes / (ms * 1e-3) / 1e9

        rec = {"case": name, "bytes": nbytes, "repeats": repeats,
               "launches_per_window": inner}
        for tag, ts in (("rt_take_rows", t_hand), ("index_select", t_yard)):
            ts = sorted(ts)
            rec[tag] = {"ms_median": round(ts[len(ts) // 2], 4),
                        "ms_min": round(ts[0], 4),
                        "ms_max": round(ts[-1], 4),
                        "gbs_median": round(gbs(ts[len(ts) // 2]), 1),
                        "gbs_min": round(gbs(ts[-1]), 1),
                        "gbs_max": round(gbs(ts[0]), 1)}
        print("TAKE " + json.dumps(rec), flush=True)
        del table, idx, out, ref, rows, t_core, o_core
        ra.sync()


def argreduce_leg(repeats=5, inner=10, n_flat=1_000_000_000, n_side=30000):
    """The arg-reduction kernels on one GPU, timed like the take leg
    (`repeats` windows of `inner` launches, implementations alternating,
    rt_event_*).  (a) flat argmax of an n_flat-element fp64 vector against
    max() on the same array (same bytes: the floor), torch.argmax on the same
    tensor, and the two-pass where/min composition; (b) argmax(axis=1) and
    argmax(axis=0) of an (n_side, n_side) fp32 array against the
    max(axis=...) kernel and torch.argmax(dim=...).  GB/s = array bytes /
    time."""
    import torch
    from ramba_amd import deferred
    from ramba_amd.shardview import exec_boxes
    rt = deferred.get_runtime()
    be = rt.backend
    lib = be.lib
    lib.rt_event_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    lib.rt_event_record.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.rt_event_elapsed.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_float)]
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    be._check(lib.rt_event_create(ctypes.byref(ev0)), "rt_event_create")
    be._check(lib.rt_event_create(ctypes.byref(ev1)), "rt_event_create")

    def window(fn):
        ms = ctypes.c_float()
        be._check(lib.rt_event_record(ev0, be._stream()), "rt_event_record")
        for _ in range(inner):
            fn()
        be._check(lib.rt_event_record(ev1, be._stream()), "rt_event_record")
        be._check(lib.rt_event_elapsed(ev0, ev1, ctypes.byref(ms)),
                  "rt_event_elapsed")
        return ms.value / inner

    def core(arr):
        bd = arr.bdarray
        _, _, _, pads = rt.shard_geometry(bd)
        sl = tuple(slice(p, p + s) for p, s in zip(pads, bd.shape))
        return be._cont(bd)[sl]

    def addressing(arr):
        bd, v = arr.bdarray, arr.view
        lb = exec_boxes(v, bd.divisions)[rt.rank]
        d_, _, cstr, pads = rt.shard_geometry(bd)
        off0, strides = v.operand_addressing(lb[0], cstr, d_[0], pads)
        return bd, v, lb, off0, strides

    def run(name, nbytes, impls, check):
        for fn in impls.values():
            fn()                            # warm-up of every shape
        torch.cuda.synchronize()
        check()
        times = {tag: [] for tag in impls}
        for _ in range(repeats):            # alternate the implementations
            for tag, fn in impls.items():
                times[tag].append(window(fn))
        rec = {"case": name, "bytes": nbytes, "repeats": repeats,
               "launches_per_window": inner}
        for tag, ts in times.items():
            ts = sorted(ts)
            rec[tag] = {"ms_median": round(ts[len(ts) // 2], 4),
                        "ms_min": round(ts[0], 4),
                        "ms_max": round(ts[-1], 4),
                        "gbs_median": round(
                            nbytes / (ts[len(ts) // 2] * 1e-3) / 1e9, 1)}
        print("ARGREDUCE " + json.dumps(rec), flush=True)

    # (a) flat
    n = n_flat
    a = ra.sin(ra.arange(n) * 1e-3)
    ra.sync()
    bd, v, lb, _, _ = addressing(a)
    t_core = core(a)
    j = ra.arange(n)

    def flat_kernel():
        return be.arg_reduce_partial(bd, rt, v, lb, None, (1,), 0, "max",
                                     False)

    def composed():
        m = a.max()
        hit = (a == m) | (ra.isnan(a) & bool(np.isnan(m)))
        return ra.where(hit, j, n).min()

    def check_flat():
        want = int(torch.argmax(t_core))
        assert int(flat_kernel()[1].cpu()[0]) == want
        assert int(a.argmax()) == want and int(composed()) == want

    run(f"argmax_flat_{n:.0e}_fp64".replace("+", ""), n * 8,
        {"rt_arg_flat": flat_kernel, "argmax()": lambda: a.argmax(),
         "max()": lambda: a.max(),
         "torch.argmax": lambda: torch.argmax(t_core),
         "where_min_composition": composed}, check_flat)
    del a, j, t_core, bd, v, lb
    ra.sync()

    # (b) one axis
    s = n_side
    A = ra.fromfunction(lambda i, k: ((i * 7 + k * 13) % 1000) * 1.0,
                        (s, s), dtype=np.float32)
    ra.sync()
    bd, v, lb, off0, strides = addressing(A)
    T = core(A)
    for axis in (1, 0):
        mult = tuple(1 if d == axis else 0 for d in range(2))

        def arg_kernel():
            return be.arg_reduce_partial(bd, rt, v, lb, axis, mult, 0,
                                         "max", False)

        def max_kernel():
            be.axis_reduce_partial(bd, off0, strides, lb, (axis,), "max",
                                   bd.dtype)
            be.free_temps()

        def check_axis():
            got = arg_kernel()[1].reshape(-1)
            assert torch.equal(got, torch.argmax(T, dim=axis))

        run(f"argmax_axis{axis}_{s}x{s}_fp32", s * s * 4,
            {"rt_arg_axis": arg_kernel, "max(axis) kernel": max_kernel,
             "torch.argmax": lambda: torch.argmax(T, dim=axis)}, check_axis)
    del A, T
    ra.sync()


def main():
    ra.init()
    if sys.argv[1:] == ["take"]:
        take_leg()
        print("done", flush=True)
        return
    if sys.argv[1:2] == ["argreduce"]:
        # optional sizes for a quick look: argreduce N_FLAT N_SIDE
        extra = [int(float(x)) for x in sys.argv[2:4]]
        argreduce_leg(*([5, 10] + extra))
        print("done", flush=True)
        return
    n = 16384
    # N-D axis cumsum, both mappings (thread-per-line / wave-per-line)
    A = ra.fromfunction(lambda i, j: (i * 3 + j) * 1e-9, (n, n))
    ra.sync()
    nb = n * n * 8 * 2     # read + write
    timed("cumsum(axis=0) 16384^2 fp64 [thread-per-line]",
          lambda: A.cumsum(axis=0), nb)
    timed("cumsum(axis=1) 16384^2 fp64 [wave-per-line]",
          lambda: A.cumsum(axis=1), nb)

    # mask-getitem at 1e9, ~50% selectivity: read a (8) + mask copy cycle
    # (a copy 16 + mask astype-write 1 + mask read 1) + write out (4)
    m = 1_000_000_000
    B = ra.arange(m) % 2
    Bf = B * 1.0
    ra.sync()
    timed("a[mask] 1e9 fp64 sel=50% [rt_mask_compact]",
          lambda: Bf[B == 1], m * (8 + 8 + 8 + 1 + 1 + 1) + m // 2 * 8)

    # reshape 1e9 fp64: flat gather + scatter = 2r + 2w = 32 B/elem
    C = ra.arange(m) * 1.0
    ra.sync()
    timed("reshape 1e9 -> (31250, 32000) fp64 [rt_flat_copy]",
          lambda: C.reshape(31250, 32000), m * 32)
    del A, B, Bf, C
    take_leg()
    argreduce_leg()
    print("done", flush=True)


if __name__ == "__main__":
    main()
