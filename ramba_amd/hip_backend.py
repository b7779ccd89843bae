"""HIP product backend: gfx950 kernels via the C-ABI runtime.

Torch is plumbing only — device allocation (shard containers as raw device
tensors), the HIP stream, and the RCCL process group.  Every compute kernel
is our own HIP: fused groups JIT-compiled by `codegen` + `rt_kernel_get`
(hiprtc, gfx950), box copies by `rt_copy_box`.  FAILS LOUDLY if the
extension or a GPU is missing — no CPU fallback exists in the product path.
"""

import ctypes
import os
import time as _time

import numpy as np

from . import codegen, common
from .common import add_time
from .shardview import box_shape

LIBPATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                       "libramba_rt.so")

TORCH_DTYPE = None  # filled at init

# rt_dtype codes of include/ramba_rt.h, by NumPy dtype name (bool containers
# are uint8).  rt_cumsum and rt_axis_scan take only the codes below 4.
RT_DTYPE = {"float64": 0, "float32": 1, "int64": 2, "int32": 3, "int16": 4,
            "int8": 5, "uint8": 6, "bool": 6}
_DT_ENUM = RT_DTYPE     # earlier name, still used by the GPU tests
_OP_ENUM = {"sum": 0, "prod": 1, "min": 2, "max": 3, "all": 4, "any": 5}


def _rt_dtype4(dtype):
    """RT_DTYPE code for the entry points that take only RT_F64 .. RT_I32
    (rt_cumsum, rt_axis_scan); KeyError for any other dtype."""
    name = str(np.dtype(dtype))
    if RT_DTYPE.get(name, 4) >= 4:
        raise KeyError(name)
    return RT_DTYPE[name]


# The C ABI of include/ramba_rt.h: name -> (restype, argtypes).  _sz carries
# a uintptr_t stream handle, _str a C string or a packed argument buffer.
_int, _uint, _i64, _sz = (ctypes.c_int, ctypes.c_uint, ctypes.c_int64,
                          ctypes.c_size_t)
_dbl, _vp, _str = ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p
_p64, _pvp, _pf = (ctypes.POINTER(ctypes.c_int64),
                   ctypes.POINTER(ctypes.c_void_p),
                   ctypes.POINTER(ctypes.c_float))
_RT_ABI = {
    "rt_init": (_int, [_int]),
    "rt_device_count": (_int, []),
    "rt_last_error": (_str, []),
    "rt_kernel_get": (_int, [_str, _str, _str, _pvp]),
    "rt_compile_check": (_int, [_str]),
    "rt_launch": (_int, [_vp, _uint, _uint, _uint, _uint, _sz, _str, _sz]),
    "rt_copy_box": (_int, [_sz, _vp, _vp, _int, _p64, _p64, _p64, _i64,
                           _i64, _int]),
    "rt_combine_box": (_int, [_sz, _vp, _vp, _int, _p64, _p64, _p64, _i64,
                              _i64, _int, _int]),
    "rt_scan_chunk": (_int, []),
    "rt_mask_chunk": (_int, []),
    "rt_cumsum": (_int, [_sz, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64,
                         _vp, _dbl, _i64, _int, _int]),
    "rt_mask_compact": (_int, [_sz, _vp, _vp, _vp, _int, _p64, _p64, _p64,
                               _vp, _i64, _int, _int]),
    "rt_axis_scan": (_int, [_sz, _vp, _vp, _vp, _int, _p64, _p64, _p64,
                            _int, _int, _vp, _i64]),
    "rt_flat_copy": (_int, [_sz, _vp, _vp, _int, _p64, _p64, _i64, _i64,
                            _int, _int]),
    "rt_take_rows": (_int, [_sz, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int,
                            _p64, _p64, _p64, _i64, _i64, _int, _vp]),
    "rt_take_regime": (_int, [_vp, _vp, _int, _p64, _p64, _p64, _i64, _i64,
                              _int]),
    "rt_arg_grid_cap": (_int, []),
    "rt_arg_flat_regime": (_int, [_vp, _i64, _int, _p64, _p64, _int]),
    "rt_arg_flat": (_int, [_sz, _vp, _i64, _int, _p64, _p64, _p64, _i64,
                           _int, _int, _int, _vp, _vp, _vp, _vp]),
    "rt_arg_axis": (_int, [_sz, _vp, _i64, _int, _p64, _p64, _int, _i64,
                           _int, _int, _int, _i64, _vp, _vp, _vp, _vp]),
    "rt_arg_combine_box": (_int, [_sz, _vp, _vp, _vp, _vp, _int, _p64, _p64,
                                  _p64, _p64, _i64, _i64, _int, _int, _int]),
    "rt_stream_sync": (_int, [_sz]),
    "rt_device_sync": (_int, []),
    "rt_event_create": (_int, [_pvp]),
    "rt_event_destroy": (_int, [_vp]),
    "rt_event_record": (_int, [_vp, _sz]),
    "rt_event_elapsed": (_int, [_vp, _vp, _pf]),
}


def _load_lib():
    # on-disk kernel cache: pre-populated by the CPU suite's compile
    # checks; ships with the snapshot so GPU boxes skip hiprtc entirely
    kc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_kcache")
    os.environ.setdefault("RAMBA_KCACHE", kc)
    os.makedirs(os.environ["RAMBA_KCACHE"], exist_ok=True)
    if not os.path.exists(LIBPATH):
        raise RuntimeError(
            f"ramba_amd HIP runtime not built: {LIBPATH} missing. "
            "Run `python __graft_entry__.py build` (hipcc, gfx950). "
            "There is no CPU fallback in the product path.")
    lib = ctypes.CDLL(LIBPATH)
    for name, (restype, argtypes) in _RT_ABI.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def _i64arr(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _hb_arg_chunks(nd, axis, nout, K):
    """Chunks of the reduced axis: the small-nout / long-K test of
    HipBackend.axis_reduce_partial (one thread per output would starve the
    chip)."""
    if axis != nd - 1 and nout < 65536 and K >= 2048:
        return max(1, min((1 << 22) // max(nout, 1), (K + 255) // 256, 4096))
    return 1


def _hb_take_dense_side(t):
    st = t.stride()
    return t.data_ptr(), tuple(st[1:]), st[0], int(t.shape[0])


class HipBackend:
    name = "hip"

    def __init__(self, device=None):
        global TORCH_DTYPE
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError(
                "ramba_amd HIP backend requires an AMD GPU "
                "(torch.cuda.is_available() is False); no CPU fallback.")
        self.lib = _load_lib()
        # RAMBA_DEVICE overrides (multi-rank-on-one-GPU dry-runs);
        # production multi-GPU uses torchrun's LOCAL_RANK
        self.device = int(os.environ.get(
            "RAMBA_DEVICE", os.environ.get("LOCAL_RANK", "0"))) \
            if device is None else device
        torch.cuda.set_device(self.device)
        self._check(self.lib.rt_init(self.device), "rt_init")
        TORCH_DTYPE = {
            np.dtype(np.float64): torch.float64,
            np.dtype(np.float32): torch.float32,
            np.dtype(np.int64): torch.int64,
            np.dtype(np.int32): torch.int32,
            np.dtype(np.int16): torch.int16,
            np.dtype(np.int8): torch.int8,
            np.dtype(np.uint8): torch.uint8,
            np.dtype(np.bool_): torch.uint8,
        }
        self.containers = {}       # gid -> torch tensor
        self.temps = {}            # name -> torch tensor
        self.kernels = {}          # structural key -> GeneratedKernel
        self.rt = None
        self._dist = None
        # optional HIP-event kernel timing (bench roofline leg)
        self.time_kernels = False
        self.kernel_times_ms = []
        self.kernel_keys = []

    # ------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(
                f"{what} failed: {self.lib.rt_last_error().decode()}")

    def attach(self, rt):
        self.rt = rt

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def init_process_group(self, rank, world):
        import torch.distributed as dist
        self._dist = dist
        # RCCL in production; RAMBA_PG_BACKEND=gloo lets tests run several
        # ranks against ONE GPU (gloo needs host tensors -> staging below)
        self._pg = os.environ.get("RAMBA_PG_BACKEND", "nccl")
        if not dist.is_initialized():
            dist.init_process_group(self._pg, rank=rank, world_size=world)

    def _d(self):
        if self._dist is None:
            import torch.distributed as dist
            self._dist = dist
        return self._dist

    # -- memory -------------------------------------------------------------

    def _tdt(self, dtype):
        return TORCH_DTYPE[np.dtype(dtype)]

    def alloc_container(self, bd, rt):
        from .common import debug_poison
        _, cshape, _, _ = rt.shard_geometry(bd)
        if cshape is None:
            self.containers[bd.gid] = None
            return
        t = self.torch.empty(cshape, dtype=self._tdt(bd.dtype),
                             device="cuda")
        if debug_poison:
            t.view(self.torch.uint8).fill_(0xCC)
        self.containers[bd.gid] = t

    def free_container(self, bd):
        self.containers.pop(bd.gid, None)

    def alloc_temp(self, name, shape, dtype):
        self.temps[name] = self.torch.empty(
            shape, dtype=self._tdt(dtype), device="cuda")

    def free_temps(self):
        self.temps.clear()

    # -- box copies -----------------------------------------------------------

    def _cont(self, bd):
        c = self.containers.get(bd.gid)
        assert c is not None, f"shard for gid {bd.gid} not allocated"
        return c

    def _copy(self, dst_t, dst_strides, dst_off, src_t, src_strides, src_off,
              shape, elemsize):
        nd = len(shape)
        self._check(self.lib.rt_copy_box(
            self._stream(), ctypes.c_void_p(dst_t.data_ptr()),
            ctypes.c_void_p(src_t.data_ptr()), nd, _i64arr(shape),
            _i64arr(dst_strides), _i64arr(src_strides),
            int(dst_off), int(src_off), elemsize), "rt_copy_box")

    def _box_off(self, bd, rt, box):
        d = bd.divisions[rt.rank]
        cont = self._cont(bd)
        cs = cont.stride()
        pads = rt.lo_pads(bd)
        off = 0
        for i in range(len(bd.shape)):
            off += (int(box[0, i] - d[0, i]) + pads[i]) * cs[i]
        return off, cs

    def copy_container_to_temp(self, bd, rt, part_box, vname, need_box):
        cont = self._cont(bd)
        tmp = self.temps[vname]
        shape = box_shape(part_box)
        src_off, cs = self._box_off(bd, rt, part_box)
        lo = part_box[0] - need_box[0]
        ts = tmp.stride()
        dst_off = sum(int(lo[i]) * ts[i] for i in range(len(shape)))
        self._copy(tmp, ts, dst_off, cont, cs, src_off, shape,
                   cont.element_size())

    def pack_box(self, bd, rt, box):
        cont = self._cont(bd)
        shape = box_shape(box)
        msg = self.torch.empty(shape, dtype=cont.dtype, device="cuda")
        src_off, cs = self._box_off(bd, rt, box)
        self._copy(msg, msg.stride(), 0, cont, cs, src_off, shape,
                   cont.element_size())
        return msg

    def new_message_buffer(self, shape, dtype):
        return self.torch.empty(shape, dtype=self._tdt(dtype), device="cuda")

    def exchange_begin(self, sends, recvs):
        """POST the pairwise exchange; returns a token for
        exchange_finish.  On the nccl(=RCCL) path this is non-blocking on
        both host and device: torch orders the RCCL stream after the
        current stream (our pack kernels), so interior compute launched
        after this call overlaps the wire time.  The gloo path stages
        through host buffers (tests only)."""
        if not sends and not recvs:
            return None
        dist = self._d()
        staged = getattr(self, "_pg", "nccl") != "nccl"
        hrecvs = None
        if staged:
            self.torch.cuda.synchronize()  # packs -> host staging copies
            sends = [(d, b.cpu()) for (d, b) in sends]
            hrecvs = [(s, b, b.cpu()) for (s, b) in recvs]
        ops = []
        for (dst, buf) in sends:
            ops.append(dist.P2POp(dist.isend, buf, dst))
        if staged:
            for (src, _, hb) in hrecvs:
                ops.append(dist.P2POp(dist.irecv, hb, src))
        else:
            for (src, buf) in recvs:
                ops.append(dist.P2POp(dist.irecv, buf, src))
        reqs = dist.batch_isend_irecv(ops) if ops else []
        return (reqs, hrecvs)

    def exchange_finish(self, token):
        if token is None:
            return
        reqs, hrecvs = token
        for req in reqs:
            req.wait()
        if hrecvs:
            for (_, dbuf, hb) in hrecvs:
                dbuf.copy_(hb.to(dbuf.device))

    def exchange(self, sends, recvs):
        self.exchange_finish(self.exchange_begin(sends, recvs))

    def unpack_box_to_container(self, bd, rt, box, buf):
        cont = self._cont(bd)
        shape = box_shape(box)
        dst_off, cs = self._box_off(bd, rt, box)
        self._copy(cont, cs, dst_off, buf, buf.stride(), 0, shape,
                   cont.element_size())

    def unpack_box_to_temp(self, vname, need_box, box, buf):
        tmp = self.temps[vname]
        shape = box_shape(box)
        lo = box[0] - need_box[0]
        ts = tmp.stride()
        dst_off = sum(int(lo[i]) * ts[i] for i in range(len(shape)))
        self._copy(tmp, ts, dst_off, buf, buf.stride(), 0, shape,
                   tmp.element_size())

    def box_to_numpy(self, bd, rt, box):
        host = self.pack_box(bd, rt, box).cpu()     # D2H syncs the stream
        self._check_take_bad()
        return host.numpy().astype(
            bd.dtype, copy=False).reshape(box_shape(box))

    def write_core_from_numpy(self, bd, rt, nparr):
        cont = self._cont(bd)
        src = self.torch.from_numpy(
            np.ascontiguousarray(nparr).view(
                np.uint8 if bd.dtype == np.bool_ else bd.dtype)).to("cuda")
        core = rt.core_box(bd, rt.rank)
        dst_off, cs = self._box_off(bd, rt, core)
        self._copy(cont, cs, dst_off, src, src.stride(), 0,
                   tuple(src.shape), cont.element_size())

    # -- collectives -----------------------------------------------------------

    def bcast_numpy(self, obj, root):
        if self.rt.world == 1:
            return obj
        dist = self._d()
        lst = [obj]
        dist.broadcast_object_list(lst, src=root)
        return lst[0]

    _RED_MAP = {"sum": "SUM", "prod": "PRODUCT", "min": "MIN", "max": "MAX",
                "all": "MIN", "any": "MAX"}

    def allreduce(self, value, kind):
        dist = self._d()
        v = np.asarray(value)
        dt = v.dtype
        if kind in ("min", "max") and dt.kind == "f":
            # NCCL/RCCL MIN/MAX does not reliably propagate NaN across
            # ranks, while the in-kernel combine and NumPy do:
            # gather the per-rank partials and combine on the host
            parts = self.allgather_scalars(value, dt)
            red = np.minimum.reduce if kind == "min" else np.maximum.reduce
            return np.asarray(red(np.asarray(parts, dtype=dt)), dtype=dt)[()]
        if dt == np.bool_:
            v = v.astype(np.uint8)
        t = self.torch.from_numpy(v.reshape(1).copy())
        if getattr(self, "_pg", "nccl") == "nccl":
            t = t.to("cuda")
        dist.all_reduce(t, op=getattr(dist.ReduceOp, self._RED_MAP[kind]))
        out = t.cpu().numpy()[0]
        if dt == np.bool_:
            out = bool(out)
        return np.asarray(out, dtype=dt)[()]

    # -- kernel execution -------------------------------------------------------

    def _compile(self, gk, what):
        """rt_kernel_get for `gk` (and its finish kernel): sets the handles."""
        if int(os.environ.get("RAMBA_SHOW_CODE", "0")):
            print(f"=== {what} kernel {gk.key} ===\n{gk.source}\n",
                  flush=True)
        h = ctypes.c_void_p()
        self._check(self.lib.rt_kernel_get(
            gk.key.encode(), gk.source.encode(), gk.kname.encode(),
            ctypes.byref(h)), f"rt_kernel_get({what})")
        gk.handle = h.value
        if gk.finish is not None:
            self._compile(gk.finish, "finish")
        return gk

    def _launch(self, gk, grid, args, what, timed=True):
        """The one rt_launch; with time_kernels, `timed` launches are
        bracketed by an event pair and logged under the kernel's key."""
        timed = timed and self.time_kernels
        if timed:
            ev0 = self.torch.cuda.Event(enable_timing=True)
            ev1 = self.torch.cuda.Event(enable_timing=True)
            ev0.record()
        self._check(self.lib.rt_launch(
            ctypes.c_void_p(gk.handle), grid[0], grid[1], grid[2], 256,
            self._stream(), args, len(args)), f"rt_launch({what})")
        if timed:
            ev1.record()
            ev1.synchronize()
            self.kernel_times_ms.append(ev0.elapsed_time(ev1))
            self.kernel_keys.append(gk.key)

    def _get_kernel(self, plan):
        # fast path: structural key without source generation
        vec, classes, anchor, key = codegen.plan_structure(plan)
        cached = self.kernels.get(key)
        if cached is None:
            cached = self._compile(codegen.generate(plan), "fused")
            assert cached.key == key
            self.kernels[key] = cached
        return cached

    def launch(self, plan, recipe=None):
        ntiming = common.ntiming
        _t0 = _time.perf_counter() if ntiming else 0.0
        if recipe is not None and recipe.backend_kernel is not None:
            gk = recipe.backend_kernel
        else:
            gk = self._maybe_load_tiled(plan) or self._get_kernel(plan)
            if recipe is not None:
                recipe.backend_kernel = gk
        if gk.kind == "lt":
            self._launch_load_tiled(gk, plan)
            if ntiming:
                add_time("hb_submit", _time.perf_counter() - _t0)
            return []
        nd = gk.nd
        shape = plan.itershape
        V = gk.vec
        nx = shape[nd - 1]
        cap = int(os.environ.get("RAMBA_GRID_CAP", "32768"))
        gx = max(1, min(cap, (nx + 256 * V - 1) // (256 * V)))
        yb = gk.yblock
        gy = max(1, min(8192, (shape[nd - 2] + yb - 1) // yb)) \
            if nd >= 2 else 1
        if nd == 3:
            gz = max(1, min(64, shape[0]))
        elif nd >= 4:
            gz = max(1, min(64, shape[0] * shape[1]))
        else:
            gz = 1
        if gk.nred:
            # bound the partials array: the finish kernel is one block
            gy = max(1, min(gy, 8192 // gx))
            gz = max(1, min(gz, max(1, 8192 // (gx * gy))))

        partials = None
        outs = []
        np_partials = gx * gy * gz
        if gk.nred:
            partials = self.torch.empty(gk.nred * np_partials,
                                        dtype=self.torch.float64,
                                        device="cuda")
            for spec in plan.reductions:
                outs.append(self.torch.empty(
                    1, dtype=self._tdt(spec.dtype), device="cuda"))

        def ptr_of(name):
            if name == "__partials__":
                return partials.data_ptr()
            if name == "__npartials__":
                return np_partials
            if name in self.temps:
                return self.temps[name].data_ptr()
            op = next(o for o in plan.operands if o.name == name)
            return self._cont(op.bd).data_ptr()

        args = codegen.pack_args(gk, plan, ptr_of)
        if ntiming:
            add_time("hb_prep", _time.perf_counter() - _t0)
            _t0 = _time.perf_counter()
        self._launch(gk, (gx, gy, gz), args, "fused")
        results = []
        if gk.nred:
            fvals = {"partials": partials.data_ptr(),
                     "npartials": np_partials}
            for i, o in enumerate(outs):
                fvals[f"out{i}"] = o.data_ptr()
            self._launch(gk.finish, (1, 1, 1), gk.finish.args.pack(fvals),
                         "finish", timed=False)
            for spec, o in zip(plan.reductions, outs):
                v = o.cpu().numpy()[0]
                results.append(np.asarray(v, dtype=spec.dtype)[()])
        if ntiming:
            add_time("hb_submit", _time.perf_counter() - _t0)
        return results

    def sync(self):
        self.torch.cuda.synchronize()
        self._check_take_bad()

    # -------------------------------------------------------------------------
    # axis reductions: local strided-reduce kernel + typed
    # combining box merges (rt_combine_box)
    # -------------------------------------------------------------------------

    def fill_container(self, bd, rt, value):
        c = self.containers.get(bd.gid)
        if c is not None:
            c.fill_(float(value) if c.is_floating_point() else int(value))

    def _hb_axred_kernel(self, nd, axes, in_dtype, out_dtype, kind,
                         chunked=False):
        ck = ("axred", nd, tuple(sorted(axes)), str(in_dtype), str(out_dtype),
              kind, chunked)
        cached = self.kernels.get(ck)
        if cached is None:
            cached = self.kernels[ck] = self._compile(
                codegen.generate_axis_reduce(nd, axes, in_dtype, out_dtype,
                                             kind, chunked=chunked), "axred")
        return cached

    def _hb_axred_launch(self, gk, out_extents, red_extents, in_ptr, in_off,
                         in_strides, out_ptr, nout, chunk_spec=None):
        vals = {"in": in_ptr, "in_off": in_off, "out": out_ptr}
        for j, d in enumerate(sorted(out_extents)):
            vals[f"oe{j}"] = out_extents[d]
        for j, d in enumerate(sorted(red_extents)):
            vals[f"ke{j}"] = red_extents[d]
        for d, s in enumerate(in_strides):
            vals[f"in_s{d}"] = s
        if chunk_spec is not None:
            vals["nchunk"], vals["clen"], vals["ktot"] = chunk_spec
        if gk.lane_split:
            gx = max(1, min(4096, (nout * 64 + 255) // 256))
        else:
            gx = max(1, min(4096, (nout + 255) // 256))
        self._launch(gk, (gx, 1, 1), gk.args.pack(vals), "axred",
                     timed=False)

    def axis_reduce_partial(self, bd, off0, strides, lb, axes, kind,
                            out_dtype):
        nd = lb.shape[1]
        axes = tuple(sorted(axes))
        shape = box_shape(lb)
        kd_shape = tuple(1 if d in axes else shape[d] for d in range(nd))
        out_extents = {d: shape[d] for d in range(nd) if d not in axes}
        red_extents = {d: shape[d] for d in axes}
        nout = 1
        for v in out_extents.values():
            nout *= v
        lane_split = (nd - 1) in axes
        K = red_extents.get(axes[0], 1) if axes else 1

        # small-nout, large-K, non-lane-split reductions (sum(axis=0)) starve
        # the chip at one thread per out element: chunk the reduced axis for
        # a parallel stage 1, then reduce the chunks (measured 320 GB/s ->
        # streaming rate)
        if (not lane_split and len(axes) == 1 and nout < 65536 and K >= 2048
                and nout >= 1):
            C = max(1, min((1 << 22) // max(nout, 1), (K + 255) // 256, 4096))
        else:
            C = 1
        out_t = self.torch.empty(kd_shape, dtype=self._tdt(out_dtype),
                                 device="cuda")
        self.temps["__axred__"] = out_t
        if C > 1:
            clen = (K + C - 1) // C
            part = self.torch.empty((C, nout), dtype=self._tdt(out_dtype),
                                    device="cuda")
            self.temps["__axred_s1__"] = part
            k1 = self._hb_axred_kernel(nd, axes, bd.dtype, out_dtype, kind,
                                       chunked=True)
            self._hb_axred_launch(k1, out_extents, red_extents,
                                  self._cont(bd).data_ptr(), off0, strides,
                                  part.data_ptr(), nout * C,
                                  chunk_spec=(C, clen, K))
            # stage 2: reduce the chunk axis of the contiguous (C, nout) temp
            k2 = self._hb_axred_kernel(2, (0,), out_dtype, out_dtype, kind)
            self._hb_axred_launch(k2, {1: nout}, {0: C}, part.data_ptr(), 0,
                                  (nout, 1), out_t.data_ptr(), nout)
            return
        gk = self._hb_axred_kernel(nd, axes, bd.dtype, out_dtype, kind)
        self._hb_axred_launch(gk, out_extents, red_extents,
                              self._cont(bd).data_ptr(), off0, strides,
                              out_t.data_ptr(), nout)

    def pack_temp_box(self, vname, rel_box):
        t = self.temps[vname]
        shape = box_shape(rel_box)
        msg = self.torch.empty(shape, dtype=t.dtype, device="cuda")
        ts = t.stride()
        src_off = sum(int(rel_box[0, i]) * ts[i] for i in range(len(shape)))
        self._copy(msg, msg.stride(), 0, t, ts, src_off, shape,
                   t.element_size())
        return msg

    def _combine(self, dst_t, dst_strides, dst_off, src_t, shape, np_dtype,
                 kind):
        self._check(self.lib.rt_combine_box(
            self._stream(), ctypes.c_void_p(dst_t.data_ptr()),
            ctypes.c_void_p(src_t.data_ptr()), len(shape), _i64arr(shape),
            _i64arr(dst_strides), _i64arr(src_t.stride()), int(dst_off), 0,
            RT_DTYPE[str(np_dtype)], _OP_ENUM[kind]), "rt_combine_box")

    def combine_box_into_container(self, bd, rt, box, buf, kind):
        dst_off, cs = self._box_off(bd, rt, box)
        self._combine(self._cont(bd), cs, dst_off, buf, box_shape(box),
                      bd.dtype, kind)

    def combine_temp_into_container(self, bd, rt, box, vname, rel_box, kind):
        t = self.temps[vname]
        shape = box_shape(rel_box)
        # pack the temp slice contiguous first (combine kernel takes any
        # strides, but reuse the packed path for simplicity)
        sl = self.pack_temp_box(vname, rel_box)
        dst_off, cs = self._box_off(bd, rt, box)
        self._combine(self._cont(bd), cs, dst_off, sl, shape, bd.dtype, kind)

    # -- cumsum -----------------------------------------------

    def _hb_cumsum_src(self, bd, off0, stride, n, out_dtype):
        cont = self._cont(bd)
        src = cont
        if np.dtype(bd.dtype) != np.dtype(out_dtype):
            # pack (handles negative strides) then cast
            tmp = self.torch.empty(n, dtype=cont.dtype, device="cuda")
            self._copy(tmp, (1,), 0, cont, (stride,), off0, (n,),
                       cont.element_size())
            src = tmp.to(self._tdt(out_dtype))
            off0, stride = 0, 1
            self.temps["__cs_src__"] = src
        return src, off0, stride

    def cumsum_local_phase12(self, bd, off0, stride, n, out_dtype):
        dt = RT_DTYPE.get(str(np.dtype(out_dtype)), 4)
        if dt >= 4:
            raise NotImplementedError(f"cumsum dtype {out_dtype}")
        src, off0, stride = self._hb_cumsum_src(bd, off0, stride, n,
                                                out_dtype)
        chunk = self.lib.rt_scan_chunk()
        nblocks = max(1, (n + chunk - 1) // chunk)
        bsums = self.torch.empty(nblocks, dtype=self._tdt(out_dtype),
                                 device="cuda")
        total = self.torch.empty(1, dtype=self._tdt(out_dtype), device="cuda")
        self.temps["__cs_bsums__"] = bsums
        self.temps["__cs_state__"] = (src, off0, stride, n, nblocks, dt)
        rc = self.lib.rt_cumsum(
            self._stream(), ctypes.c_void_p(src.data_ptr()), off0, stride, n,
            None, 0, ctypes.c_void_p(bsums.data_ptr()),
            min(nblocks, 4096), None, 0.0, 0, dt, 1)
        self._check(rc, "rt_cumsum(1)")
        rc = self.lib.rt_cumsum(
            self._stream(), None, 0, 0, 0, None, 0,
            ctypes.c_void_p(bsums.data_ptr()), nblocks,
            ctypes.c_void_p(total.data_ptr()), 0.0, 0, dt, 2)
        self._check(rc, "rt_cumsum(2)")
        return np.asarray(total.cpu().numpy()[0], dtype=out_dtype)[()]

    def cumsum_local_phase3(self, bd, off0, stride, n, out_bd, out_off,
                            offset, out_dtype):
        src, off0_, stride_, n_, nblocks, dt = self.temps["__cs_state__"]
        out = self._cont(out_bd)
        fb = float(offset) if np.dtype(out_dtype).kind == "f" else 0.0
        ib = int(offset) if np.dtype(out_dtype).kind != "f" else 0
        bsums = self.temps["__cs_bsums__"]
        rc = self.lib.rt_cumsum(
            self._stream(), ctypes.c_void_p(src.data_ptr()), off0_, stride_,
            n_, ctypes.c_void_p(out.data_ptr()), out_off,
            ctypes.c_void_p(bsums.data_ptr()), min(nblocks, 4096), None,
            fb, ib, dt, 3)
        self._check(rc, "rt_cumsum(3)")

    def allgather_scalars(self, val, dtype):
        if self.rt.world == 1:
            return [val]
        dist = self._d()
        t = self.torch.from_numpy(np.asarray([val], dtype=dtype))
        if getattr(self, "_pg", "nccl") == "nccl":
            t = t.to("cuda")
        outs = [self.torch.empty_like(t) for _ in range(self.rt.world)]
        dist.all_gather(outs, t)
        return [np.asarray(o.cpu().numpy()[0], dtype=dtype)[()] for o in outs]

    # -- boolean-mask compaction (a[mask]) ---------------------

    def mask_compact(self, bd_a, bd_m, rt):
        """Local ordered compaction of the rank's core box: returns
        (dense device tensor of selected elements, count)."""
        d, _, cstr_a, pads_a = rt.shard_geometry(bd_a)
        if d is None:
            return None, 0
        _, _, cstr_m, pads_m = rt.shard_geometry(bd_m)
        nd = len(bd_a.shape)
        shape = [int(d[1, i] - d[0, i] + 1) for i in range(nd)]
        n = 1
        for sz in shape:
            n *= sz
        if n == 0:
            return None, 0
        ca, cm = self._cont(bd_a), self._cont(bd_m)
        off_a = sum(pads_a[i] * cstr_a[i] for i in range(nd))
        off_m = sum(pads_m[i] * cstr_m[i] for i in range(nd))
        a_ptr = ca.data_ptr() + off_a * ca.element_size()
        m_ptr = cm.data_ptr() + off_m * cm.element_size()
        dtc = RT_DTYPE[str(np.dtype(bd_a.dtype))]
        chunk = self.lib.rt_mask_chunk()
        nchunks = max(1, (n + chunk - 1) // chunk)
        bcounts = self.torch.empty(nchunks, dtype=self.torch.int64,
                                   device="cuda")
        total = self.torch.empty(1, dtype=self.torch.int64, device="cuda")
        st = self._stream()
        rc = self.lib.rt_mask_compact(
            st, ctypes.c_void_p(a_ptr), ctypes.c_void_p(m_ptr), None, nd,
            _i64arr(shape), _i64arr(cstr_a), _i64arr(cstr_m),
            ctypes.c_void_p(bcounts.data_ptr()), nchunks, dtc, 1)
        self._check(rc, "rt_mask_compact(1)")
        rc = self.lib.rt_cumsum(
            st, None, 0, 0, 0, None, 0, ctypes.c_void_p(bcounts.data_ptr()),
            nchunks, ctypes.c_void_p(total.data_ptr()), 0.0, 0, 2, 2)
        self._check(rc, "rt_mask_compact(2)")
        count = int(total.cpu().numpy()[0])   # D2H syncs the stream
        if count == 0:
            return None, 0
        out = self.torch.empty(count, dtype=ca.dtype, device="cuda")
        rc = self.lib.rt_mask_compact(
            st, ctypes.c_void_p(a_ptr), ctypes.c_void_p(m_ptr),
            ctypes.c_void_p(out.data_ptr()), nd, _i64arr(shape),
            _i64arr(cstr_a), _i64arr(cstr_m),
            ctypes.c_void_p(bcounts.data_ptr()), nchunks, dtc, 3)
        self._check(rc, "rt_mask_compact(3)")
        return out, count

    def write_local_dense(self, out_bd, rt, local):
        """Write a dense 1-D local tensor into the rank's container core."""
        _, _, _, pads = rt.shard_geometry(out_bd)
        cont = self._cont(out_bd)
        cont[pads[0]:pads[0] + local.shape[0]] = local

    # -- axis-wise cumsum (N-D scumulative) --------------------

    def axis_scan_local(self, bd_in, off0, strides, lshape, axis, out_bd,
                        out_off, out_strides):
        """Local inclusive scan along `axis` over the rank's box; line totals
        land in temps["__axcs_tot__"] (dense C-order line-space tensor)."""
        dt = _rt_dtype4(out_bd.dtype)
        ca, co = self._cont(bd_in), self._cont(out_bd)
        nd = len(lshape)
        lines_shape = tuple(lshape[d] for d in range(nd) if d != axis)
        tot = self.torch.empty(lines_shape, dtype=co.dtype, device="cuda")
        self.temps["__axcs_tot__"] = tot
        in_ptr = ca.data_ptr() + off0 * ca.element_size()
        out_ptr = co.data_ptr() + out_off * co.element_size()
        # axis != last with few lines: single thread-per-line starves the
        # chip -> chunked 3-pass variant (k1 local / k2 offsets / k3 apply)
        nlines = 1
        for d in range(nd):
            if d != axis:
                nlines *= lshape[d]
        length = lshape[axis]
        nchunks, tot2_ptr = 1, None
        if axis != nd - 1 and nlines < 262144 and length >= 64:
            # enough chunks to fill the chip, but keep >=32 elems per chunk
            nchunks = min(-(-524288 // max(1, nlines)), -(-length // 32))
            if nchunks > 1:
                tot2 = self.torch.empty(nchunks * nlines, dtype=co.dtype,
                                        device="cuda")
                self.temps["__axcs_tot2__"] = tot2
                tot2_ptr = ctypes.c_void_p(tot2.data_ptr())
        rc = self.lib.rt_axis_scan(
            self._stream(), ctypes.c_void_p(in_ptr), ctypes.c_void_p(out_ptr),
            ctypes.c_void_p(tot.data_ptr()), nd, _i64arr(lshape),
            _i64arr(strides), _i64arr(out_strides), axis, dt,
            tot2_ptr, nchunks if tot2_ptr else 1)
        self._check(rc, "rt_axis_scan")

    def axcs_init_offsets(self, lines_shape, dtype):
        self._axcs_np_dtype = np.dtype(dtype)
        self.temps["__axcs_off__"] = self.torch.zeros(
            lines_shape if lines_shape else (1,), dtype=self._tdt(dtype),
            device="cuda")

    def axcs_accumulate(self, rel_box, buf):
        offs = self.temps["__axcs_off__"]
        shape = box_shape(rel_box)
        ts = offs.stride()
        dst_off = sum(int(rel_box[0, i]) * ts[i] for i in range(len(shape)))
        self._check(self.lib.rt_combine_box(
            self._stream(), ctypes.c_void_p(offs.data_ptr()),
            ctypes.c_void_p(buf.data_ptr()), len(shape), _i64arr(shape),
            _i64arr(ts), _i64arr(buf.stride()), dst_off, 0,
            RT_DTYPE[str(self._axcs_np_dtype)], _OP_ENUM["sum"]),
            "axcs_accumulate")

    def axcs_apply(self, out_bd, rt, box, axis):
        """out[box] += offsets, broadcast along the scan axis (src stride
        0)."""
        offs = self.temps["__axcs_off__"]
        cont = self._cont(out_bd)
        dst_off, cs = self._box_off(out_bd, rt, box)
        shape = box_shape(box)
        ostr = list(offs.stride())
        src_strides = []
        j = 0
        for d in range(len(shape)):
            if d == axis:
                src_strides.append(0)
            else:
                src_strides.append(ostr[j])
                j += 1
        self._check(self.lib.rt_combine_box(
            self._stream(), ctypes.c_void_p(cont.data_ptr()),
            ctypes.c_void_p(offs.data_ptr()), len(shape), _i64arr(shape),
            _i64arr(cs), _i64arr(src_strides), dst_off, 0,
            RT_DTYPE[str(np.dtype(out_bd.dtype))], _OP_ENUM["sum"]),
            "axcs_apply")

    # -- reshape flat gather/scatter ------------------------------------------

    def flat_gather(self, cont, off0, strides, shape, flat0, n):
        """Dense device buffer = C-order flat subrange [flat0, flat0+n) of the
        strided box at cont[off0...]."""
        dense = self.torch.empty(n, dtype=cont.dtype, device="cuda")
        p = cont.data_ptr() + off0 * cont.element_size()
        self._check(self.lib.rt_flat_copy(
            self._stream(), ctypes.c_void_p(p),
            ctypes.c_void_p(dense.data_ptr()), len(shape), _i64arr(shape),
            _i64arr(strides), int(flat0), int(n), cont.element_size(), 0),
            "rt_flat_copy(gather)")
        return dense

    def flat_scatter(self, cont, off0, strides, shape, flat0, buf):
        p = cont.data_ptr() + off0 * cont.element_size()
        self._check(self.lib.rt_flat_copy(
            self._stream(), ctypes.c_void_p(p),
            ctypes.c_void_p(buf.data_ptr()), len(shape), _i64arr(shape),
            _i64arr(strides), int(flat0), int(buf.numel()),
            cont.element_size(), 1), "rt_flat_copy(scatter)")

    # -- indexed row gather (a[int_array] / take; runtime.take_op) ------------
    #
    # All row data movement is rt_take_rows: the gather of table rows into a
    # dense reply, the placement of replies, and the world-1 direct path
    # (container -> container).  The frontend validates every index, so the
    # kernel's bad-row counter stays zero; it is read only where the backend
    # synchronises anyway (sync / box_to_numpy) and raises if it is not.

    def _take_cont_side(self, bd, rt):
        """(pointer at core row 0, inner strides, row stride, local rows) of
        the rank's container; the core spans axes 1.. fully (take_op
        checks)."""
        d, _, cstr, pads = rt.shard_geometry(bd)
        cont = self._cont(bd)
        off = sum(pads[i] * cstr[i] for i in range(len(bd.shape)))
        return (cont.data_ptr() + off * cont.element_size(), tuple(cstr[1:]),
                cstr[0], int(d[1, 0] - d[0, 0] + 1))

    def _take_launch(self, dst, src, inner_shape, src_rows, dst_rows, n,
                     elemsize):
        if n == 0:
            return
        if getattr(self, "_take_bad", None) is None:
            self._take_bad = self.torch.zeros(1, dtype=self.torch.int32,
                                              device="cuda")
        self._take_dirty = True
        (dptr, dstr, drs, dnrows), (sptr, sstr, srs, snrows) = dst, src
        self._check(self.lib.rt_take_rows(
            self._stream(), ctypes.c_void_p(dptr), ctypes.c_void_p(sptr),
            ctypes.c_void_p(src_rows.data_ptr()) if src_rows is not None
            else None,
            ctypes.c_void_p(dst_rows.data_ptr()) if dst_rows is not None
            else None,
            int(n), snrows, dnrows, len(inner_shape), _i64arr(inner_shape),
            _i64arr(sstr), _i64arr(dstr), srs, drs, elemsize,
            ctypes.c_void_p(self._take_bad.data_ptr())), "rt_take_rows")

    def _check_take_bad(self):
        if not getattr(self, "_take_dirty", False):
            return
        self._take_dirty = False
        nbad = int(self._take_bad.cpu().numpy()[0])
        if nbad:
            self._take_bad.zero_()
            raise IndexError(
                f"take: {nbad} row number(s) out of range reached the gather "
                "kernel and were skipped (frontend validation was bypassed)")

    def take_index(self, idx_bd, rt):
        """The rank's slice of a 1-D int64 index array, as a device tensor."""
        d, _, _, pads = rt.shard_geometry(idx_bd)
        if d is None:
            return self.torch.empty(0, dtype=self.torch.int64, device="cuda")
        n = int(d[1, 0] - d[0, 0] + 1)
        return self._cont(idx_bd)[pads[0]:pads[0] + n]

    def gather_rows(self, src_bd, rt, rows, out=None, positions=None):
        """Rows `rows` (local row numbers, device int64) of the rank's shard:
        into a fresh dense (n,)+row_shape tensor, or, with `out`, into that
        array's container core at rows positions[k] (rows 0..n-1 if None)."""
        n = int(rows.numel())
        cont = self._cont(src_bd)
        inner = tuple(src_bd.shape[1:])
        rows = rows.contiguous()
        if out is None:
            dense = self.torch.empty((n,) + inner, dtype=cont.dtype,
                                     device="cuda")
            dst = _hb_take_dense_side(dense)
        else:
            dense = None
            dst = self._take_cont_side(out, rt)
            if positions is not None:
                positions = positions.contiguous()
        self._take_launch(dst, self._take_cont_side(src_bd, rt), inner, rows,
                          positions, n, cont.element_size())
        return dense

    def place_rows(self, out_bd, rt, positions, dense):
        """out[positions[k]] = dense[k] on the rank's container core."""
        dense = dense.contiguous()
        self._take_launch(self._take_cont_side(out_bd, rt),
                          _hb_take_dense_side(dense), tuple(out_bd.shape[1:]),
                          None, positions.contiguous(), int(dense.shape[0]),
                          dense.element_size())

    # -- argmax / argmin pair reductions (runtime.arg_reduce_op) --------------
    #
    # The two hooks of ramba_amd/argreduce.py on the rt_arg_* kernels.  The
    # operand is read in place through the view's strides; pairs stay on the
    # device as (values in the array's dtype, int64 indices).

    def arg_reduce_partial(self, bd, rt, view, lb, axis, mult, idx0, kind,
                           skipna):
        d_, _, cstrides, pads = rt.shard_geometry(bd)
        off0, strides = view.operand_addressing(lb[0], cstrides, d_[0], pads)
        shape = box_shape(lb)
        nd = len(shape)
        cont = self._cont(bd)
        tdt = self._tdt(bd.dtype)
        i64 = self.torch.int64
        dtc = RT_DTYPE[str(np.dtype(bd.dtype))]
        is_max, skipna = int(kind == "max"), int(bool(skipna))

        def new(shp, dt):
            return self.torch.empty(shp, dtype=dt, device="cuda")

        if axis is None:
            cap = self.lib.rt_arg_grid_cap()
            sv, si = new(cap, tdt), new(cap, i64)
            ov, oi = new(1, tdt), new(1, i64)
            self._check(self.lib.rt_arg_flat(
                self._stream(), ctypes.c_void_p(cont.data_ptr()), int(off0),
                nd, _i64arr(shape), _i64arr(strides), _i64arr(mult),
                int(idx0), dtc, is_max, skipna,
                ctypes.c_void_p(sv.data_ptr()),
                ctypes.c_void_p(si.data_ptr()),
                ctypes.c_void_p(ov.data_ptr()),
                ctypes.c_void_p(oi.data_ptr())), "rt_arg_flat")
            return ov, oi
        kd = tuple(1 if d == axis else shape[d] for d in range(nd))
        K = shape[axis]
        nout = 1
        for s in kd:
            nout *= s
        ov, oi = new(kd, tdt), new(kd, i64)
        C = _hb_arg_chunks(nd, axis, nout, K)
        pv = pi = None
        if C > 1:
            pv, pi = new(C * nout, tdt), new(C * nout, i64)
        self._check(self.lib.rt_arg_axis(
            self._stream(), ctypes.c_void_p(cont.data_ptr()), int(off0), nd,
            _i64arr(shape), _i64arr(strides), int(axis), int(idx0), dtc,
            is_max, skipna, C,
            ctypes.c_void_p(pv.data_ptr()) if C > 1 else None,
            ctypes.c_void_p(pi.data_ptr()) if C > 1 else None,
            ctypes.c_void_p(ov.data_ptr()), ctypes.c_void_p(oi.data_ptr())),
            "rt_arg_axis")
        return ov, oi

    def arg_combine_box(self, out_bd, rt, box, best, rel, src_vals, src_idx,
                        kind, skipna):
        shape = box_shape(box)
        nd = len(shape)
        di_off, cs = self._box_off(out_bd, rt, box)
        bs = best.stride()
        dv_off = sum(int(rel[0, i]) * bs[i] for i in range(nd))
        src_vals, src_idx = src_vals.contiguous(), src_idx.contiguous()
        self._check(self.lib.rt_arg_combine_box(
            self._stream(), ctypes.c_void_p(best.data_ptr()),
            ctypes.c_void_p(self._cont(out_bd).data_ptr()),
            ctypes.c_void_p(src_vals.data_ptr()),
            ctypes.c_void_p(src_idx.data_ptr()), nd, _i64arr(shape),
            _i64arr(bs), _i64arr(cs), _i64arr(src_idx.stride()), int(dv_off),
            int(di_off), self._arg_dtc(best), int(kind == "max"),
            int(bool(skipna))), "rt_arg_combine_box")

    def _arg_dtc(self, t):
        """RT_DTYPE code of a value tensor (bool containers are uint8)."""
        code = RT_DTYPE.get(str(t.dtype).rpartition(".")[2])  # torch.int8
        if code is None:
            raise TypeError(
                f"arg reduction: unsupported value dtype {t.dtype}")
        return code

    # -- cross-stage fusion (staged/tiled kernel; ramba_amd/staged.py) --------

    supports_staged = True

    def container_addr(self, bd):
        return self._cont(bd).data_ptr()

    def tiled_kernel(self, desc):
        """Build (or fetch) the staged/tiled kernel; returns a handle token
        or None (fall back to sequential)."""
        ck = ("tiled", codegen.staged_tiled_key(desc))
        cached = self.kernels.get(ck)
        if cached is None:
            try:
                gk = codegen.generate_staged_tiled(desc)
            except NotImplementedError:
                return None
            assert gk.key == ck[1]
            cached = self.kernels[ck] = self._compile(gk, "tiled")
        return cached

    def tiled_launch(self, gk, vals, ntiles, red_dtypes=None, rec=None):
        gx = max(1, min(int(os.environ.get("RAMBA_GRID_CAP", "32768")),
                        ntiles))
        red_dtypes = red_dtypes or []
        if rec is not None and rec.partials is not None \
                and len(rec.partials) == len(red_dtypes) \
                and all(t.shape[0] == gx for t in rec.partials):
            parts = rec.partials
            for ri, t in enumerate(parts):
                vals[f"red{ri}_ptr"] = t.data_ptr()
        else:
            parts = []
            for ri, dt in enumerate(red_dtypes):
                t = self.torch.empty(gx, dtype=self._tdt(dt), device="cuda")
                parts.append(t)
                vals[f"red{ri}_ptr"] = t.data_ptr()
            if rec is not None:
                rec.partials = parts
        self._launch(gk, (gx, 1, 1), gk.args.pack(vals), "tiled")
        out = []
        for t, dt in zip(parts, red_dtypes):
            total = self.torch.empty(1, dtype=t.dtype, device="cuda")
            rc = self.lib.rt_cumsum(
                self._stream(), None, 0, 0, 0, None, 0,
                ctypes.c_void_p(t.data_ptr()), gx,
                ctypes.c_void_p(total.data_ptr()), 0.0, 0,
                _rt_dtype4(dt), 2)
            self._check(rc, "rt_cumsum(tk partials)")
            out.append(np.asarray(total.cpu().numpy()[0], dtype=dt)[()])
        return out

    # -- load-tiled stencil dispatch ----------------------

    def _maybe_load_tiled(self, plan):
        """If the plan is a qualifying 2-D stencil (>=3 same-array shifted
        readers), build the LDS load-tiled kernel instead of the vectorized
        elementwise one.  Returns its GeneratedKernel (kind 'lt') or None."""
        # measured on MI355X (profiles/README r02): at 16x256 tiles the LDS
        # kernel cuts HBM FETCH 1.56x -> 1.21-1.27x of algorithmic AND beats
        # the vectorized cross-row-sharing kernel at PRK scale (30000^2:
        # 1.562 vs 1.599 ms; 4096^2 par).  Default ON; =0 selects the
        # vectorized kernel for A/B.  (The first 32x256 tiling lost to
        # occupancy: 36 KB LDS -> 2.24 ms.)
        if os.environ.get("RAMBA_STENCIL_LDS", "1") == "0":
            return None
        if plan.reductions or len(plan.itershape) != 2:
            return None
        if plan.itershape[0] * plan.itershape[1] < (1 << 16):
            return None         # rim slabs / tiny boxes: vectorized path wins
        fams = codegen.find_stencil_families(plan)
        if not fams:
            return None
        gk = codegen.generate_load_tiled(plan, fams)
        cached = self.kernels.get(("lt", gk.key))
        if cached is None:
            cached = self.kernels[("lt", gk.key)] = self._compile(
                gk, "load_tiled")
        # fam_meta carries this plan's offsets: keep gk, share the handle
        gk.handle = cached.handle
        return gk

    def _launch_load_tiled(self, gk, plan):
        opmap = {o.name: o for o in plan.operands}
        vals = {"n0": plan.itershape[0], "n1": plan.itershape[1],
                "gs0": plan.global_start[0], "gs1": plan.global_start[1]}
        for fi, (rep, anchor, s0) in enumerate(gk.fam_meta):
            op = opmap[rep]
            vals[f"fam{fi}_ptr"] = self._cont(op.bd).data_ptr() \
                if op.kind == "container" else self.temps[op.name].data_ptr()
            vals[f"fam{fi}_off"] = anchor
            vals[f"fam{fi}_s0"] = s0
        for name in gk.others:
            op = opmap[name]
            vals[f"{name}_ptr"] = self._cont(op.bd).data_ptr() \
                if op.kind == "container" else self.temps[name].data_ptr()
            vals[f"{name}_off"] = op.offset0
            vals[f"{name}_s0"] = op.strides[0]
            vals[f"{name}_s1"] = op.strides[1]
        for n, (v, dt) in plan.scalars.items():
            vals[n] = v
        th, cw, seg = gk.tile
        tiles0 = (plan.itershape[0] + th - 1) // th
        ntiles = ((tiles0 + seg - 1) // seg) \
            * ((plan.itershape[1] + cw - 1) // cw)
        gx = max(1, min(int(os.environ.get("RAMBA_GRID_CAP", "32768")),
                        ntiles))
        self._launch(gk, (gx, 1, 1), gk.args.pack(vals), "load_tiled")
