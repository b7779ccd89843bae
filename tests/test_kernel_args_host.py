"""The argument structs of the generated kernels, checked on the host.

`codegen.KernelArgs` is the one place where a member's C type, its name and
its `struct` code meet; a slip there hands a kernel a wrong pointer.  One
kernel per struct kind (fused `Args`, its finish `FArgs`, `AxArgs` plain and
chunked, staged/tiled `TkArgs`, load-tiled `LtArgs`) is captured with a
recording backend and checked three ways:

(a) the packed bytes equal a layout written out by hand below, member by
    member (an independent restatement: format code, name, value);
(b) the declaration, compiled by the ROCm clang++ for the host, has the
    `sizeof` and `offsetof` of the Python `Struct`;
(c) a mapping that lacks a member raises KeyError, and names the struct does
    not have are ignored.
"""

import copy
import struct
import subprocess

import numpy as np
import pytest

from ramba_amd import aot, codegen

from test_preamble_host import _find_clangxx


class RecordingBackend(aot.AotCompileBackend):
    """Compile-only backend that compiles nothing: it keeps every plan and
    staged descriptor the runtime hands it."""

    def __init__(self):
        self.rt = None
        self.compiled = 0
        self.plans = []
        self.descs = []

    def _cc(self, source):
        pass

    def launch(self, plan, recipe=None):
        self.plans.append(plan)
        return super().launch(plan, recipe)

    def tiled_kernel(self, desc):
        self.descs.append(desc)
        return codegen.generate_staged_tiled(desc)


def _capture():
    """Run the five programs on a recording backend swapped into the live
    runtime, with the runtime's recipe caches set aside meanwhile (they are
    keyed by group structure, not by backend)."""
    import ramba_amd as ra
    from ramba_amd import deferred
    from oracle.numpy_backend import NumpyBackend
    if not ra._initialized["done"]:
        ra.init(backend=NumpyBackend())
    deferred.flush()
    rt = deferred.get_runtime()
    old = rt.backend
    caches = {k: rt.__dict__.pop(k) for k in ("_recipe_cache", "_staged_cache")
              if k in rt.__dict__}
    be = RecordingBackend()
    rt.backend = be
    be.attach(rt)
    out = {}
    try:
        # 1-D, vec 2, a float and an int scalar, a reduction
        F = ra.arange(4099) / 1000.0
        I = ra.arange(4099)
        ra.sync()
        be.plans.clear()
        s = (F * 2.5 + I * 3).sum()
        ra.sync()
        (out["fused"],) = be.plans
        del F, I, s
        ra.sync()
        # the 5-point staged pair of aot.seed() at 64x64, with its sum
        Z = ra.zeros((64, 64), dtype=np.float64)
        ra.sync()
        src = ra.fromfunction(lambda x, y: (x * 64 + y) * 1e-6, (64, 64),
                              dtype=np.float64)
        ss = ra.sin(src)
        Z[1:-1, 1:-1] = (ss[:-2, 1:-1] + ss[2:, 1:-1] + ss[1:-1, :-2]
                         + ss[1:-1, 2:] - 4.0 * ss[1:-1, 1:-1])
        Z.sum()
        ra.sync()
        (out["tiled"],) = be.descs
        del Z, src, ss
        ra.sync()
        # fp32 5-point stencil over a 256x256 interior: the smallest box
        # the load-tiled path accepts
        X = ra.fromfunction(lambda x, y: x + y, (258, 258), dtype=np.float32)
        Y = ra.zeros((258, 258), dtype=np.float32)
        ra.sync()
        be.plans.clear()
        Y[1:-1, 1:-1] = (X[:-2, 1:-1] + X[2:, 1:-1] + X[1:-1, :-2]
                         + X[1:-1, 2:] - 4.0 * X[1:-1, 1:-1])
        ra.sync()
        out["lt"] = next(p for p in be.plans if p.itershape == (256, 256))
        del X, Y
        ra.sync()
    finally:
        deferred.flush()
        rt.backend = old
        for k in ("_recipe_cache", "_staged_cache"):
            rt.__dict__.pop(k, None)
        rt.__dict__.update(caches)
    return out


# The layouts, by hand: (struct code, member name[, value]).  A row without
# a value gets a sentinel from its position (_value).

FUSED = [
    ("q", "n0", 4099),
    ("q", "gs0", 17),
    ("Q", "v0001_p", 0x7F0000001000),
    ("q", "v0001_off", 1001),
    ("Q", "v0004_p", 0x7F0000002000),
    ("q", "v0004_off", 1002),
    ("Q", "v0007_p", 0x7F0000003000),
    ("q", "v0007_off", 1003),
    ("d", "s0002", 6.25),
    ("q", "s0005", -7),
    ("q", "lead", 1),                # (-1003) % 2: v0007 is the anchor
    ("Q", "partials", 0x7F0000004000),
    ("q", "npartials", 77),
]
FINISH = [("Q", "partials"), ("q", "npartials"), ("Q", "out0")]
AXRED = [("q", "oe0"), ("q", "ke0"), ("Q", "in"), ("q", "in_off"),
         ("q", "in_s0"), ("q", "in_s1"), ("Q", "out")]
AXRED_CHUNKED = AXRED + [("q", "nchunk"), ("q", "clen"), ("q", "ktot")]
TILED = (
    [("q", n) for n in ("n0", "n1", "gs0", "gs1", "gb0", "gb1", "N0", "N1")]
    + [("Q", "p_v0004_ptr"), ("q", "p_v0004_off"), ("q", "p_v0004_s0"),
       ("q", "p_v0004_s1"), ("q", "p_v0004_lo0"), ("q", "p_v0004_hi0"),
       ("q", "p_v0004_lo1"), ("q", "p_v0004_hi1"),
       ("Q", "p_v0003_ptr"), ("q", "p_v0003_off"), ("q", "p_v0003_s0"),
       ("q", "p_v0003_s1"), ("q", "p_v0003_lo0"), ("q", "p_v0003_hi0"),
       ("q", "p_v0003_lo1"), ("q", "p_v0003_hi1"),
       ("Q", "v0012_ptr"), ("q", "v0012_off"), ("q", "v0012_s0"),
       ("q", "v0012_s1"),
       ("q", "p_s0001"), ("d", "p_s0002"), ("d", "s0008"),
       ("Q", "red0_ptr"),
       ("Q", "rsrc0_ptr"), ("q", "rsrc0_off"), ("q", "rsrc0_s0"),
       ("q", "rsrc0_s1"), ("q", "rim0_n")]
    + [("q", f"rim0_{k}_{f}") for k in range(4)
       for f in ("lo0", "hi0", "lo1", "hi1")])
LOAD_TILED = [
    ("q", "n0"), ("q", "n1"), ("q", "gs0"), ("q", "gs1"),
    ("Q", "fam0_ptr"), ("q", "fam0_off"), ("q", "fam0_s0"),
    ("Q", "v0012_ptr"), ("q", "v0012_off"), ("q", "v0012_s0"),
    ("q", "v0012_s1"),
    ("d", "s0008"),
]


def _value(i, row):
    if len(row) == 3:
        return row[2]
    return {"Q": 0x7F0000000000 + 0x1000 * (i + 1), "q": -(1000 + i),
            "d": i + 0.25}[row[0]]


def _values(rows):
    return {row[1]: _value(i, row) for i, row in enumerate(rows)}


def _expected(rows):
    return b"".join(struct.pack("<" + row[0], _value(i, row))
                    for i, row in enumerate(rows))


@pytest.fixture(scope="module")
def kernels():
    """name -> (GeneratedKernel, hand layout)."""
    cap = _capture()
    f64 = np.dtype(np.float64)
    fused = codegen.generate(cap["fused"])
    lt = cap["lt"]
    return {
        "fused": (fused, FUSED),
        "finish": (fused.finish, FINISH),
        "axred": (codegen.generate_axis_reduce(2, (0,), f64, f64, "sum"),
                  AXRED),
        "axred_chunked": (codegen.generate_axis_reduce(
            2, (0,), f64, f64, "sum", chunked=True), AXRED_CHUNKED),
        "tiled": (codegen.generate_staged_tiled(cap["tiled"]), TILED),
        "lt": (codegen.generate_load_tiled(
            lt, codegen.find_stencil_families(lt)), LOAD_TILED),
        "fused_plan": cap["fused"],
    }


KINDS = ["fused", "finish", "axred", "axred_chunked", "tiled", "lt"]


def test_the_kernels_are_the_ones_meant(kernels):
    fused = kernels["fused"][0]
    assert (fused.kind, fused.vec, fused.nd, fused.nred) == ("fused", 2, 1, 1)
    assert fused.anchor == "v0007" and fused.finish.kind == "finish"
    assert not kernels["axred"][0].lane_split
    tk = kernels["tiled"][0]
    assert tk.kind == "tiled" and tk.kname == "tk_" + tk.key
    lt = kernels["lt"][0]
    assert (lt.kind, lt.tile, lt.others) == ("lt", (16, 256, 1), ["v0012"])
    assert [m[0] for m in lt.fam_meta] == ["v0001"]


@pytest.mark.parametrize("kind", KINDS)
def test_packed_bytes_equal_the_hand_layout(kernels, kind):
    gk, rows = kernels[kind]
    assert [n for (_, n, _, _) in gk.args.members] == [r[1] for r in rows]
    assert gk.args.pack(_values(rows)) == _expected(rows)


def test_fused_args_resolved_against_the_plan(kernels):
    """The per-step path: pack_args resolves each member against the plan
    (and lead from the anchor's offset) into one positional pack."""
    gk, rows = kernels["fused"]
    v = _values(rows)
    plan = copy.copy(kernels["fused_plan"])
    plan.itershape, plan.global_start = (v["n0"],), (v["gs0"],)
    plan.operands = [copy.copy(o) for o in plan.operands]
    for o in plan.operands:
        o.offset0 = v[o.name + "_off"]
    plan.scalars = {n: (v[n], dt) for n, (_, dt) in plan.scalars.items()}
    ptrs = {"__partials__": v["partials"], "__npartials__": v["npartials"]}
    ptrs.update({o.name: v[o.name + "_p"] for o in plan.operands})
    assert codegen.pack_args(gk, plan, ptrs.__getitem__) == _expected(rows)


@pytest.mark.parametrize("kind", KINDS)
def test_mapping_rules(kernels, kind):
    gk, rows = kernels[kind]
    vals = _values(rows)
    extra = dict(vals, not_a_member=1, also_not=2.5)
    assert gk.args.pack(extra) == gk.args.pack(vals)
    for name in (rows[0][1], rows[len(rows) // 2][1], rows[-1][1]):
        short = dict(vals)
        del short[name]
        with pytest.raises(KeyError):
            gk.args.pack(short)


@pytest.fixture(scope="module")
def host_layout(kernels, tmp_path_factory):
    """kind -> [sizeof, offsetof of every member] from the host compiler."""
    cxx = _find_clangxx()
    if cxx is None:
        pytest.skip("no ROCm clang++ found")
    src = ["#include <cstddef>", "#include <cstdio>",
           "typedef long long i64;"]
    main = ["int main() {"]
    for kind in KINDS:
        gk, rows = kernels[kind]
        src.append(f"namespace ns_{kind} {{\n{gk.args.decl()}\n}}")
        ty = f"ns_{kind}::{gk.args.sname}"
        main.append(f'  printf("{kind} %zu", sizeof({ty}));')
        for row in rows:
            main.append(f'  printf(" %zu", offsetof({ty}, {row[1]}));')
        main.append('  printf("\\n");')
    main.append("  return 0;\n}")
    d = tmp_path_factory.mktemp("kernel_args_host")
    cpp, exe = d / "layout.cpp", d / "layout"
    cpp.write_text("\n".join(src + main) + "\n")
    subprocess.run([cxx, "-std=c++17", "-Wno-invalid-offsetof", str(cpp),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]]
            for ln in out.splitlines()}


@pytest.mark.parametrize("kind", KINDS)
def test_layout_against_the_compiler(kernels, host_layout, kind):
    gk, rows = kernels[kind]
    st = gk.args.struct
    codes = st.format[1:]
    assert codes == "".join(r[0] for r in rows)
    offsets = [struct.calcsize("<" + codes[:i]) for i in range(len(codes))]
    assert host_layout[kind] == [st.size] + offsets
    assert st.size == 8 * len(rows)
