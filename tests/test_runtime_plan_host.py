"""Planning a fused group is pure geometry: `Runtime._plan_group` makes no
backend call and needs no process group, so ONE process plans a group as
every rank of a world and checks what SPMD execution relies on but never
states: every rank derives the same exchange, launch units tile the rank's
box, messages come out of their sender's core and cover what the receiver
needs.  The Runtimes here have no backend (`None`): any backend call during
planning fails the test.

Also pins the shard-plan helpers of shardview.py to NumPy."""

import contextlib

import numpy as np
import pytest

from ramba_amd import common, deferred
from ramba_amd.common import contiguous_divisions
from ramba_amd.runtime import Runtime
from ramba_amd.shardview import (box_contains, box_intersect, box_rel,
                                 box_size, box_slices, c_strides,
                                 coord_offset, divisions_from_boxes,
                                 spans_trailing_axes)

WORLDS = (1, 2, 3, 4)
F64 = np.dtype(np.float64)


# ---------------------------------------------------------------------------
# building groups without running them
# ---------------------------------------------------------------------------

@contextlib.contextmanager
def planning_runtime(ra, world, rank):
    """The frontend bound to a backend-less Runtime of `world` ranks.
    `made` collects arrays posing as constructed; they are un-posed on exit
    so that their deletion frees nothing."""
    deferred.flush()
    prod = deferred.get_runtime()
    rt = Runtime(None, rank=rank, world=world)
    deferred.set_runtime(rt)
    made = []
    try:
        yield rt, made
    finally:
        deferred._state["group"] = None
        for a in made:
            a.bdarray.constructed = False
        deferred.set_runtime(prod)


def _constructed(ra, made, shape, dtype=np.float64, border=None,
                 distribution=None):
    """An array as an earlier flush left it: constructed, content unknown."""
    a = ra.empty(shape, dtype=dtype, local_border=border,
                 distribution=distribution)
    deferred._state["group"] = None     # drop the registration; nothing runs
    a.bdarray.constructed = True
    made.append(a)
    return a


def _chain(ra, made, world):
    A = ra.arange(4099) / 1000.0
    B = ra.sin(A)
    C = ra.cos(A)
    D = B * B + C ** 2
    return [A, B, C, D]


def _stencil2d(ra, made, world):
    X = _constructed(ra, made, (67, 131), np.float32, border=1)
    Y = _constructed(ra, made, (67, 131), np.float32, border=1)
    Y[1:-1, 1:-1] = (X[:-2, 1:-1] + X[2:, 1:-1] + X[1:-1, :-2]
                     + X[1:-1, 2:] - 4.0 * X[1:-1, 1:-1])
    return [X, Y]


def _wide_shift(ra, made, world):
    # a shift of 9 against the default border of 4: the read fits no border
    assert common.default_border < 9
    X = _constructed(ra, made, (4099,))
    Y = _constructed(ra, made, (4099,))
    Y[:-9] = X[9:] * 2.0
    return [X, Y]


def _reduction(ra, made, world):
    X = _constructed(ra, made, (4099,))
    pend = deferred.add_reduction(X[1:] + X[:-1], "sum", F64)
    return [X, pend]


def _few_rows(ra, made, world):
    # 3 rows, split by rows: from world 4 on a rank owns nothing
    divs = contiguous_divisions(world, (3, 37))
    X = _constructed(ra, made, (3, 37), distribution=divs)
    Y = _constructed(ra, made, (3, 37), distribution=divs)
    Y[1:] = X[:-1] + 1.0
    return [X, Y]


CASES = {"chain": _chain, "stencil2d": _stencil2d, "wide_shift": _wide_shift,
         "reduction": _reduction, "few_rows": _few_rows}


class Planned:
    """One rank's plan of one case, with what the checks need beside it."""

    def __init__(self, rt, group, live, recipe, keep):
        self.rt, self.group, self.live = rt, group, live
        self.recipe, self.keep = recipe, keep
        self.ebox = group.exec_boxes()[rt.rank]

    def msgs(self):
        """comm_msgs in a form comparable across ranks (a "border" target
        names a gid, which differs between two builds of the same program;
        the owner var names the same array)."""
        out = []
        for (dst, src, owner, bx, tgt) in self.recipe.comm_msgs:
            what = owner if tgt[0] == "border" else tgt[1]
            out.append((dst, src, owner, tuple(bx[0].tolist()),
                        tuple(bx[1].tolist()), tgt[0], what))
        return sorted(out)


def plan_world(ra, case, world):
    """The case planned as every rank of `world` (built afresh per rank:
    planning adopts partitions, which a second plan would find adopted)."""
    out = []
    for rank in range(world):
        with planning_runtime(ra, world, rank) as (rt, made):
            keep = CASES[case](ra, made, world)
            group = deferred._state["group"]
            deferred._state["group"] = None
            assert group is not None and group.producer is None
            live, dead = deferred.compute_live_vars(group)
            recipe = rt._plan_group(group, live, dead)
            out.append(Planned(rt, group, live, recipe, keep))
    return out


@pytest.fixture(scope="module")
def plans(ra):
    return {(case, world): plan_world(ra, case, world)
            for case in CASES for world in WORLDS}


def _unit_box(unit):
    lo = np.array(unit.plan.global_start, dtype=np.int64)
    return np.array([lo, lo + np.array(unit.plan.itershape) - 1])


# ---------------------------------------------------------------------------
# the cases exercise what they are meant to
# ---------------------------------------------------------------------------

def test_cases_reach_their_paths(plans):
    assert all(p.recipe.adopted_divs is not None
               for w in WORLDS for p in plans["chain", w])
    assert any(p.recipe.units is not None for p in plans["stencil2d", 4])
    assert all(not p.recipe.temp_specs for p in plans["wide_shift", 1])
    for w in (2, 3, 4):
        assert any(p.recipe.temp_specs for p in plans["wide_shift", w])
    for w in WORLDS:
        for p in plans["reduction", w]:
            assert len(p.recipe.plan.reductions) == 1
            assert p.recipe.units is None      # reductions stay sequential
    empty = [p for p in plans["few_rows", 4] if p.ebox is None]
    assert empty
    for p in empty:
        assert p.recipe.units is None
        assert p.recipe.plan.itershape is None


def test_unsplit_plan_is_addressed(plans):
    """What _run_recipe launches when `units` is None."""
    for ps in plans.values():
        for p in ps:
            plan = p.recipe.plan
            if p.recipe.units is not None or p.ebox is None:
                assert plan.itershape is None
                continue
            assert plan.itershape == tuple(
                (p.ebox[1] - p.ebox[0] + 1).tolist())
            assert plan.global_start == tuple(p.ebox[0].tolist())
            assert [o.name for o in plan.operands] == list(p.live)


# ---------------------------------------------------------------------------
# rank identity
# ---------------------------------------------------------------------------

def test_every_rank_plans_the_same_exchange(plans):
    for (case, world), ps in plans.items():
        first = ps[0].msgs()
        for p in ps[1:]:
            assert p.msgs() == first, (case, world, p.rt.rank)
        adopted = [p.recipe.adopted_divs for p in ps]
        for a in adopted[1:]:
            if adopted[0] is None:
                assert a is None, (case, world)
            else:
                assert np.array_equal(a, adopted[0]), (case, world)


# ---------------------------------------------------------------------------
# launch units
# ---------------------------------------------------------------------------

def test_units_tile_the_exec_box(plans):
    split = send_only = 0
    for (case, world), ps in plans.items():
        for p in ps:
            units = p.recipe.units
            if units is None:
                assert p.recipe.pre_wait_units == 0
                continue
            split += 1
            me = p.rt.rank
            assert p.recipe.pre_wait_units == 1
            boxes = [_unit_box(u) for u in units]
            for i, b in enumerate(boxes):
                assert box_contains(p.ebox, b), (case, world, me)
                for c in boxes[i + 1:]:
                    assert box_intersect(b, c) is None, (case, world, me)
            assert sum(box_size(b) for b in boxes) == box_size(p.ebox)
            # the unit launched before the wait reads owned cells only
            for oi in p.live.values():
                if oi.written:
                    continue
                need = oi.view.image_box(boxes[0])
                if need is not None:
                    core = p.rt.core_box(oi.bd, me)
                    assert core is not None and box_contains(core, need), \
                        (case, world, me, oi.name)
            if not any(m[0] == me for m in p.recipe.comm_msgs):
                send_only += 1
                assert len(units) == 1, (case, world, me)
    assert split and send_only      # neither loop body went unvisited


def test_no_units_without_overlap(ra, monkeypatch):
    monkeypatch.setattr(common, "overlap_exchange", 0)
    for case in CASES:
        for world in WORLDS:
            for p in plan_world(ra, case, world):
                assert p.recipe.units is None, (case, world, p.rt.rank)
                assert p.recipe.pre_wait_units == 0


# ---------------------------------------------------------------------------
# messages
# ---------------------------------------------------------------------------

def test_messages_come_from_the_senders_core(plans):
    seen = 0
    for (case, world), ps in plans.items():
        for p in ps:
            for (dst, src, owner, bx, tgt) in p.recipe.comm_msgs:
                seen += 1
                assert dst != src
                core = p.rt.core_box(p.live[owner].bd, src)
                assert core is not None and box_contains(core, bx), \
                    (case, world, dst, src)
    assert seen


def _fill_boxes(p):
    """Per owner var, the hull of the needs that spill out of the rank's
    core but fit its border ring: what the border exchange must fill."""
    fills = {}
    if p.ebox is None:
        return fills
    me = p.rt.rank
    for names in p.group.vars_by_gid.values():
        here = [p.live[n] for n in names if n in p.live]
        if not here:
            continue
        bd = here[0].bd
        core, ring = p.rt.core_box(bd, me), p.rt.border_box(bd, me)
        fit = []
        for oi in here:
            need = oi.view.image_box(p.ebox)
            if need is None or (core is not None
                                and box_contains(core, need)):
                continue
            if ring is not None and box_contains(ring, need):
                fit.append(need)
        if fit:
            fills[here[0].name] = (core, np.array(
                [np.min([b[0] for b in fit], axis=0),
                 np.max([b[1] for b in fit], axis=0)]))
    return fills


def test_border_messages_cover_the_fill_boxes(plans):
    seen = 0
    for (case, world), ps in plans.items():
        for p in ps:
            me = p.rt.rank
            for owner, (core, fill) in _fill_boxes(p).items():
                seen += 1
                parts = [bx for (dst, src, own, bx, tgt)
                         in p.recipe.comm_msgs
                         if dst == me and own == owner and tgt[0] == "border"]
                # cores are disjoint, so the pieces are: count the cells
                got = box_size(box_intersect(fill, core))
                got += sum(box_size(box_intersect(fill, bx)) for bx in parts)
                assert got == box_size(fill), (case, world, me, owner)
    assert seen


def test_temp_needs_are_tiled_exactly(plans):
    seen = 0
    for (case, world), ps in plans.items():
        for p in ps:
            me = p.rt.rank
            for (vname, shape, dtype, owner, need, part) \
                    in p.recipe.temp_specs:
                seen += 1
                assert shape == tuple((need[1] - need[0] + 1).tolist())
                assert np.array_equal(p.recipe.temp_geom[vname][0], need)
                assert p.recipe.temp_geom[vname][1] == c_strides(shape)
                pieces = [bx for (dst, src, own, bx, tgt)
                          in p.recipe.comm_msgs
                          if dst == me and tgt == ("temp", vname)]
                if part is not None:
                    pieces.append(part)
                for i, b in enumerate(pieces):
                    assert box_contains(need, b)
                    for c in pieces[i + 1:]:
                        assert box_intersect(b, c) is None
                assert sum(box_size(b) for b in pieces) == box_size(need), \
                    (case, world, me, vname)
    assert seen


# ---------------------------------------------------------------------------
# shard-plan helpers against NumPy
# ---------------------------------------------------------------------------

def _box(lo, hi):
    return np.array([lo, hi], dtype=np.int64)


@pytest.mark.parametrize("shape", [(), (7,), (1,), (4, 1, 3), (2, 3, 5, 7),
                                   (67, 131)])
def test_c_strides_matches_numpy(shape):
    a = np.empty(shape, dtype=np.float64)
    assert c_strides(shape) == tuple(s // a.itemsize for s in a.strides)


@pytest.mark.parametrize("shape", [(0,), (0, 5), (3, 0, 4), (2, 3, 0)])
def test_c_strides_of_a_zero_extent_shape(shape):
    """No element of such an array is addressable and NumPy's own strides
    for it are unspecified (all zero in NumPy 2, the row-major recurrence
    before), so the recurrence itself is pinned: stride[i] =
    stride[i+1] * shape[i+1], innermost 1, and a reshape NumPy accepts."""
    st = c_strides(shape)
    assert st[-1] == 1
    for i in range(len(shape) - 1):
        assert st[i] == st[i + 1] * shape[i + 1]
    v = np.lib.stride_tricks.as_strided(
        np.empty(0), shape=shape, strides=tuple(8 * s for s in st))
    assert v.shape == shape and v.size == 0


def test_box_slices_and_box_rel_match_numpy():
    a = np.arange(6 * 7 * 5).reshape(6, 7, 5)
    b = _box([1, 0, 2], [4, 6, 2])
    assert np.array_equal(a[box_slices(b)], a[1:5, 0:7, 2:3])
    # the same cells through a window of `a` whose first cell is `origin`
    origin = np.array([1, 0, 1])
    win = a[1:, 0:, 1:]
    assert np.array_equal(win[box_slices(b, origin)], a[box_slices(b)])
    rel = box_rel(b, origin)
    assert rel.dtype == np.int64 and rel.tolist() == [[0, 0, 1], [3, 6, 1]]
    assert b.tolist() == [[1, 0, 2], [4, 6, 2]]          # input untouched
    assert box_slices(_box([3], [3])) == (slice(3, 4),)
    assert box_slices(np.zeros((2, 0), dtype=np.int64)) == ()


def test_spans_trailing_axes_matches_c_contiguity():
    shape = (5, 4, 3)
    a = np.empty(shape)
    for lo, hi in [([0, 0, 0], [4, 3, 2]), ([2, 0, 0], [3, 3, 2]),
                   ([2, 1, 0], [3, 3, 2]), ([0, 0, 0], [4, 3, 1]),
                   ([1, 0, 1], [1, 3, 2])]:
        b = _box(lo, hi)
        # one C-order interval <=> the slice is a C-contiguous block
        assert spans_trailing_axes(b, shape) == \
            a[box_slices(b)].flags["C_CONTIGUOUS"], (lo, hi)
    assert spans_trailing_axes(_box([2], [3]), (9,))        # 1-D: always
    # a 0-extent trailing axis has no full-extent box (hi would be -1 ...)
    assert spans_trailing_axes(_box([0, 0], [2, -1]), (3, 0))
    assert not spans_trailing_axes(_box([0, 0], [2, 0]), (3, 0))


def test_divisions_from_boxes_with_an_empty_rank():
    boxes = [_box([0, 0], [1, 4]), None, _box([2, 0], [2, 4])]
    divs = divisions_from_boxes(boxes, 2)
    assert divs.shape == (3, 2, 2) and divs.dtype == np.int64
    assert divs[0].tolist() == [[0, 0], [1, 4]]
    assert divs[1].tolist() == [[0, 0], [-1, -1]]           # hi < lo: empty
    assert divs[2].tolist() == [[2, 0], [2, 4]]
    rt = Runtime(None, rank=1, world=3)
    bd = deferred.bdarray((3, 5), F64, divs, 0, flex=False)
    assert rt.core_box(bd, 1) is None
    assert np.array_equal(rt.core_box(bd, 2), boxes[2])
    # round trip through the runtime's own reading of divisions
    back = [rt.core_box(bd, r) for r in range(3)]
    assert np.array_equal(divisions_from_boxes(back, 2), divs)
    assert divisions_from_boxes([None, None], 1).tolist() == \
        [[[0], [-1]], [[0], [-1]]]


def test_coord_offset_and_local_addressing_match_numpy():
    """Offsets into a padded container, checked by reading one through
    NumPy: the container of rank 1's shard of a (9, 10) array."""
    divs = divisions_from_boxes([_box([0, 0], [3, 9]), _box([4, 0], [8, 9])],
                                2)
    bd = deferred.bdarray((9, 10), F64, divs, 2, flex=False)
    rt = Runtime(None, rank=1, world=2)
    d, cshape, cstrides, pads = rt.shard_geometry(bd)
    assert cstrides == c_strides(cshape)
    cont = np.arange(int(np.prod(cshape))).reshape(cshape)
    for coord in ([4, 0], [6, 7], [8, 9], [2, 0]):          # last: in the ring
        off = coord_offset(coord, d[0], pads, cstrides)
        assert cont.reshape(-1)[off] == cont[coord[0] - 4 + pads[0],
                                             coord[1] - 0 + pads[1]]
    from ramba_amd.shardview import View
    v = View.identity((9, 10)).apply_index((slice(1, None), slice(2, 8, 2)))
    lb = _box([4, 1], [7, 2])           # view box; rows 5..8, cols 4 and 6
    off0, strides = rt.local_addressing(bd, v, lb)
    got = np.lib.stride_tricks.as_strided(
        cont.reshape(-1)[off0:], shape=(4, 2),
        strides=tuple(s * cont.itemsize for s in strides))
    want = cont[rt.container_slice(bd, _box([5, 4], [8, 6]))][:, ::2]
    assert np.array_equal(got, want)
