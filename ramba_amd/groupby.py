"""groupby reductions: the `Groupby` object, the CSR of the labels, and the
portable host hook.

`ndarray.groupby(dim, value_to_group, num_groups)` is the reference's
RambaGroupby (ramba/ramba.py:6896, 10290-10607): the rows of axis `dim`
carry one integer label each, and every method reduces the rows of a label
into one row of the result, whose shape is the input's with shape[dim]
replaced by num_groups.  `runtime.group_op` reduces each rank's box through
one backend hook:

    group_partial(bd, rt, view, lb, dim, members, seg, ngroups, op, skipna)
        -> the rank's partial over its view-space box `lb`, a dense torch
        tensor shaped like the box with ngroups rows on `dim`;
        members, seg: the CSR of the box's rows (build_csr), host int32;
        op: SUM, PROD, MIN, MAX or COUNT_VALID (the int64 number of non-NaN
            members); skipna: a NaN counts as the identity.

`HipBackend` implements it on the rt_group_reduce kernels.  A backend without
it (the NumPy oracle backend, which is frozen test infrastructure) gets
`HostGroup`, built only on box_to_numpy and the np.<ufunc>.at functions,
which are also the definition of every result: floats accumulate in their
own dtype, integers and bool in int64 with wrap-around for SUM / PROD, MIN /
MAX keep the dtype (bool as uint8), an empty group holds the identity.
"""

import numpy as np

from .shardview import box_shape, c_strides

SUM, PROD, MIN, MAX, COUNT_VALID = range(5)
COMBINE = {SUM: "sum", PROD: "prod", MIN: "min", MAX: "max",
           COUNT_VALID: "sum"}
_UFUNC = {SUM: np.add, PROD: np.multiply, MIN: np.minimum, MAX: np.maximum,
          COUNT_VALID: np.add}


def acc_dtype(dtype, op):
    """dtype of a partial and of the result's storage (bool as uint8)."""
    dtype = np.dtype(dtype)
    if op == COUNT_VALID or (op in (SUM, PROD) and dtype.kind != "f"):
        return np.dtype(np.int64)
    return np.dtype(np.uint8) if dtype == np.bool_ else dtype


def result_dtype(dtype, op):
    """dtype of the array a reduction returns (MIN / MAX of bool is bool)."""
    return np.dtype(dtype) if op in (MIN, MAX) else acc_dtype(dtype, op)


def identity(dtype, op):
    """What an empty group holds, as a scalar of acc_dtype(dtype, op)."""
    dt = acc_dtype(dtype, op)
    if op in (SUM, COUNT_VALID):
        return dt.type(0)
    if op == PROD:
        return dt.type(1)
    if dt.kind == "f":
        return dt.type(np.inf if op == MIN else -np.inf)
    if np.dtype(dtype) == np.bool_:
        return dt.type(op == MIN)
    info = np.iinfo(dt)
    return dt.type(info.max if op == MIN else info.min)


def build_csr(labels, ngroups):
    """(members, seg) of a validated 1-D label array: the row numbers stably
    sorted by label, and ngroups + 1 offsets, both int32.  A stable counting
    sort: NumPy's stable sort of 16-bit keys is a radix sort, O(len); with
    more than 2**16 groups it is a merge sort."""
    labels = np.asarray(labels)
    key = labels.astype(np.uint16) if ngroups <= 1 << 16 else labels
    members = np.argsort(key, kind="stable").astype(np.int32)
    seg = np.zeros(ngroups + 1, dtype=np.int64)
    np.cumsum(np.bincount(labels, minlength=ngroups), out=seg[1:])
    return members, seg.astype(np.int32)


def hooks_for(backend):
    """The object serving the hook for `backend`."""
    if hasattr(backend, "group_partial"):
        return backend
    return HostGroup(backend)


class HostGroup:
    """Portable host implementation of the groupby hook."""

    def __init__(self, backend):
        self.backend = backend

    def group_partial(self, bd, rt, view, lb, dim, members, seg, ngroups, op,
                      skipna):
        import torch
        core = rt.core_box(bd, rt.rank)
        local = self.backend.box_to_numpy(bd, rt, core)
        # the operand is read in place through the view's strides
        off0, strides = view.operand_addressing(
            lb[0], c_strides(local.shape), core[0], (0,) * local.ndim)
        flat = local.reshape(-1)
        x = np.lib.stride_tricks.as_strided(
            flat[off0:] if off0 else flat, shape=box_shape(lb),
            strides=tuple(s * local.itemsize for s in strides))
        x = np.moveaxis(x, dim, 0)
        labels = np.empty(x.shape[0], dtype=np.int64)
        labels[members] = np.repeat(np.arange(ngroups), np.diff(seg))
        dt, ident = acc_dtype(bd.dtype, op), identity(bd.dtype, op)
        if op == COUNT_VALID:
            vals = (x == x).astype(dt)
        else:
            vals = x.astype(dt)
            if skipna and dt.kind == "f":
                vals = np.where(np.isnan(vals), ident, vals)
        out = np.full((ngroups,) + x.shape[1:], ident, dtype=dt)
        _UFUNC[op].at(out, labels, vals)
        return torch.from_numpy(np.ascontiguousarray(np.moveaxis(out, 0, dim)))


def _labels_to_host(value_to_group):
    if hasattr(value_to_group, "asarray"):        # a ramba array
        return np.asarray(value_to_group.asarray())
    return np.asarray(value_to_group)


class Groupby:
    """The rows of axis `dim` of `array`, grouped by the integer labels
    `value_to_group` (a NumPy array, a list or a ramba array of length
    shape[dim]; brought to the host, as the reference does).  num_groups=None
    means max(label) + 1; the reference takes `max()` there, one short, so
    that its last group is out of range.  Every method returns a ramba array
    shaped like the input with shape[dim] replaced by num_groups, and takes
    the reference's ignored `dim=None`."""

    def __init__(self, array, dim, value_to_group, num_groups=None):
        if array.dtype.kind == "c":
            raise NotImplementedError("groupby: complex input is not "
                                      "supported")
        if array.ndim > 4:
            raise NotImplementedError(
                "groupby supports arrays of up to 4 dimensions")
        if array.dtype.kind not in "fib" or array.dtype.itemsize > 8 \
                or array.dtype == np.float16:
            raise NotImplementedError(
                f"groupby: dtype {array.dtype} is not supported")
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) \
                or not 0 <= dim < array.ndim:
            raise ValueError(f"groupby: dim={dim!r} is out of range for an "
                             f"array of {array.ndim} dimension(s)")
        labels = _labels_to_host(value_to_group)
        if labels.dtype.kind not in "iu" and labels.size:   # [] is float64
            raise ValueError("groupby: value_to_group must be an integer "
                             f"array, not {labels.dtype}")
        if labels.shape != (array.shape[dim],):
            raise ValueError(
                f"groupby: value_to_group has shape {labels.shape}, expected "
                f"({array.shape[dim]},) for dim={dim}")
        if num_groups is None:
            num_groups = int(labels.max()) + 1 if labels.size else 0
        num_groups = int(num_groups)
        if num_groups < 1:
            raise ValueError(f"groupby: num_groups={num_groups} must be at "
                             "least 1")
        if labels.size and (int(labels.min()) < 0
                            or int(labels.max()) >= num_groups):
            raise ValueError(
                f"groupby: labels must lie in [0, {num_groups}); got "
                f"{int(labels.min())} .. {int(labels.max())}")
        self.array, self.dim, self.num_groups = array, int(dim), num_groups
        self.labels = labels.astype(np.int64)

    @property
    def _out_shape(self):
        shape = list(self.array.shape)
        shape[self.dim] = self.num_groups
        return tuple(shape)

    def _reduce(self, op, skipna=False):
        from . import deferred
        from .ndarray import _from_bd, full
        if self.array.size == 0:
            return full(self._out_shape, identity(self.array.dtype, op),
                        dtype=result_dtype(self.array.dtype, op))
        deferred.flush()
        return _from_bd(deferred.get_runtime().group_op(
            self.array, self.dim, self.labels, self.num_groups, op, skipna))

    def sum(self, dim=None):
        return self._reduce(SUM)

    def prod(self, dim=None):
        return self._reduce(PROD)

    def min(self, dim=None):
        return self._reduce(MIN)

    def max(self, dim=None):
        return self._reduce(MAX)

    def count(self, dim=None):
        """The int64 number of members of each group, broadcast to the
        result's shape (host arithmetic on the labels)."""
        from .ndarray import fromarray
        shape = [1] * self.array.ndim
        shape[self.dim] = self.num_groups
        counts = np.bincount(self.labels, minlength=self.num_groups)
        return fromarray(counts.astype(np.int64).reshape(shape)) \
            .broadcast_to(self._out_shape)

    def _ratio(self, total, count):
        """total / count: in the dtype of a float input, in float64 for an
        integer one; 0 / 0 is NaN, without NumPy's warning."""
        from . import deferred
        if total.dtype.kind == "f":
            count = count.astype(total.dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = total / count
            deferred.flush()
        return out

    def mean(self, dim=None, ret_separate=False):
        total, count = self.sum(), self.count()
        return (total, count) if ret_separate else self._ratio(total, count)

    def nanmean(self, dim=None, ret_separate=False):
        """mean over the members that are not NaN; both the sum and the
        int64 count of such members come from the kernel."""
        total = self._reduce(SUM, skipna=True)
        count = self._reduce(COUNT_VALID)
        return (total, count) if ret_separate else self._ratio(total, count)

    def var(self, dim=None):
        """Population variance (ddof=0, as the reference): the grouped sum
        of (a - mean[label]) ** 2 over the count."""
        from .ndarray import take
        spread = self.array - take(self.mean(), self.labels, axis=self.dim)
        return self._ratio(
            Groupby(spread * spread, self.dim, self.labels,
                    self.num_groups).sum(), self.count())

    def std(self, dim=None):
        return self.var() ** 0.5
