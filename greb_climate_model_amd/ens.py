"""Ensemble output: the statistics across the members of a group of every monthly record, made on the device along the
member axis -- of the records themselves or of each member's difference to its control member.

The member axis is what makes the output of a many-member run big, and what its user looks at is a spread: the median
and the 5-95 % range of the response per grid point.  A plan puts each member into a group (-1: none) and optionally
names its control; per group, csrc/greb_ens.hip takes mean, sample variance, min and max in one pass over the staging
slot a model year was integrated into, and the quantiles by a sort in LDS (include/greb_engine.h: greb_ens_*,
greb_engine_run_ens):

    pairs = 256                                   # members 0 ... 255 at control CO2, 256 ... 511 the same physics at 2 x CO2
    group = [-1] * pairs + [0] * pairs            # the control members are in no group, their partners are group 0
    control = [-1] * pairs + list(range(pairs))   # member 256 + k responds to member k
    plan = ens.Plan(nx, ny, 2 * pairs, group, control=control, probs=(0.05, 0.5, 0.95))
    res = engine.Engine(inp, p, members=...).run_ens(100, co2, plan)
    res.quant[0, :, 1, 11, 0]                     # [years][ny][nx]: the median December Tsurf response
    ens.Plan(nx, ny, 2 * pairs, [0] * pairs + [1] * pairs)   # no control map: the statistics of the records themselves

reference() is the numpy statement of the products: the same IEEE operations in the same order as the kernels, so the
tests hold the device to it bit for bit.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _plan, abi

MOMENTS = abi.S_MEAN | abi.S_VAR | abi.S_RANGE
ALL = MOMENTS | abi.S_QUANTILES
PRODUCTS = ("mean", "var", "min", "max", "quant")


def selected(what: int) -> tuple:
    """Which of PRODUCTS the flags `what` (abi.S_*) deliver, as five booleans."""
    rng = bool(what & abi.S_RANGE)
    return (bool(what & abi.S_MEAN), bool(what & abi.S_VAR), rng, rng, bool(what & abi.S_QUANTILES))


def empty_products(plan, lead: tuple, rec: tuple) -> list:
    """Host arrays for the plan's products, [n_groups] + lead + rec (quant: [n_groups] + lead + [n_probs] + rec); None
    where not selected."""
    shape = lambda i: (plan.ng,) + tuple(lead) + ((len(plan.probs),) if i == 4 else ()) + tuple(rec)
    return [np.empty(shape(i), np.float32) if on else None for i, on in enumerate(selected(plan.what))]


@dataclass
class Result:
    """What run_ens / reduce_dev / reference hand back; a product that was not selected is None.  mean, var, min, max
    [n_groups][..]; quant [n_groups][..][n_probs][record] from Engine.run_ens (`..` = [years], record = [12][5][ny][nx]),
    [n_groups][n_probs][..] from reduce_dev and reference.  var is the sample variance (ddof = 1; 0 for a group of one)."""
    mean: object
    var: object
    min: object
    max: object
    quant: object
    yearly: object = None
    vars: tuple = None  # the names of the variables (the axis the shapes call [5]) where the run knows them

    @property
    def std(self):
        """The sample standard deviation: the square root of `var`, taken on the host (numpy array or torch tensor)."""
        if self.var is None:
            return None
        return np.sqrt(self.var) if isinstance(self.var, np.ndarray) else self.var.sqrt()


class Plan(_plan.Handle):
    """greb_ens handle: grid, member count, each member's group (-1: in none; groups are 0 ... max(group)), each member's
    control member (None: no control map -- the statistics are of the records themselves), the probabilities of the
    quantiles and the products (abi.S_* bits; default: MEAN, VAR and RANGE, and QUANTILES when probs are given).  Host data
    only; creating one needs no GPU, and every argument error is a GrebError(-1) naming the offender (-4: a group of more
    than 4096 members with quantiles)."""
    _destroy = "greb_ens_destroy"

    def __init__(self, nx: int, ny: int, n_members: int, group, control=None, probs=(), what: int | None = None):
        from . import engine
        self.nx, self.ny, self.nm = int(nx), int(ny), int(n_members)
        self.probs = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, np.float32)))
        if self.probs.ndim != 1:
            raise engine.GrebError(-1, "ens.Plan: probs must be a list of probabilities")
        if what is None:
            what = MOMENTS | (abi.S_QUANTILES if len(self.probs) else 0)
        self.what = int(what)

        def members(name, a):
            a = np.asarray(a)
            if a.shape != (max(self.nm, 0),) or (a.size and a.dtype.kind not in "iu"):
                raise engine.GrebError(-1, f"ens.Plan: {name} must hold {self.nm} integers, one per member")
            return np.ascontiguousarray(a, np.int32)

        self.group = members("group", group)
        self.control = None if control is None else members("control", control)
        self.ng = int(self.group.max()) + 1 if self.group.size else 0
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        self._create("greb_ens_create", self.nx, self.ny, self.nm, ip(self.group), self.ng, ip(self.control),
                     abi.fptr(self.probs) if len(self.probs) else None, len(self.probs), self.what & 0xFFFFFFFF)


def reduce_dev(plan: Plan, x) -> Result:
    """The plan's statistics of a contiguous float32 GPU tensor [n_members][...] (any trailing shape), as torch tensors
    [n_groups][...] (quant [n_groups][n_probs][...]) on the same device, on torch's current stream, without synchronising
    (greb_ens_reduce_dev)."""
    import torch
    from . import engine
    dev = _plan.gpu_tensor_check(x, x.dim() >= 1 and x.shape[0] == plan.nm and x.numel() > 0, "ens.reduce_dev", f"[{plan.nm}][...]")
    rec = tuple(x.shape[1:])
    n = x.numel() // plan.nm
    out = [torch.empty((plan.ng,) + ((len(plan.probs),) if i == 4 else ()) + rec, dtype=torch.float32, device=f"cuda:{dev}")
           if on else None for i, on in enumerate(selected(plan.what))]
    _plan.call_on_current_stream(dev, engine.lib().greb_ens_reduce_dev, plan.h, int(dev), _plan.ptr(x), n, *map(_plan.ptr, out))
    return Result(*out)


def reference(x, group, control=None, probs=(), what: int | None = None) -> Result:
    """The products in numpy, operation by operation as csrc/greb_ens.hip performs them (include/greb_engine.h states
    them): x [n_members][...] float32, group [n_members] (-1: none), control [n_members] or None, probs the quantiles'
    probabilities.  Returns a Result of float32 arrays [n_groups][...] (quant [n_groups][n_probs][...]); products not in
    `what` are None.  Loops over a group's members in ascending order, vectorised over the elements."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 1:
        raise ValueError("reference: float32 x [n_members][...] expected")
    group = np.asarray(group, np.int64)
    ctl = None if control is None else np.asarray(control, np.int64)
    probs = np.atleast_1d(np.asarray(probs, np.float32))
    if group.shape != (x.shape[0],) or (ctl is not None and ctl.shape != group.shape):
        raise ValueError("reference: one group (and control) index per member")
    if what is None:
        what = MOMENTS | (abi.S_QUANTILES if len(probs) else 0)
    sel = selected(what)
    ng = int(group.max()) + 1
    rec = x.shape[1:]
    out = [np.empty((ng,) + ((len(probs),) if i == 4 else ()) + rec, np.float32) if on else None for i, on in enumerate(sel)]
    for g in range(ng):
        members = np.flatnonzero(group == g)  # ascending
        if not len(members):
            raise ValueError(f"reference: group {g} is empty")
        # the sample: one fp32 subtraction
        sample = lambda m: x[m] if ctl is None else x[m] - x[ctl[m]]
        n = np.float64(len(members))
        S = np.zeros(rec, np.float64)
        S1, S2 = np.zeros(rec, np.float64), np.zeros(rec, np.float64)
        K = sample(members[0]).astype(np.float64)
        lo, hi = np.full(rec, np.inf, np.float32), np.full(rec, -np.inf, np.float32)
        for m in members:
            v = sample(m)
            assert v.dtype == np.float32
            v64 = v.astype(np.float64)
            S = S + v64
            d = v64 - K
            S1 = S1 + d
            S2 = S2 + d * d
            lo, hi = np.minimum(lo, v), np.maximum(hi, v)
        if sel[0]:
            out[0][g] = (S / n).astype(np.float32)
        if sel[1]:
            if len(members) > 1:
                var = (S2 - S1 * S1 / n) / (n - np.float64(1.0))
                out[1][g] = np.where(var < 0.0, 0.0, var).astype(np.float32)
            else:
                out[1][g] = 0.0
        if sel[2]:
            out[2][g], out[3][g] = lo, hi
        if sel[4]:
            v = np.sort(np.stack([sample(m) for m in members]), axis=0)  # [n_g][...] float32, ascending
            for q, p in enumerate(probs):
                h = np.float64(p) * np.float64(len(members) - 1)
                i = min(max(int(np.floor(h)), 0), len(members) - 1)
                t = h - np.float64(i)
                a, b = v[i].astype(np.float64), v[min(i + 1, len(members) - 1)].astype(np.float64)
                out[4][g, q] = (a + t * (b - a)).astype(np.float32)
    return Result(*out)
