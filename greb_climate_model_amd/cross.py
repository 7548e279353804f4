"""Crossing output: WHEN members pass thresholds, made on the device along the time axis.

clim.Plan reduces the years linearly -- means, seasons, trends.  In which year each member's annual-mean warming passes
2 K and whether it stays there, in which year September's albedo first falls below 0.4, in what share of a
perturbed-physics ensemble that has happened by year y: a threshold is not linear in the record, so none of the other
plans' products give it.  Here each model year updates a few state words per (member, event, point) in the device staging
slot it was integrated into (csrc/greb_cross.hip; include/greb_engine.h: greb_cross_*, greb_engine_run_cross), and what
comes back is a handful of maps per member and event, whatever the length of the run:

    M = 256                                                           # member m rises 1 %/yr, member M + m is its control
    events = [cross.Event(0, cross.ANN, 1.5, rel=True), cross.Event(0, cross.ANN, 2.0, rel=True),
              cross.Event(4, cross.SEP, 0.4, dir=-1)]                 # Tsurf response >= 1.5 K, >= 2 K; September albedo <= 0.4
    plan = cross.Plan(nx, ny, 2 * M, events, control=list(range(M, 2 * M)) * 2, group=[0] * M + [-1] * M)
    res = eng.run_cross(100, co2, plan)
    cross.as_year(res.first[:M, 1], 1940)                             # [M][ny][nx]: the year each member first passes 2 K
    res.fraction[:, 0, 1]                                             # [100][ny][nx]: the share of the members above 2 K

reference() is the numpy statement of the products: the same IEEE operations in the same order as the kernels, so the
tests hold the device to it for equal integers and equal float bits.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _plan, abi

JAN, FEB, MAR, APR, MAY, JUN, JUL, AUG, SEP, OCT, NOV, DEC = range(12)
DJF, MAM, JJA, SON, ANN = range(12, 17)
SELECTORS = ("JAN", "FEB", "MAR", "APR", "MAY", "JUN", "JUL", "AUG", "SEP", "OCT", "NOV", "DEC", "DJF", "MAM", "JJA", "SON", "ANN")
# the months of each season in the order they are added (DJF: Dec, Jan, Feb of the same model year), as clim.SEASON_MONTHS
SEASON_MONTHS = ((11, 0, 1), (2, 3, 4), (5, 6, 7), (8, 9, 10), tuple(range(12)))
MAPS = abi.T_FIRST | abi.T_LAST | abi.T_STAY | abi.T_COUNT | abi.T_PEAK
ALL = MAPS | abi.T_FRACTION
PRODUCTS = ("first", "last", "stay", "count", "peak", "peak_year", "fraction")
_FLAGS = (abi.T_FIRST, abi.T_LAST, abi.T_STAY, abi.T_COUNT, abi.T_PEAK, abi.T_PEAK, abi.T_FRACTION)


@dataclass
class Event:
    """One event: variable `var` of the records, selector `sel` (JAN ... DEC, DJF ... ANN), threshold `thr`, direction `dir`
    (+1: a hit is q >= thr, -1: q <= thr) and `rel` (the quantity is the member minus its control)."""
    var: int
    sel: int
    thr: float
    dir: int = +1
    rel: bool = False


@dataclass
class Result:
    """What run_cross / finish_dev / reference hand back; a product that was not selected is None.  first, last, stay,
    count, peak_year int32 and peak float32 [n_members][n_events][ny][nx], years 0-based (-1: never); fraction float32
    [years][n_groups][n_events][ny][nx] (from add_year_dev: one year's [n_groups][n_events][ny][nx])."""
    first: object
    last: object
    stay: object
    count: object
    peak: object
    peak_year: object
    fraction: object = None
    yearly: object = None
    vars: tuple = None  # the names of the variables of the records where the run knows them


def selected(what: int) -> tuple:
    """Which of PRODUCTS the flags `what` (abi.T_*) deliver, as seven booleans."""
    return tuple(bool(what & f) for f in _FLAGS)


def memory_bytes(what: int, n_members: int, n_events: int, ny: int, nx: int, n_groups: int = 0) -> int:
    """Device memory of a plan: 4 bytes per selected state word (PEAK has two) per (member, event, point); FRACTION adds
    one hit byte each and two output slots [n_groups][n_events][ny][nx] of floats.  Nothing grows with the years."""
    el = n_members * n_events * ny * nx
    words = sum(bool(what & f) for f in (abi.T_FIRST, abi.T_LAST, abi.T_STAY, abi.T_COUNT)) + (2 if what & abi.T_PEAK else 0)
    return 4 * words * el + ((el + 8 * n_groups * n_events * ny * nx) if what & abi.T_FRACTION else 0)


class Plan(_plan.Handle):
    """greb_cross handle: grid, member count, 1 ... 16 events, the variables per month of the records (5: a year of state
    records), each member's control member (-1: none; None: no control map), each member's group (-1: in none; None: no
    group map) and the products (abi.T_* bits; default: the five maps, and FRACTION when there is a group map).  Host data
    only; creating one needs no GPU, and every argument error is a GrebError(-1) naming the offender.  Device memory:
    memory_bytes() -- 24 bytes per (member, event, point) for all five maps."""
    _destroy = "greb_cross_destroy"

    def __init__(self, nx: int, ny: int, n_members: int, events, n_vars: int = 5, control=None, group=None, what: int | None = None,
                 n_groups: int | None = None):
        from . import engine
        self.nx, self.ny, self.nm, self.nv = int(nx), int(ny), int(n_members), int(n_vars)
        self.events = [ev if isinstance(ev, Event) else Event(*ev) for ev in events]
        self.ne = len(self.events)

        def ints(name, a):
            a = np.asarray(a)
            if a.shape != (max(self.nm, 0),) or (a.size and a.dtype.kind not in "iu"):
                raise engine.GrebError(-1, f"cross.Plan: {name} must hold {self.nm} integers, one per member")
            return np.ascontiguousarray(a, np.int32)

        self.control = None if control is None else ints("control", control)
        self.group = None if group is None else ints("group", group)
        self.ng = 0 if self.group is None else (int(n_groups) if n_groups is not None else int(self.group.max()) + 1 if self.group.size else 0)
        if what is None:
            what = ALL if self.group is not None else MAPS
        self.what = int(what)
        evs = (abi.GrebCrossEvent * max(self.ne, 1))()
        for c, ev in zip(evs, self.events):
            c.var, c.sel, c.rel, c.dir, c.thr = int(ev.var), int(ev.sel), int(ev.rel), int(ev.dir), float(ev.thr)
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        self._create("greb_cross_create", self.nx, self.ny, self.nm, self.nv, evs, self.ne, ip(self.control), ip(self.group), self.ng,
                     C.c_uint(self.what & 0xFFFFFFFF))

    def describe(self) -> str:
        mb = memory_bytes(self.what, self.nm, self.ne, self.ny, self.nx, self.ng) / 1e6
        names = [n for n, on in zip(PRODUCTS, selected(self.what)) if on]
        return (f"cross.Plan: {self.nm} members x {self.ne} events at {self.nx} x {self.ny}, products {', '.join(names)}: "
                f"{mb:.1f} MB of device memory, whatever the number of years")


def empty_products(plan: Plan, years: int) -> list:
    """Host arrays for the selected products of a run of `years` years (None where not selected), in PRODUCTS' order."""
    shape = (plan.nm, plan.ne, plan.ny, plan.nx)
    dtypes = (np.int32, np.int32, np.int32, np.int32, np.float32, np.int32)
    out = [np.empty(shape, dt) if on else None for dt, on in zip(dtypes, selected(plan.what))]
    out.append(np.empty((years, plan.ng, plan.ne, plan.ny, plan.nx), np.float32) if plan.what & abi.T_FRACTION else None)
    return out


def add_year_dev(plan: Plan, x, k: int):
    """Year k (0-based) of the current period, a contiguous float32 GPU tensor [n_members][12][plan.nv][ny][nx], into the
    plan's state where it is (greb_cross_add_year_dev) on torch's current stream, without synchronising.  Returns that
    year's fraction [n_groups][n_events][ny][nx] as a torch tensor where the plan selects FRACTION, else None."""
    import torch
    from . import engine
    want = (plan.nm, 12, plan.nv, plan.ny, plan.nx)
    dev = _plan.gpu_tensor_check(x, tuple(x.shape) == want, "cross.add_year_dev", str(list(want)))
    frac = None
    if plan.what & abi.T_FRACTION:
        frac = torch.empty((plan.ng, plan.ne, plan.ny, plan.nx), dtype=torch.float32, device=f"cuda:{dev}")
    _plan.call_on_current_stream(dev, engine.lib().greb_cross_add_year_dev, plan.h, int(dev), _plan.ptr(x), int(k), _plan.ptr(frac))
    plan._device = dev
    return frac


def finish_dev(plan: Plan, n_years: int) -> Result:
    """The maps of the n_years years added since the last finish (greb_cross_finish_dev), torch tensors
    [n_members][n_events][ny][nx] on the device of the years, on torch's current stream, without synchronising."""
    import torch
    from . import engine
    dev = getattr(plan, "_device", None)
    if dev is None:
        raise engine.GrebError(-1, "cross.finish_dev: no year was added to this plan")
    shape = (plan.nm, plan.ne, plan.ny, plan.nx)
    dtypes = (torch.int32, torch.int32, torch.int32, torch.int32, torch.float32, torch.int32)
    out = [torch.empty(shape, dtype=dt, device=f"cuda:{dev}") if on else None for dt, on in zip(dtypes, selected(plan.what))]
    _plan.call_on_current_stream(dev, engine.lib().greb_cross_finish_dev, plan.h, int(dev), int(n_years), *map(_plan.ptr, out))
    return Result(*out)


def quantity(year, ev: Event, control=None) -> np.ndarray:
    """The year's quantity q of event `ev`, [n_members][ny][nx] float32, from one model year [n_members][12][V][ny][nx]
    float32, operation by operation as include/greb_engine.h states it."""
    x = np.asarray(year)
    if x.dtype != np.float32 or x.ndim != 5 or x.shape[1] != 12:
        raise ValueError("quantity: a float32 year [n_members][12][V][ny][nx] expected")
    if ev.sel < 12:
        a = x[:, ev.sel, ev.var]
    else:
        months = SEASON_MONTHS[ev.sel - 12]
        acc = np.zeros(x[:, 0, ev.var].shape, np.float64)
        for mo in months:  # multiply, then add: never fused
            acc = acc + np.float64(abi.JDAY_MON[mo]) * x[:, mo, ev.var].astype(np.float64)
        a = (acc / np.float64(sum(abi.JDAY_MON[mo] for mo in months))).astype(np.float32)
    if not ev.rel:
        return np.ascontiguousarray(a)
    if control is None:
        raise ValueError("quantity: a `rel` event needs a control map")
    ctl = np.asarray(control, np.int64)
    has = ctl >= 0
    with np.errstate(invalid="ignore"):
        d = a - a[np.where(has, ctl, 0)]  # ONE fp32 subtraction
    assert d.dtype == np.float32
    return np.where(has[:, None, None], d, np.float32(np.nan)).astype(np.float32)


def reference(x, events, control=None, group=None, n_groups: int | None = None) -> Result:
    """The products in numpy, operation by operation as include/greb_engine.h states them: x [years][n_members][12][V][ny][nx]
    float32 (any sequence of years), events a list of Event, control / group [n_members] or None.  Returns a Result of all
    five maps, and of fraction [years][n_groups][n_events][ny][nx] where a group map is given."""
    events = [ev if isinstance(ev, Event) else Event(*ev) for ev in events]
    n = len(x)
    if n < 1 or not events:
        raise ValueError("reference: at least one year and one event")
    x0 = np.asarray(x[0])
    nm, (ny, nx) = x0.shape[0], x0.shape[3:]
    shape = (nm, len(events), ny, nx)
    first, last, miss = (np.full(shape, -1, np.int32) for _ in range(3))
    count, peak_year = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    peak = np.zeros(shape, np.float32)
    fraction = None
    if group is not None:
        grp = np.asarray(group, np.int64)
        ng = int(n_groups) if n_groups is not None else int(grp.max()) + 1
        lists = [np.flatnonzero(grp == g) for g in range(ng)]  # ascending member index
        if any(len(l) == 0 for l in lists):
            raise ValueError("reference: an empty group")
        fraction = np.zeros((n, ng, len(events), ny, nx), np.float32)
    for k in range(n):  # ascending years; year 0 stores
        xk = np.asarray(x[k])
        for e, ev in enumerate(events):
            q = quantity(xk, ev, control)
            thr = np.float32(ev.thr)
            with np.errstate(invalid="ignore"):
                hit = (q >= thr) if ev.dir > 0 else (q <= thr)  # a NaN never hits
                if k == 0:
                    peak[:, e], peak_year[:, e] = q, 0
                else:
                    p = peak[:, e]
                    take = ((q > p) if ev.dir > 0 else (q < p)) | (np.isnan(p) & ~np.isnan(q))  # strict: a tie keeps the earlier year
                    peak[:, e] = np.where(take, q, p)
                    peak_year[:, e] = np.where(take, np.int32(k), peak_year[:, e])
            first[:, e] = np.where((first[:, e] < 0) & hit, np.int32(k), first[:, e])
            last[:, e] = np.where(hit, np.int32(k), last[:, e])
            miss[:, e] = np.where(hit, miss[:, e], np.int32(k))
            count[:, e] += hit.astype(np.int32)
            if fraction is not None:
                for g, l in enumerate(lists):
                    c = hit[l].sum(axis=0, dtype=np.int64)  # (an integer count: its order does not matter)
                    fraction[k, g, e] = (c.astype(np.float64) / np.float64(len(l))).astype(np.float32)
    stay = np.where(miss + 1 <= n - 1, miss + 1, -1).astype(np.int32)
    return Result(first, last, stay, count, peak, peak_year, fraction)


def as_year(a, year0: int = 0, never=np.nan) -> np.ndarray:
    """A map of 0-based years (first, last, stay, peak_year; -1: never) as calendar years, float32: year0 + a where a >= 0,
    `never` elsewhere.  With never = the number of years of the run (and year0 = 0) it is a censored map that
    ens.reduce_dev can take: a member that never crosses counts as crossing right after the run."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError("as_year: an integer map expected")
    return np.where(a >= 0, (a.astype(np.int64) + int(year0)).astype(np.float32), np.float32(never)).astype(np.float32)
