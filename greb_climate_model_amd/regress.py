"""Regression output: each member's records per unit of its OWN index, made on the device along the time axis.

clim.Plan's TREND regresses on the year number, which is known before the run.  The local change per degree of the
member's own global-mean warming (pattern scaling), polar amplification as a number per member, Arctic albedo or humidity
per degree: the regressor is a scalar the run itself produces -- a regional mean of the same member's year --, known only
once the year has been reduced in space, so no other plan's sums give the product sum of g * y over the years.  Members of
a perturbed-physics ensemble differ in climate sensitivity; their patterns become comparable only after normalising by
the member's own index.  Here each model year is reduced to its regional means where it was integrated (the device code
of diag.reduce_dev), the indices are formed from them, and a few fp64 sums per (member, term, point) follow the years
(csrc/greb_reg.hip; include/greb_engine.h: greb_reg_*, greb_engine_run_reg).  What comes back is up to three maps per member
and term, whatever the length of the run:

    M = 256                                                            # member m rises 1 %/yr, member M + m is its control
    indices = [regress.Index(0, cross.ANN, rel=True)]                  # the annual global-mean Tsurf response
    terms = [regress.Term(0, cross.ANN, rel=True), regress.Term(4, cross.SEP, rel=True)]
    plan = regress.Plan(nx, ny, 2 * M, indices, terms, control=list(range(M, 2 * M)) * 2)
    res = eng.run_reg(100, co2, plan)
    res.slope[:M, 0]                                                   # [M][ny][nx]: K of local warming per K of global warming
    res.index[:M, :, 0]                                                # [M][100]: each member's global-mean warming

reference() is the numpy statement of the products: the same IEEE operations in the same order as the kernels, so the
tests hold the device to it for equal float bits.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace

import numpy as np

from . import _plan, abi, cross, diag

MAPS = abi.R_SLOPE | abi.R_INTERCEPT | abi.R_R2
ALL = MAPS | abi.R_INDEX
PRODUCTS = ("slope", "intercept", "r2", "index")
_FLAGS = (abi.R_SLOPE, abi.R_INTERCEPT, abi.R_R2, abi.R_INDEX)


@dataclass
class Index:
    """One index: the mean over `region` (0: the globe; 1 ...: the plan's regions in their order) of variable `var`, selector
    `sel` (cross.JAN ... cross.DEC, cross.DJF ... cross.ANN), and `rel` (the member's value minus its control's)."""
    var: int
    sel: int
    region: int = 0
    rel: bool = False


@dataclass
class Term:
    """One term: variable `var` of the records, selector `sel`, the index it is regressed on and `rel` (the quantity is the
    member minus its control), as cross.Event has them."""
    var: int
    sel: int
    index: int = 0
    rel: bool = False


@dataclass
class Result:
    """What run_reg / finish_dev / reference hand back; a product that was not selected is None.  slope, intercept, r2
    float32 [n_members][n_terms][ny][nx] (NaN where fewer than two years were added or the index did not vary; r2 also where
    the term did not vary); index float32 [n_members][years][n_indices] (from add_year_dev: one year's
    [n_members][n_indices])."""
    slope: object
    intercept: object
    r2: object
    index: object = None
    yearly: object = None
    vars: tuple = None  # the names of the variables of the records where the run knows them


def selected(what: int) -> tuple:
    """Which of PRODUCTS the flags `what` (abi.R_*) deliver, as four booleans."""
    return tuple(bool(what & f) for f in _FLAGS)


def memory_bytes(what: int, n_members: int, n_terms: int, n_indices: int, ny: int, nx: int, n_vars: int = 5, n_regions: int = 0,
                 run_years: int = 0) -> int:
    """Device memory of a plan: y0, Sy and Sgy -- 20 bytes per (member, term, point) --, 8 more for Syy with R2; 28 bytes per
    (member, index); one year's regional means with diag's tables and scratch.  run_years > 0: what Engine.run_reg adds, one
    float map per (member, term, point) where a map is selected and the INDEX series.  Nothing else grows with the years."""
    el, nr = n_members * n_terms * ny * nx, 1 + n_regions
    rows = max(1, 256 // (nx // 4))
    bands = (ny + rows - 1) // rows
    total = (28 if what & abi.R_R2 else 20) * el + 28 * n_members * n_indices
    total += 4 * n_members * 12 * n_vars * nr + 8 * n_members * n_vars * bands * 12 * nr + 8 * nr * (ny * nx + 1)
    if run_years > 0:
        total += (4 * el if what & MAPS else 0) + (4 * n_members * run_years * n_indices if what & abi.R_INDEX else 0)
    return total


class Plan(_plan.Handle):
    """greb_reg handle: grid, member count, 1 ... 8 indices, 1 ... 16 terms, the regions (name -> weights [ny][nx] in [0, 1],
    as diag.Plan takes them; the globe is always region 0), the variables per month of the records (5: a year of state
    records), each member's control member (-1: none; None: no control map) and the products (abi.R_* bits; default all
    four).  An Index may name its region.  Host data only; creating one needs no GPU, and every argument error is a
    GrebError(-1) naming the offender.  Device memory: memory_bytes()."""
    _destroy = "greb_reg_destroy"

    def __init__(self, nx: int, ny: int, n_members: int, indices, terms, regions: dict | None = None, n_vars: int = 5, control=None,
                 what: int | None = None):
        from . import engine
        regions = dict(regions or {})
        self.nx, self.ny, self.nm, self.nv = int(nx), int(ny), int(n_members), int(n_vars)
        self.names = (diag.GLOBE,) + tuple(regions)
        self.nr = len(self.names)
        self.indices = [replace(ix) if isinstance(ix, Index) else Index(*ix) for ix in indices]  # copies: a name is resolved below
        for ix in self.indices:
            if isinstance(ix.region, str):
                if ix.region not in self.names:
                    raise engine.GrebError(-1, f"regress.Plan: an index names region {ix.region!r}, the plan has {self.names}")
                ix.region = self.names.index(ix.region)
        self.terms = [replace(t) if isinstance(t, Term) else Term(*t) for t in terms]
        self.ni, self.nt = len(self.indices), len(self.terms)
        for k, v in regions.items():
            if np.shape(v) != (self.ny, self.nx):
                raise engine.GrebError(-1, f"regress.Plan: region {k!r} has shape {np.shape(v)}, the grid is {(self.ny, self.nx)}")
        self.weights = (np.ascontiguousarray(np.stack([np.asarray(v, np.float32) for v in regions.values()]))
                        if regions else np.zeros((0, self.ny, self.nx), np.float32))
        if control is not None:
            control = np.asarray(control)
            if control.shape != (max(self.nm, 0),) or (control.size and control.dtype.kind not in "iu"):
                raise engine.GrebError(-1, f"regress.Plan: control must hold {self.nm} integers, one per member")
            control = np.ascontiguousarray(control, np.int32)
        self.control = control
        self.what = ALL if what is None else int(what)
        ixs = (abi.GrebRegIndex * max(self.ni, 1))()
        for c, ix in zip(ixs, self.indices):
            c.var, c.sel, c.rel, c.region = int(ix.var), int(ix.sel), int(ix.rel), int(ix.region)
        tms = (abi.GrebRegTerm * max(self.nt, 1))()
        for c, t in zip(tms, self.terms):
            c.var, c.sel, c.rel, c.index = int(t.var), int(t.sel), int(t.rel), int(t.index)
        self._create("greb_reg_create", self.nx, self.ny, self.nm, self.nv, abi.fptr(self.weights) if regions else None, len(regions),
                     None if control is None else control.ctypes.data_as(C.POINTER(C.c_int32)), ixs, self.ni, tms, self.nt,
                     C.c_uint(self.what & 0xFFFFFFFF))

    def _reword(self, msg: str) -> str:
        for i, k in enumerate(self.names[1:]):  # the library counts regions, the caller named them
            msg = msg.replace(f"region {i + 1}:", f"region {i + 1} ({k!r}):").replace(f"region {i + 1} has", f"region {i + 1} ({k!r}) has")
        return msg

    def memory_bytes(self, run_years: int = 0) -> int:
        return memory_bytes(self.what, self.nm, self.nt, self.ni, self.ny, self.nx, self.nv, self.nr - 1, run_years)

    def describe(self) -> str:
        names = [n for n, on in zip(PRODUCTS, selected(self.what)) if on]
        return (f"regress.Plan: {self.nm} members x {self.nt} terms on {self.ni} indices over {self.nr} regions at {self.nx} x {self.ny}, "
                f"products {', '.join(names)}: {self.memory_bytes() / 1e6:.1f} MB of device memory, whatever the number of years")


def empty_products(plan: Plan, years: int) -> list:
    """Host arrays for the selected products of a run of `years` years (None where not selected), in PRODUCTS' order."""
    on = selected(plan.what)
    out = [np.empty((plan.nm, plan.nt, plan.ny, plan.nx), np.float32) if o else None for o in on[:3]]
    out.append(np.empty((plan.nm, years, plan.ni), np.float32) if on[3] else None)
    return out


def add_year_dev(plan: Plan, x, k: int):
    """Year k (0-based) of the current period, a contiguous float32 GPU tensor [n_members][12][plan.nv][ny][nx], into the
    plan's state where it is (greb_reg_add_year_dev) on torch's current stream, without synchronising.  Returns that
    year's index values [n_members][n_indices] as a torch tensor where the plan selects INDEX, else None."""
    import torch
    from . import engine
    want = (plan.nm, 12, plan.nv, plan.ny, plan.nx)
    dev = _plan.gpu_tensor_check(x, tuple(x.shape) == want, "regress.add_year_dev", str(list(want)))
    index = None
    if plan.what & abi.R_INDEX:
        index = torch.empty((plan.nm, plan.ni), dtype=torch.float32, device=f"cuda:{dev}")
    _plan.call_on_current_stream(dev, engine.lib().greb_reg_add_year_dev, plan.h, int(dev), _plan.ptr(x), int(k), _plan.ptr(index))
    plan._device = dev
    return index


def finish_dev(plan: Plan, n_years: int) -> Result:
    """The maps of the n_years years added since the last finish (greb_reg_finish_dev), torch tensors
    [n_members][n_terms][ny][nx] on the device of the years, on torch's current stream, without synchronising."""
    import torch
    from . import engine
    dev = getattr(plan, "_device", None)
    if dev is None:
        raise engine.GrebError(-1, "regress.finish_dev: no year was added to this plan")
    shape = (plan.nm, plan.nt, plan.ny, plan.nx)
    out = [torch.empty(shape, dtype=torch.float32, device=f"cuda:{dev}") if on else None for on in selected(plan.what)[:3]]
    _plan.call_on_current_stream(dev, engine.lib().greb_reg_finish_dev, plan.h, int(dev), int(n_years), *map(_plan.ptr, out))
    return Result(*out)


def index_values(regions_year, indices, control=None) -> np.ndarray:
    """The year's index values g, [n_members][n_indices] float32, from the year's fp32 regional means
    [n_members][12][V][n_regions + 1], operation by operation as include/greb_engine.h states it: cross.quantity over the
    regional means in place of the points."""
    r = np.asarray(regions_year)
    if r.dtype != np.float32 or r.ndim != 4 or r.shape[1] != 12:
        raise ValueError("index_values: float32 regional means [n_members][12][V][regions] expected")
    year = r[:, :, :, None, :]  # the regions where a year has its longitudes
    g = np.empty((r.shape[0], len(indices)), np.float32)
    for j, ix in enumerate(indices):
        g[:, j] = cross.quantity(year, cross.Event(ix.var, ix.sel, 0.0, +1, ix.rel), control)[:, 0, ix.region]
    return g


def reference(x, indices, terms, control=None, region_w=None, regions=None) -> Result:
    """The products in numpy, operation by operation as include/greb_engine.h states them: x [years][n_members][12][V][ny][nx]
    float32 (any sequence of years), indices a list of Index, terms a list of Term, control [n_members] or None.  The
    regional means the indices are taken from: `regions` [years][n_members][12][V][1 + n_regions] float32 -- those made on the
    device (diag.reduce_dev) -- are used as given; without it, diag.reduce_reference over region_w [n_regions][ny][nx] rounded
    to float32.  Returns a Result of the three maps and index [n_members][years][n_indices]."""
    indices = [ix if isinstance(ix, Index) else Index(*ix) for ix in indices]
    terms = [t if isinstance(t, Term) else Term(*t) for t in terms]
    n = len(x)
    if n < 1 or not indices or not terms:
        raise ValueError("reference: at least one year, one index and one term")
    x0 = np.asarray(x[0])
    nm, (ny, nx) = x0.shape[0], x0.shape[3:]
    shape = (nm, len(terms), ny, nx)
    y0 = np.zeros(shape, np.float32)
    Sy, Sgy, Syy = (np.zeros(shape, np.float64) for _ in range(3))
    g0 = np.zeros((nm, len(indices)), np.float32)
    Sg, Sgg = (np.zeros((nm, len(indices)), np.float64) for _ in range(2))
    series = np.zeros((nm, n, len(indices)), np.float32)
    with np.errstate(all="ignore"):
        for k in range(n):  # ascending years; year 0 stores
            xk = np.asarray(x[k])
            rk = np.asarray(regions[k], np.float32) if regions is not None else diag.reduce_reference(xk, region_w)[0].astype(np.float32)
            g = index_values(rk, indices, control)
            series[:, k] = g
            if k == 0:
                g0[:] = g
                G = np.zeros(g.shape, np.float64)
            else:
                G = g.astype(np.float64) - g0.astype(np.float64)
                Sg = Sg + G
                Sgg = Sgg + G * G  # multiply, then add: never fused
            for t, tm in enumerate(terms):
                y = cross.quantity(xk, cross.Event(tm.var, tm.sel, 0.0, +1, tm.rel), control)
                if k == 0:
                    y0[:, t] = y
                    continue
                Y = y.astype(np.float64) - y0[:, t].astype(np.float64)
                Gt = G[:, tm.index][:, None, None]
                Sy[:, t] = Sy[:, t] + Y
                Sgy[:, t] = Sgy[:, t] + Gt * Y
                Syy[:, t] = Syy[:, t] + Y * Y
        nd = np.float64(n)
        of = [tm.index for tm in terms]
        sg, sgg, gz = (a[:, of][:, :, None, None] for a in (Sg, Sgg, g0.astype(np.float64)))  # each term's index
        Sxx = sgg - sg * sg / nd  # every step a separate fp64 operation
        Sxy = Sgy - sg * Sy / nd
        Syc = Syy - Sy * Sy / nd
        b = Sxy / Sxx
        ok = np.broadcast_to((n >= 2) & (Sxx > 0), shape)
        nan = np.float32(np.nan)
        slope = np.where(ok, b.astype(np.float32), nan)
        intercept = np.where(ok, ((y0.astype(np.float64) + Sy / nd) - b * (gz + sg / nd)).astype(np.float32), nan)
        r2 = np.where(ok & (Syc > 0), ((Sxy * Sxy) / (Sxx * Syc)).astype(np.float32), nan)
    return Result(slope.astype(np.float32), intercept.astype(np.float32), r2.astype(np.float32), series)
