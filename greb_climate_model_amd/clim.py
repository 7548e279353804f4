"""Climatology output: multi-year monthly means, seasonal means, trends and responses to a control member, made on the
device along the time axis.

What an ensemble with a control member beside its other members is run for is answered the same way every time: average
each calendar month over a window of years, then subtract the control.  The reference leaves that to R scripts over the
files of separate processes.  Here each model year is added to fp64 sums in the device staging slot it was integrated
into (csrc/greb_clim.hip; include/greb_engine.h: greb_clim_*, greb_engine_run_clim), and what comes back per averaging
period is a handful of maps per member, whatever the length of the run:

    plan = clim.Plan(inp.nx, inp.ny, 512, control=[-1] + [0] * 511)           # member 0 is everyone's control
    res = engine.Engine(inp, p, n_members=512).run_clim(100, co2, plan, [(0, 30), (70, 30)])
    res.seasons_resp[:, 1, clim.SEASONS.index("ANN"), 0]                       # [512][ny][nx]: annual Tsurf response, years 70-99

reference() is the numpy fp64 statement of the products: the same IEEE operations in the same order as the kernels, so
the tests hold the device to it bit for bit.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _plan, abi

SEASONS = ("DJF", "MAM", "JJA", "SON", "ANN")
# the months of each season in the order they are added (DJF: Dec, Jan, Feb of the same calendar years)
SEASON_MONTHS = ((11, 0, 1), (2, 3, 4), (5, 6, 7), (8, 9, 10), tuple(range(12)))
ALL = abi.C_MEAN | abi.C_SEASONS | abi.C_TREND | abi.C_RESPONSE
PRODUCTS = ("mean", "seasons", "trend", "mean_resp", "seasons_resp")


def selected(what: int) -> tuple:
    """Which of PRODUCTS the flags `what` (abi.C_*) deliver, as five booleans."""
    resp = bool(what & abi.C_RESPONSE)
    return (bool(what & abi.C_MEAN), bool(what & abi.C_SEASONS), bool(what & abi.C_TREND),
            resp and bool(what & abi.C_MEAN), resp and bool(what & abi.C_SEASONS))


def empty_products(what: int, lead: tuple, ny: int, nx: int, n_vars: int = 5) -> list:
    """Host arrays for the selected products, lead + [12 or 5][n_vars][ny][nx] (None where not selected)."""
    n = (12, 5, 12, 12, 5)
    return [np.empty(tuple(lead) + (k, n_vars, ny, nx), np.float32) if on else None for k, on in zip(n, selected(what))]


@dataclass
class Result:
    """What run_clim / finish_dev / reference hand back; a product that was not selected is None.
    mean, trend, mean_resp [..][12][5][ny][nx]; seasons, seasons_resp [..][5: SEASONS][5][ny][nx]; `..` =
    [n_members][n_periods] from Engine.run_clim and [n_members] from finish_dev and reference.  The responses are member
    minus its control; a member without one (control -1) holds NaN there.  Where the plan has another n_vars than 5
    (budget records: Engine.run_clim(records=...)), that count stands in place of the variables' [5]."""
    mean: object
    seasons: object
    trend: object
    mean_resp: object
    seasons_resp: object
    yearly: object = None
    vars: tuple = None  # the names of the variables (the axis the shapes call [5]) where the run knows them

    def season(self, name: str, response: bool = False):
        a = self.seasons_resp if response else self.seasons
        return a[..., SEASONS.index(name), :, :, :]


class Plan(_plan.Handle):
    """greb_clim handle: grid, member count, each member's control member (-1: none; None: no control map) and the
    products (abi.C_* bits; default: MEAN, SEASONS and TREND, and their RESPONSE when there is a control map).  Host data
    only; creating one needs no GPU, and every argument error is a GrebError(-1) naming the offender.  n_vars: the
    variables per month of the records it sums (5: a year of state records; 1 ... abi.MAX_RECORD_VARS)."""
    _destroy = "greb_clim_destroy"

    def __init__(self, nx: int, ny: int, n_members: int, control=None, what: int | None = None, n_vars: int = 5):
        from . import engine
        self.nx, self.ny, self.nm, self.nv = int(nx), int(ny), int(n_members), int(n_vars)
        if what is None:
            what = ALL if control is not None else ALL & ~abi.C_RESPONSE
        self.what = int(what)
        self.control = None
        if control is not None:
            ctl = np.asarray(control)
            if ctl.shape != (self.nm,) or ctl.dtype.kind not in "iu":
                raise engine.GrebError(-1, f"clim.Plan: control must hold {self.nm} integers, one per member")
            self.control = np.ascontiguousarray(ctl, np.int32)
        cp = None if self.control is None else self.control.ctypes.data_as(C.POINTER(C.c_int32))
        self._create("greb_clim_create_vars", self.nx, self.ny, self.nm, cp, C.c_uint(self.what & 0xFFFFFFFF), self.nv)


def add_year_dev(plan: Plan, monthly_year, k: int) -> None:
    """Year k (0-based) of the current period, a contiguous float32 GPU tensor [n_members][12][plan.nv][ny][nx], added to the
    plan's sums where it is (greb_clim_add_year_dev) on torch's current stream, without synchronising."""
    from . import engine
    x = monthly_year
    want = (plan.nm, 12, plan.nv, plan.ny, plan.nx)
    dev = _plan.gpu_tensor_check(x, tuple(x.shape) == want, "clim.add_year_dev", str(list(want)))
    _plan.call_on_current_stream(dev, engine.lib().greb_clim_add_year_dev, plan.h, int(dev), _plan.ptr(x), int(k))
    plan._device = dev


def finish_dev(plan: Plan, n_years: int) -> Result:
    """The products of the n_years years added since the last finish (greb_clim_finish_dev), torch tensors [n_members]...
    on the device of the years, on torch's current stream, without synchronising."""
    import torch
    from . import engine
    dev = getattr(plan, "_device", None)
    if dev is None:
        raise engine.GrebError(-1, "clim.finish_dev: no year was added to this plan")
    n = (12, 5, 12, 12, 5)
    out = [torch.empty((plan.nm, k, plan.nv, plan.ny, plan.nx), dtype=torch.float32, device=f"cuda:{dev}") if on else None
           for k, on in zip(n, selected(plan.what))]
    _plan.call_on_current_stream(dev, engine.lib().greb_clim_finish_dev, plan.h, int(dev), int(n_years), *map(_plan.ptr, out))
    return Result(*out)


def reference(monthly_years, control=None, what: int | None = None) -> Result:
    """The products in numpy fp64, operation by operation as csrc/greb_clim.hip performs them (include/greb_engine.h
    states them): monthly_years [n_years][n_members][12][V][ny][nx] float32 (any sequence of years; V = 5 for state
    records, any other count for budget records), control
    [n_members] or None.  Returns a Result of float32 arrays [n_members]...; products not in `what` are None."""
    if what is None:
        what = ALL if control is not None else ALL & ~abi.C_RESPONSE
    n = len(monthly_years)
    if n < 1:
        raise ValueError("reference: at least one year")
    S = T = None
    for k in range(n):  # ascending years; year 0 stores
        x = np.asarray(monthly_years[k])
        if x.dtype != np.float32 or x.ndim != 5 or x.shape[1] != 12 or (S is not None and x.shape != S.shape):
            raise ValueError("reference: float32 years [n_members][12][V][ny][nx] expected, all of one shape")
        x = x.astype(np.float64)
        if k == 0:
            S, T = x, np.zeros_like(x)
        else:
            S = S + x
            T = T + np.float64(k) * x
    nn = np.float64(n)
    mean64 = S / nn
    days = np.asarray(abi.JDAY_MON, np.float64)

    def seasons_of(m64):
        out = []
        for months in SEASON_MONTHS:
            acc = np.zeros_like(m64[:, 0])
            for mo in months:
                acc = acc + days[mo] * m64[:, mo]
            out.append(acc / np.float64(sum(abi.JDAY_MON[mo] for mo in months)))
        return np.stack(out, axis=1)

    season64 = seasons_of(mean64)
    if n == 1:
        trend64 = np.zeros_like(S)
    else:
        kbar, sxx = (nn - 1.0) / 2.0, nn * (nn * nn - 1.0) / 12.0
        trend64 = (T - kbar * S) / sxx
    sel = selected(what)
    mean_resp = seasons_resp = None
    if sel[3] or sel[4]:
        ctl = np.asarray(control, np.int64)
        if ctl.shape != (S.shape[0],):
            raise ValueError("reference: one control index per member")
        has = ctl >= 0
        pick = np.where(has, ctl, 0)
        blank = lambda d: np.where(has.reshape((-1,) + (1,) * (d.ndim - 1)), d, np.nan).astype(np.float32)
        with np.errstate(invalid="ignore"):
            mean_resp = blank(mean64 - mean64[pick]) if sel[3] else None
            seasons_resp = blank(season64 - season64[pick]) if sel[4] else None
    f32 = lambda a, on: a.astype(np.float32) if on else None
    return Result(f32(mean64, sel[0]), f32(season64, sel[1]), f32(trend64, sel[2]), mean_resp, seasons_resp)
