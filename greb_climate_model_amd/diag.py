"""Reduced output: regional means, zonal means and annual-mean maps of an ensemble, made on the device.

The reference leaves diagnostics to R scripts over the output file (R/analyse_output_fields.R computes a global-mean
series from the full records).  An ensemble of hundreds of members cannot hand back every monthly field; what its
analysis wants per member is small and comes from one pass over each model year while it is still in HBM
(csrc/greb_diag.hip; include/greb_engine.h: greb_diag_*, greb_engine_run_diag):

    plan = diag.Plan(inp.nx, inp.ny, diag.standard_regions(inp))
    res = engine.Engine(inp, p, n_members=512).run_diag(100, co2, plan)      # res.regions [512][100][12][5][9], ...
    warming = diag.annual_from_monthly(res.regions)[:, -1, 0] - diag.annual_from_monthly(res.regions)[:, 0, 0]

reduce_reference() is the numpy fp64 statement of the three products, written from their definition and not from the
kernel: it is what the tests hold the device against.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _plan, abi

ALL = abi.D_REGIONS | abi.D_ZONAL | abi.D_ANNUAL
GLOBE = "globe"  # region 0 of every plan


def latitudes(ny: int) -> np.ndarray:
    """Cell-centre latitudes in degrees, row 0 = south (src/greb.f90:580 without the model's pi)."""
    return (np.arange(ny, dtype=np.float64) + 0.5) * 180.0 / ny - 90.0


@dataclass
class Result:
    """What run_diag / reduce_dev hand back; a product that was not asked for is None.
    regions [..][12][5][1 + n_regions], zonal [..][12][5][ny], annual [..][5][ny][nx]; `..` = [n_members][years] from
    Engine.run_diag and [n_members] from reduce_dev.  names[r] is the name of region r (names[0] the globe).  Where the
    plan has another n_vars than 5 (budget records: Engine.run_diag(records=...)), that count stands in place of [5]."""
    regions: object
    zonal: object
    annual: object
    yearly: object
    names: tuple
    vars: tuple = None  # the names of the variables (the axis the shapes call [5]) where the run knows them

    def region(self, name: str):
        return self.regions[..., self.names.index(name)]


class Plan(_plan.Handle):
    """greb_diag handle: the grid, the regions (name -> weights [ny][nx] in [0, 1]; the globe is always region 0) and
    n_vars, the variables per month of the records it reduces (5: a year of state records; 1 ... abi.MAX_RECORD_VARS).
    Host data only; creating one needs no GPU, and every argument error is a GrebError(-1) naming the offender."""
    _destroy = "greb_diag_destroy"

    def __init__(self, nx: int, ny: int, regions: dict | None = None, n_vars: int = 5):
        from . import engine
        regions = dict(regions or {})
        self.nx, self.ny, self.nv = int(nx), int(ny), int(n_vars)
        self.names = (GLOBE,) + tuple(regions)
        self.nr = len(self.names)
        for k, v in regions.items():
            if np.shape(v) != (self.ny, self.nx):
                raise engine.GrebError(-1, f"diag.Plan: region {k!r} has shape {np.shape(v)}, the grid is {(self.ny, self.nx)}")
        self.weights = (np.ascontiguousarray(np.stack([np.asarray(v, np.float32) for v in regions.values()]))
                        if regions else np.zeros((0, self.ny, self.nx), np.float32))
        self._create("greb_diag_create_vars", self.nx, self.ny, abi.fptr(self.weights) if regions else None, len(regions), self.nv)

    def _reword(self, msg: str) -> str:
        for i, k in enumerate(self.names[1:]):  # the library counts regions, the caller named them
            msg = msg.replace(f"region {i + 1}:", f"region {i + 1} ({k!r}):").replace(f"region {i + 1} has", f"region {i + 1} ({k!r}) has")
        return msg


def reduce_dev(plan: Plan, monthly_year, what: int = ALL) -> Result:
    """One model year on the GPU, a contiguous float32 torch tensor [n_members][12][plan.nv][ny][nx], reduced where it is
    (greb_diag_reduce_dev) on torch's current stream, without synchronising.  Returns torch tensors on the same device."""
    import torch
    from . import engine
    x = monthly_year
    dev = _plan.gpu_tensor_check(x, tuple(x.shape[1:]) == (12, plan.nv, plan.ny, plan.nx), "diag.reduce_dev",
                                f"[n][12][{plan.nv}][{plan.ny}][{plan.nx}]")
    n = x.shape[0]
    mk = lambda *s: torch.empty((n,) + s, dtype=torch.float32, device=x.device)
    regions = mk(12, plan.nv, plan.nr) if what & abi.D_REGIONS else None
    zonal = mk(12, plan.nv, plan.ny) if what & abi.D_ZONAL else None
    annual = mk(plan.nv, plan.ny, plan.nx) if what & abi.D_ANNUAL else None
    _plan.call_on_current_stream(dev, engine.lib().greb_diag_reduce_dev, plan.h, int(dev), _plan.ptr(x), int(n), _plan.ptr(regions),
                                 _plan.ptr(zonal), _plan.ptr(annual))
    return Result(regions, zonal, annual, None, plan.names)


def standard_regions(inp) -> dict:
    """The usual cuts of a workload.Inputs as 0/1 masks [ny][nx]: land / ocean as the model's albedo and sea-ice
    routines split them (z_topo >= 0 / < 0, src/greb.f90:384-391), glacier (mask > 0.5, :393), the hemispheres, the
    tropics (|lat| < 30), Arctic (lat > 66) and Antarctic (lat < -66)."""
    lat = np.broadcast_to(latitudes(inp.ny)[:, None], (inp.ny, inp.nx))
    z = np.asarray(inp.z_topo)
    m = {"land": z >= 0, "ocean": z < 0, "glacier": np.asarray(inp.glacier) > 0.5, "NH": lat > 0, "SH": lat < 0,
         "tropics": np.abs(lat) < 30, "Arctic": lat > 66, "Antarctic": lat < -66}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in m.items()}


def reduce_reference(monthly_year, weights=None):
    """The three products in numpy fp64, from their definitions: monthly_year [..][12][V][ny][nx] (V = 5 for state
    records, any other count for budget records), weights [n_regions][ny][nx] (the globe is added in front).  Returns
    (regions [..][12][V][1 + n_regions], zonal [..][12][V][ny], annual [..][V][ny][nx]) as float64."""
    x = np.asarray(monthly_year, np.float64)
    ny, nx = x.shape[-2:]
    if x.ndim < 4 or x.shape[-4] != 12:
        raise ValueError("reduce_reference: [..][12][V][ny][nx] expected")
    area = np.cos(np.deg2rad(latitudes(ny)))[:, None] * np.ones((ny, nx))
    w = [area] if weights is None else [area] + [np.asarray(wr, np.float64) * area for wr in weights]
    w = np.stack(w).reshape(len(w), ny * nx)
    regions = x.reshape(x.shape[:-2] + (ny * nx,)) @ w.T / w.sum(axis=1)
    zonal = x.mean(axis=-1)
    days = np.asarray(abi.JDAY_MON, np.float64)
    annual = (x * days[:, None, None, None]).sum(axis=-4) / days.sum()
    return regions, zonal, annual


def annual_from_monthly(series, axis: int = -3):
    """Day-weighted annual mean of a monthly series, e.g. Result.regions or Result.zonal (month axis -3), in fp64:
    sum jday_mon[m] x_m / 365 (src/greb.f90:42)."""
    x = np.moveaxis(np.asarray(series, np.float64), axis, -1)
    if x.shape[-1] != 12:
        raise ValueError("annual_from_monthly: the month axis must have 12 entries")
    return x @ np.asarray(abi.JDAY_MON, np.float64) / 365.0
