"""Forcing tables for Engine.set_forcing_tables / Engine.set_member_forcing (include/greb_engine.h: per-member forcing).

Host-side numpy only.  The engine takes any tables; these are the usual partial-CO2 experiments -- CO2 changed in one
hemisphere, in or outside the tropics, over land or ocean only, in one half of the year -- and a scaled copy of the
workload's own insolation; and, for Engine.set_sst_tables / Engine.set_member_sst (prescribed SST), the cos^2 patches of
a Green's-function experiment and the basin weight of a pacemaker run."""
from __future__ import annotations

import numpy as np

from . import abi, diag

PARTIAL_NAMES = ("NH", "SH", "tropics", "extratropics", "land", "ocean", "Apr-Sep", "Oct-Mar")
# complementary pairs of partial_co2_patterns: space[a] * season[a] + space[b] * season[b] = 1 everywhere, all year
PARTIAL_PAIRS = ((0, 1), (2, 3), (4, 5), (6, 7))


def half_year_steps() -> np.ndarray:
    """[730] bool: the steps (two per day, src/greb.f90:251) of April ... September, month ends from abi.JDAY_MON."""
    end = np.cumsum(abi.JDAY_MON)  # last day of each month, 1-based
    jday = np.arange(abi.NSTEP_YR) // 2 + 1
    return (jday > end[2]) & (jday <= end[8])


def partial_co2_patterns(inp):
    """(names, space [8][ny][nx], season [8][730]) for PARTIAL_NAMES: NH / SH, tropics (|lat| < 30 degrees) / extratropics,
    land (z_topo > 0) / ocean, and the two halves of the year (space all ones, season 0 or 1).  All weights are 0 or 1 and
    each complementary pair (PARTIAL_PAIRS) sums to exactly one at every point and step."""
    ny, nx = inp.ny, inp.nx
    lat = np.broadcast_to(diag.latitudes(ny)[:, None], (ny, nx))
    land = np.asarray(inp.z_topo) > 0
    summer = half_year_steps()
    one = np.ones((ny, nx), bool)
    space = np.stack([lat > 0, lat <= 0, np.abs(lat) < 30, np.abs(lat) >= 30, land, ~land, one, one]).astype(np.float32)
    season = np.ones((8, abi.NSTEP_YR), np.float32)
    season[6] = summer
    season[7] = ~summer
    return PARTIAL_NAMES, np.ascontiguousarray(space), season


def scaled_solar(inp, factor: float) -> np.ndarray:
    """The workload's insolation [730][ny] times `factor`, in fp32 (the same numbers as solar_scale = factor on the
    engine's own table: one rounding per value)."""
    return (np.asarray(inp.sw_solar, np.float32) * np.float32(factor)).astype(np.float32)


# ---- prescribed SST (Engine.set_sst_tables / Engine.set_member_sst; include/greb_engine.h: prescribed SST)
def longitudes(nx: int) -> np.ndarray:
    """Cell-centre longitudes in degrees east, column 0 at half a cell east of Greenwich."""
    return (np.arange(nx, dtype=np.float64) + 0.5) * 360.0 / nx


def _east_of(lon, lon0):
    """Signed longitude difference in [-180, 180)."""
    return (np.asarray(lon, np.float64) - lon0 + 180.0) % 360.0 - 180.0


def _hump(d, half):
    """cos^2 of a distance d over a half-width: 1 at 0, 0 at the half-width and beyond."""
    d = np.abs(np.asarray(d, np.float64))
    return np.where(d < half, np.cos(0.5 * np.pi * np.minimum(d, half) / half) ** 2, 0.0)


def sst_patch(inp, lat0: float, lon0: float, dlat: float, dlon: float) -> np.ndarray:
    """[ny][nx] fp32: the cos^2 x cos^2 hump of the Green's-function experiments, 1 at (lat0, lon0) and 0 at the half-widths
    dlat, dlon (degrees) and beyond; longitude is periodic.  It is an SST anomaly pattern in units of the member's amp."""
    if not (dlat > 0 and dlon > 0):
        raise ValueError("sst_patch: the half-widths must be positive")
    a = _hump(diag.latitudes(inp.ny) - lat0, dlat)[:, None] * _hump(_east_of(longitudes(inp.nx), lon0), dlon)[None, :]
    return np.ascontiguousarray(a, np.float32)


def sst_patch_lattice(inp, nlat: int, nlon: int, lat_range=(-60.0, 60.0)):
    """(centres [nlat * nlon][2] as (lat, lon), patches [nlat * nlon][ny][nx]): sst_patch on a lattice whose centres are one
    half-width apart -- nlat latitudes from lat_range[0] to lat_range[1], nlon longitudes around the globe from 0 -- so
    that cos^2 + sin^2 of neighbours makes the patches sum to 1 between the outermost centre latitudes.  One latitude: the
    centre of the range, half-width half the range; one longitude: no dependence on longitude."""
    if nlat < 1 or nlon < 1:
        raise ValueError("sst_patch_lattice: nlat and nlon must be at least 1")
    lo, hi = float(lat_range[0]), float(lat_range[1])
    if not hi > lo:
        raise ValueError("sst_patch_lattice: lat_range must ascend")
    lats = np.linspace(lo, hi, nlat) if nlat > 1 else np.asarray([0.5 * (lo + hi)])
    hlat = (hi - lo) / (nlat - 1) if nlat > 1 else 0.5 * (hi - lo)
    lons = np.arange(nlon) * 360.0 / nlon
    lat, lon = diag.latitudes(inp.ny), longitudes(inp.nx)
    centres, patches = [], []
    for la in lats:
        for lo_ in lons:
            x = _hump(_east_of(lon, lo_), 360.0 / nlon) if nlon > 1 else np.ones(inp.nx)
            centres.append((la, lo_))
            patches.append(_hump(lat - la, hlat)[:, None] * x[None, :])
    return np.asarray(centres, np.float64), np.ascontiguousarray(np.stack(patches), np.float32)


def basin_weight(inp, box, buffer_deg: float) -> np.ndarray:
    """[ny][nx] fp32 nudging weight of a pacemaker run: 1 inside box = (lat_south, lat_north, lon_west, lon_east) (degrees;
    the box runs eastwards from lon_west to lon_east and may cross Greenwich), falling linearly to 0 over buffer_deg degrees
    outside it (the larger of the latitude and the longitude distance), 0 beyond.  buffer_deg = 0: a sharp edge."""
    south, north, west, east = (float(v) for v in box)
    if north < south or buffer_deg < 0:
        raise ValueError("basin_weight: box is (lat_south, lat_north, lon_west, lon_east), buffer_deg >= 0")
    lat, lon = diag.latitudes(inp.ny), longitudes(inp.nx)
    dlat = np.maximum(np.maximum(south - lat, lat - north), 0.0)
    span = 360.0 if east - west >= 360.0 else (east - west) % 360.0
    x = (lon - west) % 360.0
    dlon = np.where(x <= span, 0.0, np.minimum(x - span, 360.0 - x))
    d = np.maximum(dlat[:, None], dlon[None, :])
    w = (d == 0).astype(np.float64) if buffer_deg == 0 else np.clip(1.0 - d / buffer_deg, 0.0, 1.0)
    return np.ascontiguousarray(w, np.float32)
