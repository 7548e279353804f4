"""Forcing tables for Engine.set_forcing_tables / Engine.set_member_forcing (include/greb_engine.h: per-member forcing).

Host-side numpy only.  The engine takes any tables; these are the usual partial-CO2 experiments -- CO2 changed in one
hemisphere, in or outside the tropics, over land or ocean only, in one half of the year -- and a scaled copy of the
workload's own insolation."""
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
