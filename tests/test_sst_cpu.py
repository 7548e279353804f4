"""CPU: prescribed SST per member (include/greb_engine.h: greb_engine_set_sst_tables, greb_engine_set_member_sst).

The yardstick of the GPU tests -- tests/sst_mirror.py, forcing_mirror's year with the SST blend before every step -- is held
to the oracle before anything is measured against it: with an all-ones anomaly it is Oracle.run under GREB_X_SST_PLUS1, with
weight 0 it is the unhooked year, both bit for bit.  The pattern helpers of greb_climate_model_amd/forcing.py, the header
and the export list are checked as they stand.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import budget_mirror
import forcing_mirror
import sst_mirror
from greb_climate_model_amd import abi, build, forcing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CO2 = 680.0


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_lib())


@pytest.fixture(scope="module")
def years(oracle_lib, inputs, params):
    """One flux-correction year; from its end: the mirror year under anom = 1 / no weight / no season / amp 1, Oracle.run
    under GREB_X_SST_PLUS1, the mirror year under weight 0 and amp 123, the unhooked forcing_mirror year, and the mirror
    year of a member that has the switch AND a weight-0 pattern."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    ones = np.ones((inputs.ny, inputs.nx), f32)
    args = (inputs.tclim, inputs.z_topo, inputs.sw_solar)
    plus1 = sst_mirror.run_year(o, start, CO2, sst_mirror.Sst(ones), *args)
    off = sst_mirror.run_year(o, start, CO2, sst_mirror.Sst(ones, 0 * ones, None, 123.0), *args)
    both = sst_mirror.run_year(o, start, CO2, sst_mirror.Sst(ones, 0 * ones, None, 123.0, plus1=True), *args)
    plain = forcing_mirror.run_year(o, start, CO2, forcing_mirror.Forcing(), inputs.sw_solar)
    start.restore(o)
    o.set_switches(abi.X_SST_PLUS1)
    ref, ref_yearly = o.run(1, CO2)
    ref_state = o.state5()
    o.close()
    return dict(plus1=plus1, off=off, both=both, plain=(plain[0], plain[1], plain[2], plain[4]), ref=(ref[0], ref_state, ref_yearly[0]))


def test_all_ones_mirror_year_equals_oracle_run_under_sst_plus1(years):
    """The condition that ties the mirror to the reference: monthly records, state and the console values, bit for bit."""
    monthly, _, state, yearly = years["plus1"]
    ref, ref_state, ref_yearly = years["ref"]
    assert np.array_equal(monthly, ref), float(np.abs(monthly.astype(np.float64) - ref).max())
    assert np.array_equal(state, ref_state)
    assert np.array_equal(yearly, ref_yearly), (yearly, ref_yearly)
    # (and the switch did something: the plain year is another run)
    assert not np.array_equal(monthly, years["plain"][0])


def test_weight_zero_mirror_year_equals_the_unhooked_year(years):
    for got, want, name in zip(years["off"], years["plain"], ("monthly", "budget", "state", "yearly")):
        assert np.array_equal(got, want), name


def test_switch_acts_first_and_the_blend_on_its_result(years):
    """Switch and a weight-0 pattern: the blend leaves the switch's result, so the year is the switch's."""
    monthly, _, state, yearly = years["both"]
    ref, ref_state, ref_yearly = years["ref"]
    assert np.array_equal(monthly, ref) and np.array_equal(state, ref_state) and np.array_equal(yearly, ref_yearly)


def test_blend_ends_are_exact_and_land_is_never_touched(inputs):
    rng = np.random.default_rng(5)
    ny, nx = inputs.ny, inputs.nx
    Ts = (270.0 + 30.0 * rng.random((ny, nx))).astype(f32)
    anom = rng.standard_normal((ny, nx)).astype(f32)
    season = rng.standard_normal(abi.NSTEP_YR).astype(f32)
    ocean = np.asarray(inputs.z_topo) < 0
    assert ocean.any() and (~ocean).any()
    for ityr in (1, 2, 366, 730):
        prev = np.asarray(inputs.tclim[(ityr - 2) % abi.NSTEP_YR], f32)
        target = prev + ((anom * season[ityr - 1]).astype(f32) * f32(2.5)).astype(f32)
        one = sst_mirror.prescribe(sst_mirror.Sst(anom, np.ones((ny, nx), f32), season, 2.5), ityr, Ts, inputs.tclim, inputs.z_topo)
        none = sst_mirror.prescribe(sst_mirror.Sst(anom, None, season, 2.5), ityr, Ts, inputs.tclim, inputs.z_topo)
        zero = sst_mirror.prescribe(sst_mirror.Sst(anom, np.zeros((ny, nx), f32), season, 2.5), ityr, Ts, inputs.tclim, inputs.z_topo)
        assert np.array_equal(one[ocean], target[ocean]) and np.array_equal(none, one)
        assert np.array_equal(zero, Ts)
        assert np.array_equal(one[~ocean], Ts[~ocean])
    # step 1 reads slice 730
    first = sst_mirror.prescribe(sst_mirror.Sst(0 * anom), 1, Ts, inputs.tclim, inputs.z_topo)
    assert np.array_equal(first[ocean], np.asarray(inputs.tclim[abi.NSTEP_YR - 1], f32)[ocean])


def test_sst_patch(inputs):
    lat = (np.arange(inputs.ny) + 0.5) * 180.0 / inputs.ny - 90.0
    lon = forcing.longitudes(inputs.nx)
    j, i = inputs.ny // 2 + 3, 1  # a centre on a cell centre, close to Greenwich: the patch wraps
    p = forcing.sst_patch(inputs, lat[j], lon[i], 15.0, 20.0)
    assert p.dtype == f32 and p.shape == (inputs.ny, inputs.nx)
    assert p.min() >= 0.0 and p.max() <= 1.0 and p[j, i] == 1.0 and (p == 1.0).sum() == 1
    assert (p[j, -4:] > 0).all() and (p[j, :6] > 0).all() and p[j, inputs.nx // 2] == 0  # wraps in longitude
    assert np.array_equal(p[j, i + 1:i + 5], p[j, [i - 1, i - 2, i - 3, i - 4]])          # and is symmetric across it
    assert (p[np.abs(lat - lat[j]) >= 15.0] == 0).all()
    d = np.abs((lon - lon[i] + 180.0) % 360.0 - 180.0)
    assert (p[:, d >= 20.0] == 0).all() and (p[np.abs(lat - lat[j]) < 15.0][:, d < 20.0] > 0).all()
    with pytest.raises(ValueError):
        forcing.sst_patch(inputs, 0.0, 0.0, 0.0, 10.0)


@pytest.mark.parametrize("nlat,nlon", [(2, 3), (5, 8), (8, 16), (1, 1), (3, 2)])
def test_sst_patch_lattice_sums_to_one(inputs, nlat, nlon):
    centres, patches = forcing.sst_patch_lattice(inputs, nlat, nlon)
    assert centres.shape == (nlat * nlon, 2) and patches.shape == (nlat * nlon, inputs.ny, inputs.nx) and patches.dtype == f32
    assert patches.min() >= 0.0 and patches.max() <= 1.0
    lat = (np.arange(inputs.ny) + 0.5) * 180.0 / inputs.ny - 90.0
    inside = (lat >= centres[:, 0].min()) & (lat <= centres[:, 0].max())
    total = patches.astype(np.float64).sum(axis=0)
    if nlat > 1:
        assert inside.sum() > 10
        err = np.abs(total[inside] - 1.0).max() / np.spacing(f32(1))
        assert err <= 2.0, err
    assert (total <= 1.0 + 2 * np.spacing(f32(1))).all()
    assert (total[np.abs(lat) > 60.0 + (120.0 / max(nlat - 1, 2))] == 0).all()


def test_basin_weight(inputs):
    lat = (np.arange(inputs.ny) + 0.5) * 180.0 / inputs.ny - 90.0
    lon = forcing.longitudes(inputs.nx)
    box = (-20.0, 20.0, 150.0, 260.0)
    w = forcing.basin_weight(inputs, box, 15.0)
    assert w.dtype == f32 and w.min() == 0.0 and w.max() == 1.0
    in_lat, in_lon = (lat >= -20) & (lat <= 20), (lon >= 150) & (lon <= 260)
    assert (w[np.ix_(in_lat, in_lon)] == 1).all()
    assert (w[np.abs(lat) >= 35.0] == 0).all() and (w[:, (lon <= 135.0) | (lon >= 275.0)] == 0).all()
    mid = inputs.ny // 2
    east = w[mid, (lon > 260)]           # leaving the box eastwards: never rising, strictly falling inside the buffer
    assert (np.diff(east) <= 0).all() and ((east > 0) & (east < 1)).sum() >= 3
    assert (np.diff(east[(east > 0)]) < 0).all()
    north = w[lat > 20][:, inputs.nx // 2 + 4]
    assert (np.diff(north) <= 0).all() and ((north > 0) & (north < 1)).sum() >= 3
    # a box across Greenwich, and a sharp edge
    g = forcing.basin_weight(inputs, (-10.0, 10.0, 340.0, 20.0), 0.0)
    assert set(np.unique(g)) == {0.0, 1.0} and g[mid, 0] == 1 and g[mid, -1] == 1 and g[mid, inputs.nx // 2] == 0


def test_case3_tables_are_what_the_gpu_case_asks_for(inputs):
    anom, weight, season, s = sst_mirror.case3(inputs)
    assert anom.max() == 1.0 and (anom > 0).sum() > 20 and s.amp == f32(2.0)
    assert ((weight > 0) & (weight < 1)).any() and (weight == 1).any() and (weight == 0).any()
    assert season[0] > 0 > season[abi.NSTEP_YR // 2] and (np.sign(season[:180]) == 1).all() and (np.sign(season[190:540]) == -1).all()
    ocean = np.asarray(inputs.z_topo) < 0
    assert ((anom > 0) & (weight > 0) & ocean).sum() > 20  # the patch lies in the basin, on the ocean


def test_header_and_exports_carry_the_two_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    from greb_climate_model_amd import engine
    for name in ("greb_engine_set_sst_tables", "greb_engine_set_member_sst"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in engine.EXPORTS and hasattr(lib, name), name
    m = re.search(r"typedef struct greb_member_sst \{(.*?)\} greb_member_sst;", hdr, re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", m.group(1))
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(abi.GrebMemberSst._fields_)
    assert C.sizeof(abi.GrebMemberSst) == 8
    assert int(re.search(r"#define\s+GREB_MAX_SST_PATTERNS\s+(\d+)", hdr).group(1)) == abi.MAX_SST_PATTERNS == 1024
    assert hasattr(engine.Engine, "set_sst_tables") and hasattr(engine.Engine, "set_member_sst")


def test_setters_reject_a_null_engine(lib):
    """Argument errors come before anything touches a device."""
    a = np.ones((1, 48, 96), f32)
    s = (abi.GrebMemberSst * 1)()
    for rc in (lib.greb_engine_set_sst_tables(None, 1, abi.fptr(a), None, None), lib.greb_engine_set_sst_tables(None, 0, None, None, None),
               lib.greb_engine_set_member_sst(None, s), lib.greb_engine_set_member_sst(None, None)):
        assert rc in (-1, -3), rc
    lib.greb_engine_last_error.restype = C.c_char_p
    assert b"no engine" in lib.greb_engine_last_error(None)
