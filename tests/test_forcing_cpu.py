"""CPU: per-member forcing (include/greb_engine.h: greb_engine_set_forcing_tables, greb_engine_set_member_forcing).

The yardstick of the GPU tests -- tests/forcing_mirror.py, budget_mirror's year with a CO2 field and an insolation row
vector per step -- is held to the oracle before anything is measured against it; the identities the lerp form of the
forcing rests on are checked in numpy fp32; the tables of greb_climate_model_amd/forcing.py, the header and the export list
are checked as they stand.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import budget_mirror
import forcing_mirror
from greb_climate_model_amd import abi, build, forcing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LEVELS = (680.0, 340.0, 298.0)


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_lib())


@pytest.fixture(scope="module")
def neutral_year(oracle_lib, inputs, params):
    """One flux-correction year, then one mirror year under neutral forcing and one year of Oracle.run from the same state."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    monthly, budget, state, kept, yearly = forcing_mirror.run_year(o, start, 680.0, forcing_mirror.Forcing(), inputs.sw_solar,
                                                           keep_sw_steps=(1, 365, 730))
    start.restore(o)
    ref, ref_yearly = o.run(1, 680.0)
    ref_state = o.state5()
    o.close()
    return monthly, state, kept, ref[0], ref_state, yearly, ref_yearly[0]


def test_recomputed_sw_equals_the_oracles(neutral_year):
    """Base table, scale 1: solar[:, None] * (1 - albedo) from the oracle's albedo IS the oracle's sw, at steps 1, 365, 730."""
    kept = neutral_year[2]
    assert sorted(kept) == [1, 365, 730]
    for ityr, (mine, oracles) in kept.items():
        assert np.array_equal(mine, oracles), (ityr, float(np.abs(mine.astype(np.float64) - oracles).max()))
        assert mine.max() > 0


def test_neutral_mirror_year_equals_oracle_run(neutral_year):
    monthly, state, _, ref, ref_state, yearly, ref_yearly = neutral_year
    assert np.array_equal(monthly, ref), float(np.abs(monthly.astype(np.float64) - ref).max())
    assert np.array_equal(state, ref_state)
    assert np.array_equal(yearly, ref_yearly), (yearly, ref_yearly)  # the console values, summed in the reference's order


@pytest.mark.parametrize("co2", LEVELS)
@pytest.mark.parametrize("ref", LEVELS)
def test_lerp_identities_in_fp32(co2, ref):
    """w = 1 gives co2_ppm bit for bit, w = 0 gives co2_ref, scale = 1 gives S: what the neutral and the complementary
    GPU cases rest on.  (The affine form ref + w (co2 - ref) has neither end exact in general.)"""
    shape = (3, 4)
    for season in (None, np.ones(abi.NSTEP_YR, f32)):
        one = forcing_mirror.Forcing(np.ones(shape, f32), season, ref)
        zero = forcing_mirror.Forcing(np.zeros(shape, f32), season, ref)
        assert np.array_equal(forcing_mirror.co2_field(one, 17, co2, shape), np.full(shape, f32(co2)))
        assert np.array_equal(forcing_mirror.co2_field(zero, 17, co2, shape), np.full(shape, f32(ref)))
    off = forcing_mirror.Forcing(np.ones(shape, f32), np.zeros(abi.NSTEP_YR, f32), ref)  # a season weight of 0 switches it off
    assert np.array_equal(forcing_mirror.co2_field(off, 730, co2, shape), np.full(shape, f32(ref)))
    none = forcing_mirror.Forcing(co2_ref=ref)
    assert np.array_equal(forcing_mirror.co2_field(none, 1, co2, shape), np.full(shape, f32(co2)))
    S = np.linspace(0.0, 551.3, 2 * 48, dtype=f32).reshape(2, 48)
    assert np.array_equal(forcing_mirror.solar_rows(forcing_mirror.Forcing(scale=1.0), 2, S), S[1])
    assert np.array_equal(forcing_mirror.solar_rows(forcing_mirror.Forcing(solar=S[::-1], scale=1.0), 1, S), S[1])


def test_complementary_weights_give_the_same_field():
    """(pattern w, 680, ref 340) and (pattern 1 - w, 340, ref 680) are the same sum with its operands swapped, for 0/1
    weights bit for bit: the GPU's complementary-pattern case."""
    w = (np.arange(12).reshape(3, 4) % 2).astype(f32)
    a = forcing_mirror.co2_field(forcing_mirror.Forcing(w, None, 340.0), 5, 680.0, w.shape)
    b = forcing_mirror.co2_field(forcing_mirror.Forcing(f32(1) - w, None, 680.0), 5, 340.0, w.shape)
    assert np.array_equal(a, b) and set(np.unique(a)) == {f32(340.0), f32(680.0)}


def test_partial_patterns_pair_up_to_one(inputs):
    names, space, season = forcing.partial_co2_patterns(inputs)
    assert names == forcing.PARTIAL_NAMES and len(names) == 8
    assert space.shape == (8, inputs.ny, inputs.nx) and season.shape == (8, abi.NSTEP_YR)
    assert space.dtype == f32 and season.dtype == f32
    assert set(np.unique(space)) <= {0.0, 1.0} and set(np.unique(season)) <= {0.0, 1.0}
    for a, b in forcing.PARTIAL_PAIRS:
        w = space[a][None] * season[a][:, None, None] + space[b][None] * season[b][:, None, None]
        assert np.array_equal(w, np.ones_like(w)), (names[a], names[b])
        assert space[a].any() and space[b].any() and season[a].any() and season[b].any()
    # the halves of the year: April 1 is day 91 (steps 181 and 182, 1-based), September 30 day 273 (steps 545, 546)
    summer = season[6].astype(bool)
    assert summer.sum() == 2 * sum(abi.JDAY_MON[3:9]) == 366
    assert not summer[179] and summer[180] and summer[545] and not summer[546]
    lat = (np.arange(inputs.ny) + 0.5) * 180.0 / inputs.ny - 90.0
    assert np.array_equal(space[0][:, 0] > 0, lat > 0) and np.array_equal(space[2][:, 0] > 0, np.abs(lat) < 30)
    assert np.array_equal(space[4] > 0, np.asarray(inputs.z_topo) > 0)


def test_scaled_solar(inputs):
    s = forcing.scaled_solar(inputs, 1.02)
    assert s.dtype == f32 and s.shape == (abi.NSTEP_YR, inputs.ny)
    assert np.array_equal(s, np.asarray(inputs.sw_solar, f32) * f32(1.02))
    assert np.array_equal(forcing.scaled_solar(inputs, 1.0), np.asarray(inputs.sw_solar, f32))


def test_case3_tables_are_what_the_gpu_case_asks_for(inputs):
    space, season, solar, f = forcing_mirror.case3(inputs)
    assert set(np.unique(space)) == {f32(0), f32(0.25), f32(1)} and set(np.unique(season)) == {f32(0), f32(0.5), f32(1)}
    assert (np.diff(space, axis=1) != 0).any(axis=1).all() and (np.diff(space, axis=0) != 0).any(axis=0).all()
    assert (space[0] > 0).all() and (space[-1] > 0).all()
    for a, b in ((1, 2), (365, 366), (729, 730)):
        assert season[a - 1] != season[b - 1], (a, b)
    assert solar.shape == (abi.NSTEP_YR, inputs.ny) and (solar >= 0).all() and not np.array_equal(solar, inputs.sw_solar)
    assert f.scale == f32(1.02) and f.co2_ref == f32(298.0)


def test_header_and_exports_carry_the_two_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    from greb_climate_model_amd import engine
    for name in ("greb_engine_set_forcing_tables", "greb_engine_set_member_forcing"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in engine.EXPORTS and hasattr(lib, name), name
    m = re.search(r"typedef struct greb_member_forcing \{(.*?)\} greb_member_forcing;", hdr, re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", m.group(1))
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(abi.GrebMemberForcing._fields_)
    assert C.sizeof(abi.GrebMemberForcing) == 16
    assert int(re.search(r"#define\s+GREB_MAX_FORCING_TABLES\s+(\d+)", hdr).group(1)) == abi.MAX_FORCING_TABLES == 16
    assert hasattr(engine.Engine, "set_forcing_tables") and hasattr(engine.Engine, "set_member_forcing")


def test_setters_reject_a_null_engine(lib):
    """Argument errors come before anything touches a device."""
    w = np.ones((1, 48, 96), f32)
    f = (abi.GrebMemberForcing * 1)()
    for rc in (lib.greb_engine_set_forcing_tables(None, 1, abi.fptr(w), None, 0, None),
               lib.greb_engine_set_forcing_tables(None, 0, None, None, 0, None),
               lib.greb_engine_set_member_forcing(None, f), lib.greb_engine_set_member_forcing(None, None)):
        assert rc in (-1, -3), rc
    lib.greb_engine_last_error.restype = C.c_char_p
    assert b"no engine" in lib.greb_engine_last_error(None)
