"""CPU: the climatology interface (include/greb_engine.h: greb_clim_*, greb_engine_run_clim) -- its symbols, its kernels
in the built library, its argument errors (all reported before any device query) -- and the numpy fp64 mirror
clim.reference on cases whose answer is known exactly.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, clim, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("greb_clim_create", "greb_clim_destroy", "greb_clim_add_year_dev", "greb_clim_finish_dev", "greb_engine_run_clim")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


def test_new_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    f90 = open(os.path.join(ROOT, "greb_climate_model_amd", "host", "greb_c_api.f90")).read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", code), n
        assert n in engine.EXPORTS and hasattr(lib, n), n
        assert f'name="{n}"' in f90, n
    for name, val in (("GREB_C_MEAN", abi.C_MEAN), ("GREB_C_SEASONS", abi.C_SEASONS), ("GREB_C_TREND", abi.C_TREND),
                      ("GREB_C_RESPONSE", abi.C_RESPONSE)):
        assert re.search(rf"#define {name}\s+{val}u", code), name
    assert (abi.C_MEAN, abi.C_SEASONS, abi.C_TREND, abi.C_RESPONSE) == (1, 2, 4, 8)
    assert clim.SEASONS == ("DJF", "MAM", "JJA", "SON", "ANN")


def test_library_has_the_climatology_kernels_for_gfx950(lib):
    from greb_climate_model_amd import codesha
    assert "greb_clim.hip" in build.SOURCES and "greb_clim.h" in build.HEADERS
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["greb_clim.hip"]  # the operation order is the definition of the results
    add = codesha.kernel_functions(build.LIB, "clim_add_year_kernel")
    assert len(add) == 4 and all(len(c) > 64 for c in add.values()), sorted(add)  # {sums, sums + trend} x {store, add}
    fin = codesha.kernel_functions(build.LIB, "clim_finish_kernel")
    assert len(fin) == 1 and len(next(iter(fin.values()))) > 64


def _err(fn):
    with pytest.raises(engine.GrebError) as ei:
        fn()
    assert ei.value.code == -1, ei.value
    return str(ei.value)


def test_plan_argument_errors_name_the_offender(lib):
    nx, ny = 96, 48
    clim.Plan(nx, ny, 3, control=[-1, 0, 2]).close()  # a member may be its own control
    clim.Plan(nx, ny, 1).close()
    msg = _err(lambda: clim.Plan(nx, ny, 3, control=[-1, 0, 3]))
    assert "member 2" in msg and "control = 3" in msg, msg
    msg = _err(lambda: clim.Plan(nx, ny, 3, control=[-2, 0, 0]))
    assert "member 0" in msg and "control = -2" in msg, msg
    assert "`what` = 0" in _err(lambda: clim.Plan(nx, ny, 3, what=0))
    assert "`what` = 16" in _err(lambda: clim.Plan(nx, ny, 3, what=16))
    assert "`what` = 17" in _err(lambda: clim.Plan(nx, ny, 3, what=abi.C_MEAN | 16))
    msg = _err(lambda: clim.Plan(nx, ny, 3, control=[-1, 0, 0], what=abi.C_RESPONSE | abi.C_TREND))
    assert "GREB_C_RESPONSE needs GREB_C_MEAN or GREB_C_SEASONS" in msg
    msg = _err(lambda: clim.Plan(nx, ny, 3, what=abi.C_RESPONSE | abi.C_MEAN))
    assert "`control` is NULL" in msg
    assert "n_members = 0" in _err(lambda: clim.Plan(nx, ny, 0))
    for gx, gy in ((95, 48), (8, 48), (96, 4), (96, 193)):  # the grids diag.Plan rejects
        assert f"grid {gx} x {gy}" in _err(lambda: clim.Plan(gx, gy, 1))
    assert "3 integers" in _err(lambda: clim.Plan(nx, ny, 3, control=[0, 0]))
    assert lib.greb_clim_create(nx, ny, 1, None, C.c_uint(1), None) == -1
    assert lib.greb_clim_destroy(None) == 0


def _aligned():
    buf = np.zeros(64, np.float32)
    return buf, C.c_void_p((buf.ctypes.data + 15) & ~15)


def test_dev_argument_errors_come_before_any_device_query(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, ok = _aligned()
    bad = C.c_void_p(ok.value + 4)
    plan = clim.Plan(96, 48, 2, control=[-1, 0])
    add, fin = lib.greb_clim_add_year_dev, lib.greb_clim_finish_dev
    assert add(None, 0, ok, 0, None) == -1 and "no plan" in last()
    assert add(plan.h, 0, None, 0, None) == -1 and "monthly_year_dev is NULL" in last()
    assert add(plan.h, 0, bad, 0, None) == -1 and "monthly_year_dev is not 16-byte aligned" in last()
    assert add(plan.h, 0, ok, 1, None) == -1 and "k = 1, but 0 years were added" in last()
    assert add(plan.h, 0, ok, -1, None) == -1 and "k = -1" in last()
    assert fin(None, 0, 1, ok, ok, ok, ok, ok, None) == -1 and "no plan" in last()
    for i, name in enumerate(clim.PRODUCTS):  # the plan selects all five: each needs a pointer, 16-byte aligned
        assert fin(plan.h, 0, 1, *[None if j == i else ok for j in range(5)], None) == -1
        assert f"selected but `{name}_dev` is NULL" in last(), last()
        assert fin(plan.h, 0, 1, *[bad if j == i else ok for j in range(5)], None) == -1
        assert f"{name}_dev is not 16-byte aligned" in last(), last()
    assert fin(plan.h, 0, 1, ok, ok, ok, ok, ok, None) == -1 and "n_years = 1, but 0 years were added" in last()
    assert fin(plan.h, 0, 0, ok, ok, ok, ok, ok, None) == -1 and "n_years = 0" in last()
    plan.close()


PERIOD_CASES = (([(0, 2), (1, 2)], "period 1", "overlaps period 0"),
                ([(2, 1), (0, 1)], "period 1", "ascending"),
                ([(0, 1), (3, 2)], "period 1", "not inside the run's years 0 ... 3"),
                ([(-1, 2)], "period 0", "not inside"),
                ([(0, 5)], "period 0", "not inside"),
                ([(1, 0)], "period 0", "has no years"))


def test_run_clim_argument_errors_are_decided_without_an_engine(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, ok = _aligned()
    p = abi.fptr(buf)
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    plan = clim.Plan(96, 48, 2, control=[-1, 0])
    run = lib.greb_engine_run_clim
    one = (ip([0]), ip([1]))
    assert run(None, 1, p, None, 1, *one, p, p, p, p, p, None) == -1 and "no plan" in last()
    assert run(None, 0, p, plan.h, 1, *one, p, p, p, p, p, None) == -1 and "years = 0" in last()
    assert run(None, 1, p, plan.h, 0, *one, p, p, p, p, p, None) == -1 and "n_periods = 0" in last()
    assert run(None, 1, p, plan.h, 1, None, None, p, p, p, p, p, None) == -1 and "NULL" in last()
    for periods, who, what in PERIOD_CASES:
        per = np.asarray(periods, np.int32)
        assert run(None, 4, p, plan.h, len(per), ip(per[:, 0]), ip(per[:, 1]), p, p, p, p, p, None) == -1
        assert who in last() and what in last(), (periods, last())
    for i, name in enumerate(clim.PRODUCTS):
        ptr = [None if j == i else p for j in range(5)]
        assert run(None, 1, p, plan.h, 1, *one, *ptr, None) == -1 and f"selected but `{name}` is NULL" in last(), last()
    assert run(None, 1, p, plan.h, 1, *one, p, p, p, p, p, None) == -1 and "bad argument (engine" in last()
    only_mean = clim.Plan(96, 48, 2, what=abi.C_MEAN)  # unselected products may be NULL: the next check is reached
    assert run(None, 1, p, only_mean.h, 1, *one, p, None, None, None, None, None) == -1 and "bad argument (engine" in last()
    plan.close(); only_mean.close()


def test_dev_calls_without_a_gpu_are_a_loud_error(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    buf, ok = _aligned()
    plan = clim.Plan(96, 48, 1)
    assert lib.greb_clim_add_year_dev(plan.h, 0, ok, 0, None) == -2
    assert b"no CPU path" in lib.greb_engine_last_error(None)
    # finish_dev: its argument checks refuse a plan without years, so the device query is reached only through them
    assert lib.greb_clim_finish_dev(plan.h, 0, 1, ok, ok, ok, None, None, None) == -1
    plan.close()


# ---- the mirror on cases with a known answer -------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("nx,ny", [(96, 48), (100, 37)])
def test_mirror_constant_field_comes_back_exactly(nx, ny):
    for c in (np.float32(287.65), np.float32(0.0123), np.float32(0.31)):
        years = [np.full((2, 12, 5, ny, nx), c, np.float32) for _ in range(4)]
        r = clim.reference(years, control=[-1, 0])
        assert r.mean.shape == r.trend.shape == r.mean_resp.shape == (2, 12, 5, ny, nx)
        assert r.seasons.shape == r.seasons_resp.shape == (2, 5, 5, ny, nx)
        assert r.mean.dtype == r.seasons.dtype == r.trend.dtype == np.float32
        assert np.array_equal(r.mean, np.full(r.mean.shape, c)) and np.array_equal(r.seasons, np.full(r.seasons.shape, c))
        assert not r.trend.any() and not r.mean_resp[1].any() and not r.seasons_resp[1].any()


def test_mirror_season_weights():
    assert sum(abi.JDAY_MON) == 365
    x = np.zeros((1, 12, 5, 5, 12), np.float32)
    x[:, 1] = 365.0  # February alone
    r = clim.reference([x, x])
    ann, djf = r.seasons[0, clim.SEASONS.index("ANN")], r.seasons[0, clim.SEASONS.index("DJF")]
    assert np.array_equal(ann, np.full(ann.shape, 28.0, np.float32))
    assert np.array_equal(djf, np.full(djf.shape, np.float32(28.0 * 365.0 / 90.0)))
    assert not r.seasons[0, 1:4].any()  # MAM, JJA, SON do not see February
    y = np.zeros((1, 12, 5, 5, 12), np.float32)
    y[:, 11], y[:, 0], y[:, 1] = 90.0, 180.0, 270.0  # Dec, Jan, Feb of the same calendar year
    s = clim.reference([y]).seasons[0]
    assert np.array_equal(s[0], np.full(s[0].shape, 31.0 + 2 * 31.0 + 3 * 28.0, np.float32))  # 31/31/28 over 90
    assert np.array_equal(s[4], np.full(s[4].shape, np.float32((90.0 * 31 + 180.0 * 31 + 270.0 * 28) / 365.0)))
    z = np.zeros((1, 12, 5, 5, 12), np.float32)
    for mo, d in enumerate((92.0, 92.0, 91.0)):
        z[:, 2 + 3 * mo:5 + 3 * mo] = d * (mo + 1)  # MAM = 92, JJA = 184, SON = 273
    s = clim.reference([z]).seasons[0]
    assert [float(s[k].max()) for k in (1, 2, 3)] == [92.0, 184.0, 273.0] and not s[0].any()


@pytest.mark.parametrize("n", [2, 3, 5, 7, 10, 50])
def test_mirror_trend_of_exactly_representable_linear_series(n):
    shape = (2, 12, 5, 5, 12)
    years = []
    for k in range(n):
        x = np.empty(shape, np.float32)
        x[0] = 280.0 + 0.5 * k
        x[1] = 2.0 ** -7 - 2.0 ** -11 * k
        assert x[0, 0, 0, 0, 0] == 280.0 + 0.5 * k and float(x[1, 0, 0, 0, 0]) == 2.0 ** -7 - 2.0 ** -11 * k  # exact in fp32
        years.append(x)
    r = clim.reference(years)
    assert np.array_equal(r.trend[0], np.full(shape[1:], 0.5, np.float32))
    assert np.array_equal(r.trend[1], np.full(shape[1:], -2.0 ** -11, np.float32))
    assert np.array_equal(r.mean[0], np.full(shape[1:], np.float32(280.0 + 0.25 * (n - 1))))


def test_mirror_one_year_response_to_itself_and_no_control():
    rng = np.random.default_rng(4)
    x = (rng.random((3, 12, 5, 5, 12), dtype=np.float32) * 90 + 220).astype(np.float32)
    r = clim.reference([x], control=[-1, 1, 0])
    assert np.array_equal(_bits(r.mean), _bits(x)), "S / 1 is the input"
    assert not r.trend.any(), "one year has no slope"
    assert not r.mean_resp[1].any() and not r.seasons_resp[1].any(), "a member's response to itself is zero"
    assert np.isnan(r.mean_resp[0]).all() and np.isnan(r.seasons_resp[0]).all(), "no control: NaN, not zero"
    assert np.array_equal(r.mean_resp[2], (x[2].astype(np.float64) - x[0].astype(np.float64)).astype(np.float32))
    # products follow the flags
    one = clim.reference([x], control=[-1, 1, 0], what=abi.C_SEASONS | abi.C_RESPONSE)
    assert one.mean is None and one.trend is None and one.mean_resp is None
    assert np.array_equal(_bits(one.seasons), _bits(r.seasons)) and np.array_equal(_bits(one.seasons_resp), _bits(r.seasons_resp))
    none = clim.reference([x])
    assert none.mean_resp is None and none.seasons_resp is None and none.mean is not None


def test_tool_parses_its_command_line():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_clim.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--compare" in out.stdout and "--window" in out.stdout and "members" in out.stdout
