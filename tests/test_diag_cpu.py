"""CPU: the reduced-output interface (include/greb_engine.h: greb_diag_*, greb_engine_run_diag) -- its symbols, its
argument errors (all reported before any device query) -- and the numpy fp64 mirror diag.reduce_reference on cases whose
answer is known exactly.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, diag, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("greb_diag_create", "greb_diag_destroy", "greb_diag_reduce_dev", "greb_engine_run_diag")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


def test_new_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", code), n
        assert n in engine.EXPORTS and hasattr(lib, n), n
    for name, val in (("GREB_D_REGIONS", abi.D_REGIONS), ("GREB_D_ZONAL", abi.D_ZONAL), ("GREB_D_ANNUAL", abi.D_ANNUAL)):
        assert re.search(rf"#define {name}\s+{val}u", code), name
    f90 = open(os.path.join(ROOT, "greb_climate_model_amd", "host", "greb_c_api.f90")).read()
    for n in NEW:
        assert f'name="{n}"' in f90, n


def test_library_has_the_reduction_kernels_for_gfx950(lib):
    from greb_climate_model_amd import codesha
    assert "greb_diag.hip" in build.SOURCES
    for k in ("diag_year_kernel", "diag_regions_kernel"):
        fns = codesha.kernel_functions(build.LIB, k)
        assert len(fns) == 1 and len(next(iter(fns.values()))) > 64, k


def _err(fn):
    with pytest.raises(engine.GrebError) as ei:
        fn()
    assert ei.value.code == -1, ei.value
    return str(ei.value)


def test_plan_argument_errors_name_the_offender(lib):
    ny, nx = 48, 96
    ones = np.ones((ny, nx), np.float32)
    assert "n_regions = 16" in _err(lambda: diag.Plan(nx, ny, {f"r{i}": ones for i in range(16)}))
    diag.Plan(nx, ny, {f"r{i}": ones for i in range(15)}).close()
    msg = _err(lambda: diag.Plan(nx, ny, {"a": ones, "empty": np.zeros((ny, nx), np.float32)}))
    assert "region 2 ('empty') has zero weight" in msg
    for bad in (1.5, -0.25, np.nan, np.inf):
        w = ones.copy()
        w[7, 11] = bad
        msg = _err(lambda: diag.Plan(nx, ny, {"a": ones, "b": w}))
        assert "region 2 ('b')" in msg and "row 7, column 11" in msg and "not in [0, 1]" in msg, msg
    for gx, gy in ((95, 48), (8, 48), (96, 4), (96, 193)):
        assert f"grid {gx} x {gy}" in _err(lambda: diag.Plan(gx, gy))
    assert "shape" in _err(lambda: diag.Plan(nx, ny, {"a": np.ones((ny, nx + 4), np.float32)}))
    h = C.c_void_p()
    assert lib.greb_diag_create(nx, ny, None, 2, C.byref(h)) == -1 and not h
    assert b"region_w is NULL" in lib.greb_engine_last_error(None)
    assert lib.greb_diag_create(nx, ny, None, 0, None) == -1
    assert lib.greb_diag_destroy(None) == 0


def test_reduce_and_run_argument_errors_come_before_any_device_query(lib):
    plan = diag.Plan(96, 48)
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf = np.zeros(64, np.float32)
    p = abi.fptr(buf)
    aligned = C.c_void_p((buf.ctypes.data + 15) & ~15)
    assert lib.greb_diag_reduce_dev(None, 0, aligned, 1, aligned, None, None, None) == -1 and "no plan" in last()
    assert lib.greb_diag_reduce_dev(plan.h, 0, None, 1, aligned, None, None, None) == -1 and "monthly_year_dev is NULL" in last()
    assert lib.greb_diag_reduce_dev(plan.h, 0, aligned, 0, aligned, None, None, None) == -1 and "n_members = 0" in last()
    assert lib.greb_diag_reduce_dev(plan.h, 0, aligned, 1, None, None, None, None) == -1 and "all NULL" in last()
    misaligned = C.c_void_p(aligned.value + 4)
    assert lib.greb_diag_reduce_dev(plan.h, 0, misaligned, 1, aligned, None, None, None) == -1 and "monthly_year_dev is not 16-byte" in last()
    assert lib.greb_diag_reduce_dev(plan.h, 0, aligned, 1, None, None, misaligned, None) == -1 and "annual_dev is not 16-byte" in last()
    # run_diag: the plan and `what` are checked first, so these are decided without an engine (and without a GPU)
    run = lib.greb_engine_run_diag
    assert run(None, 1, p, None, C.c_uint(7), p, p, p, None) == -1 and "no plan" in last()
    assert run(None, 1, p, plan.h, C.c_uint(0), p, p, p, None) == -1 and "`what` = 0" in last()
    assert run(None, 1, p, plan.h, C.c_uint(8), p, p, p, None) == -1 and "`what` = 8" in last()
    for bit, name in ((abi.D_REGIONS, "regions"), (abi.D_ZONAL, "zonal"), (abi.D_ANNUAL, "annual")):
        ptr = [None if n == name else p for n in ("regions", "zonal", "annual")]
        assert run(None, 1, p, plan.h, C.c_uint(diag.ALL), *ptr, None) == -1
        assert f"selected but `{name}` is NULL" in last(), last()
        assert run(None, 1, p, plan.h, C.c_uint(diag.ALL & ~bit), *ptr, None) == -1 and "bad argument" in last()  # (no engine)
    plan.close()


def test_reduce_dev_without_a_gpu_is_a_loud_error(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    plan = diag.Plan(96, 48)
    buf = np.zeros(64, np.float32)
    aligned = C.c_void_p((buf.ctypes.data + 15) & ~15)
    assert lib.greb_diag_reduce_dev(plan.h, 0, aligned, 1, aligned, None, None, None) == -2
    assert b"no CPU path" in lib.greb_engine_last_error(None)


# ---- the mirror on cases with a known answer -------------------------------------------------------------------------
def _weights(ny, nx, seed=3):
    rng = np.random.default_rng(seed)
    lat = diag.latitudes(ny)[:, None] * np.ones((1, nx))
    return np.stack([(lat > 0).astype(np.float32), (np.abs(lat) < 30).astype(np.float32),
                     rng.uniform(0.0, 1.0, (ny, nx)).astype(np.float32)])


@pytest.mark.parametrize("nx,ny", [(96, 48), (100, 37)])
def test_mirror_constant_field_comes_back_exactly(nx, ny):
    w = _weights(ny, nx)
    for c in (np.float32(287.65), np.float32(0.0123), np.float32(0.31)):
        x = np.full((2, 12, 5, ny, nx), c, np.float32)
        reg, zon, ann = diag.reduce_reference(x, w)
        assert reg.shape == (2, 12, 5, 4) and zon.shape == (2, 12, 5, ny) and ann.shape == (2, 5, ny, nx)
        for a in (reg, zon, ann):
            assert np.array_equal(a.astype(np.float32), np.full(a.shape, c, np.float32))


def test_mirror_field_varying_with_longitude_gives_its_row_mean():
    ny, nx = 48, 96
    rng = np.random.default_rng(11)
    row = rng.uniform(250.0, 300.0, nx).astype(np.float32)
    x = np.broadcast_to(row, (12, 5, ny, nx))
    mean = row.astype(np.float64).mean()
    reg, zon, ann = diag.reduce_reference(x, _weights(ny, nx)[:2])  # globe, NH, tropics: every row whole
    assert np.abs(zon - mean).max() < 1e-12 * mean
    assert np.abs(reg - mean).max() < 1e-12 * mean
    assert np.abs(ann - row.astype(np.float64)).max() < 1e-12 * mean


def test_annual_weights_sum_to_365_and_weigh_by_days():
    assert sum(abi.JDAY_MON) == 365 and len(abi.JDAY_MON) == 12
    x = np.zeros((12, 5, 5, 12), np.float32)
    x[1] = 365.0  # February alone
    ann = diag.reduce_reference(x)[2]
    assert np.array_equal(ann, np.full((5, 5, 12), 28.0))
    series = np.arange(12, dtype=np.float64)[:, None, None] * np.ones((12, 5, 3))
    want = float((np.arange(12) * np.asarray(abi.JDAY_MON)).sum() / 365.0)
    assert np.allclose(diag.annual_from_monthly(series), want, rtol=0, atol=1e-13)
    assert diag.annual_from_monthly(series).shape == (5, 3)


def test_mirror_global_mean_is_the_hand_rolled_one(inputs):
    """conftest.global_mean_fp64 is the unweighted mean the console prints; region 0 here is AREA weighted.  On a field
    that is constant along every row the two differ exactly by the weighting: checked against a direct formula."""
    ny, nx = inputs.ny, inputs.nx
    lat = diag.latitudes(ny)
    prof = (250.0 + 40.0 * np.cos(np.deg2rad(lat))).astype(np.float32)
    x = np.broadcast_to(prof[:, None], (12, 5, ny, nx))
    c = np.cos(np.deg2rad(lat))
    want = float((prof.astype(np.float64) * c).sum() / c.sum())
    reg = diag.reduce_reference(x)[0]
    assert reg.shape == (12, 5, 1) and np.abs(reg - want).max() < 1e-12 * want


def test_standard_regions_partition_the_workload(inputs):
    r = diag.standard_regions(inputs)
    assert list(r) == ["land", "ocean", "glacier", "NH", "SH", "tropics", "Arctic", "Antarctic"]
    for k, v in r.items():
        assert v.shape == (inputs.ny, inputs.nx) and v.dtype == np.float32 and set(np.unique(v)) <= {0.0, 1.0}, k
        assert v.sum() > 0, f"{k} is empty"
    assert np.array_equal(r["land"] + r["ocean"], np.ones_like(r["land"]))
    assert np.array_equal(r["NH"] + r["SH"], np.ones_like(r["NH"]))
    lat = diag.latitudes(inputs.ny)
    assert np.array_equal(r["Arctic"][:, 0] > 0, lat > 66) and np.array_equal(r["Antarctic"][:, 0] > 0, lat < -66)
    plan = diag.Plan(inputs.nx, inputs.ny, r)  # the library accepts them: no region is empty, all weights in [0, 1]
    assert plan.names == ("globe",) + tuple(r) and plan.nr == 9
    plan.close()


def test_tool_parses_its_command_line():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_diag.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--compare" in out.stdout and "members" in out.stdout
