"""GPU: the on-device diagnostics (csrc/greb_diag.hip) against diag.reduce_reference, the numpy fp64 statement of the
three products.

Tolerance of every comparison with the mirror: 1 fp32 ulp of the mirror's value (np.spacing).  It is derived, not
measured: device and mirror add fp64 products of the same weights to the same fp32 data in fp64 -- with the test data
strictly positive there is no cancellation, so the two fp64 sums agree to ~1e-13 relative whatever the order -- and only
the final rounding to fp32 can fall on the other side of a rounding boundary."""
import types

import numpy as np
import pytest

from greb_climate_model_amd import abi, diag, engine, workload

pytestmark = pytest.mark.gpu

LO = np.array([220.0, 220.0, 271.0, 1e-3, 0.05], np.float32)  # Tsurf, Tair, Tocean [K], q [kg/kg], albedo
HI = np.array([310.0, 300.0, 303.0, 2e-2, 0.80], np.float32)


def synth(n, ny, nx, seed):
    """Strictly positive fp32 records of physical magnitude, [n][12][5][ny][nx]."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 12, 5, ny, nx), dtype=np.float32)
    x *= (HI - LO)[:, None, None]
    x += LO[:, None, None]
    assert x.dtype == np.float32 and x.min() > 0
    return x


def regions_for(nx, ny, seed=5):
    """The standard regions of the grid plus one region of fractional weights."""
    if nx % 96 == 0 and ny % 48 == 0:
        b = workload.load_basis()
        up = (lambda a: a) if (ny, nx) == (48, 96) else (lambda a: workload._upsample2d(a, ny, nx))
        src = types.SimpleNamespace(nx=nx, ny=ny, z_topo=up(b["topography"]), glacier=up(b["glacier"]))
    else:  # a grid the workload has no boundary data for: smooth synthetic continents and polar caps
        lat = np.deg2rad(diag.latitudes(ny))[:, None]
        lon = (np.arange(nx) + 0.5)[None, :] * 2 * np.pi / nx
        src = types.SimpleNamespace(nx=nx, ny=ny, z_topo=(1000.0 * np.sin(2 * lon) * np.cos(3 * lat) + 100.0).astype(np.float32),
                                    glacier=(np.abs(lat) > 1.3).astype(np.float32) * np.ones((1, nx), np.float32))
    r = diag.standard_regions(src)
    r["fractional"] = np.random.default_rng(seed).uniform(0.0, 1.0, (ny, nx)).astype(np.float32)
    return r


def within_one_ulp(got, ref64, label):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref64.shape, (label, got.dtype, got.shape, ref64.shape)
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref64) / ulp
    print(f"{label}: max |device - mirror| = {err.max():.3f} ulp over {err.size} values")
    assert err.max() <= 1.0, (label, float(err.max()))


def check_against_mirror(res, x, weights, label):
    """res: Result of numpy arrays [n]...; x: [n][12][5][ny][nx].  The mirror runs member by member (fp64 copies)."""
    for k in range(x.shape[0]):
        reg, zon, ann = diag.reduce_reference(x[k], weights)
        within_one_ulp(res.regions[k], reg, f"{label} member {k} regions")
        within_one_ulp(res.zonal[k], zon, f"{label} member {k} zonal")
        within_one_ulp(res.annual[k], ann, f"{label} member {k} annual")


def to_host(res):
    import torch
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.cpu().numpy()
    return diag.Result(f(res.regions), f(res.zonal), f(res.annual), None, res.names)


@pytest.mark.parametrize("n", [1, 7, 64])
@pytest.mark.parametrize("nx,ny", [(96, 48), (192, 96), (384, 192), (100, 37)])
def test_reduce_dev_against_mirror(nx, ny, n):
    import torch
    r = regions_for(nx, ny)
    plan = diag.Plan(nx, ny, r)
    assert plan.nr == 10
    x = synth(n, ny, nx, seed=1000 + nx + n)
    res = to_host(diag.reduce_dev(plan, torch.from_numpy(x).cuda()))
    check_against_mirror(res, x, plan.weights, f"{nx}x{ny} n={n}")
    plan.close()


@pytest.mark.parametrize("nx,ny", [(96, 48), (384, 192), (100, 37)])
def test_deterministic_and_independent_of_the_batch(nx, ny):
    import torch
    plan = diag.Plan(nx, ny, regions_for(nx, ny))
    xd = torch.from_numpy(synth(7, ny, nx, seed=77)).cuda()
    a, b = to_host(diag.reduce_dev(plan, xd)), to_host(diag.reduce_dev(plan, xd))
    for name in ("regions", "zonal", "annual"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for k in (0, 3, 6):
        one = to_host(diag.reduce_dev(plan, xd[k:k + 1].contiguous()))
        for name in ("regions", "zonal", "annual"):
            assert np.array_equal(getattr(one, name)[0], getattr(a, name)[k]), (name, k)
    plan.close()


@pytest.mark.parametrize("nx,ny", [(96, 48), (100, 37)])
def test_each_single_flag_gives_the_numbers_of_the_full_call(nx, ny):
    import torch
    plan = diag.Plan(nx, ny, regions_for(nx, ny))
    xd = torch.from_numpy(synth(5, ny, nx, seed=9)).cuda()
    full = to_host(diag.reduce_dev(plan, xd))
    for bit, name in ((abi.D_REGIONS, "regions"), (abi.D_ZONAL, "zonal"), (abi.D_ANNUAL, "annual")):
        one = to_host(diag.reduce_dev(plan, xd, what=bit))
        assert np.array_equal(getattr(one, name), getattr(full, name)), name
        assert [getattr(one, o) is None for o in ("regions", "zonal", "annual")].count(True) == 2
    two = to_host(diag.reduce_dev(plan, xd, what=abi.D_REGIONS | abi.D_ANNUAL))
    assert two.zonal is None and np.array_equal(two.regions, full.regions) and np.array_equal(two.annual, full.annual)
    plan.close()


def _same_engine_state(a, b, yr_a, yr_b):
    assert np.array_equal(yr_a, yr_b), "yearly differs"
    for m in range(a.nm):
        assert np.array_equal(a.state(m), b.state(m)), f"state of member {m} differs"


def test_run_diag_against_run(inputs, params):
    """Two identically created engines, flux correction, then the same scenario through run() and run_diag()."""
    co2 = np.array([[340.0, 350.0], [680.0, 700.0], [1020.0, 1000.0]], np.float32)
    plan = diag.Plan(inputs.nx, inputs.ny, regions_for(inputs.nx, inputs.ny))
    ea, eb, ec = (engine.Engine(inputs, params, n_members=3) for _ in range(3))
    for e in (ea, eb, ec):
        e.flux_correction(1)
    mon, yr_a = ea.run(2, co2)
    res = eb.run_diag(2, co2, plan)
    assert res.regions.shape == (3, 2, 12, 5, 10) and res.zonal.shape == (3, 2, 12, 5, 48) and res.annual.shape == (3, 2, 5, 48, 96)
    for y in range(2):
        check_against_mirror(diag.Result(res.regions[:, y], res.zonal[:, y], res.annual[:, y], None, res.names), mon[:, y],
                             plan.weights, f"run_diag year {y}")
    _same_engine_state(ea, eb, yr_a, res.yearly)
    # one call of two years == two calls of one year, bit for bit
    r1, r2 = ec.run_diag(1, co2[:, :1], plan), ec.run_diag(1, co2[:, 1:], plan)
    for name in ("regions", "zonal", "annual", "yearly"):
        assert np.array_equal(np.concatenate([getattr(r1, name), getattr(r2, name)], axis=1), getattr(res, name)), name
    _same_engine_state(eb, ec, res.yearly[:, 1:], r2.yearly)
    # and run() continues from a run_diag() as from a run()
    mon_a, yr2_a = ea.run(1, 500.0)
    mon_b, yr2_b = eb.run(1, 500.0)
    assert np.array_equal(mon_a, mon_b) and np.array_equal(yr2_a, yr2_b)
    for e in (ea, eb, ec):
        e.close()
    plan.close()


def test_run_diag_five_years_reuse_both_output_slots(inputs, params):
    """One call of five years: the products of years 2, 3 and 4 are made in an output slot that an earlier year's products
    must have left first, in both parities.  The CO2 differs from year to year and between the members, so a product
    delivered from the wrong slot, or before its kernel, is not the mirror's."""
    co2 = np.array([[340.0, 400.0, 480.0, 560.0, 680.0], [1020.0, 900.0, 800.0, 700.0, 600.0]], np.float32)
    plan = diag.Plan(inputs.nx, inputs.ny, regions_for(inputs.nx, inputs.ny))
    ea, eb, ec = (engine.Engine(inputs, params, n_members=2) for _ in range(3))
    for e in (ea, eb, ec):
        e.flux_correction(1)
    mon, yr_a = ea.run(5, co2)
    res = eb.run_diag(5, co2, plan)
    for y in range(5):
        check_against_mirror(diag.Result(res.regions[:, y], res.zonal[:, y], res.annual[:, y], None, res.names), mon[:, y],
                             plan.weights, f"run_diag year {y} of 5")
    _same_engine_state(ea, eb, yr_a, res.yearly)
    # one call of five years == five calls of one year, bit for bit
    parts = [ec.run_diag(1, co2[:, y:y + 1], plan) for y in range(5)]
    for name in ("regions", "zonal", "annual", "yearly"):
        assert np.array_equal(np.concatenate([getattr(r, name) for r in parts], axis=1), getattr(res, name)), name
    _same_engine_state(eb, ec, res.yearly[:, 4:], parts[-1].yearly)
    for e in (ea, eb, ec):
        e.close()
    plan.close()


def test_run_diag_against_run_any_grid(params):
    inp = workload.make_inputs(192, 96)
    plan = diag.Plan(192, 96, regions_for(192, 96))
    ea, eb = engine.Engine(inp, params), engine.Engine(inp, params)
    for e in (ea, eb):
        e.flux_correction(1)
    mon, yr_a = ea.run(1, 680.0)
    res = eb.run_diag(1, 680.0, plan)
    check_against_mirror(diag.Result(res.regions[:, 0], res.zonal[:, 0], res.annual[:, 0], None, res.names), mon[:, 0],
                         plan.weights, "192x96 run_diag")
    _same_engine_state(ea, eb, yr_a, res.yearly)
    ea.close(); eb.close(); plan.close()


def test_run_diag_single_flags_and_errors(inputs, params):
    plan = diag.Plan(inputs.nx, inputs.ny, regions_for(inputs.nx, inputs.ny))
    co2 = [[400.0], [800.0]]
    es = [engine.Engine(inputs, params, n_members=2) for _ in range(4)]
    full = es[0].run_diag(1, co2, plan)
    for e, (bit, name) in zip(es[1:], ((abi.D_REGIONS, "regions"), (abi.D_ZONAL, "zonal"), (abi.D_ANNUAL, "annual"))):
        one = e.run_diag(1, co2, plan, what=bit)
        assert np.array_equal(getattr(one, name), getattr(full, name)), name
        assert np.array_equal(one.yearly, full.yearly)
        _same_engine_state(es[0], e, full.yearly, one.yearly)
    other = diag.Plan(100, 37)
    with pytest.raises(engine.GrebError) as ei:
        es[0].run_diag(1, co2, other)
    assert ei.value.code == -1 and "100 x 37" in str(ei.value) and "96 x 48" in str(ei.value)
    _same_engine_state(es[0], es[1], full.yearly, full.yearly)  # the refused call left the engine alone
    for e in es:
        e.close()
    plan.close(); other.close()


def test_products_pinned_to_the_reference(inputs, params):
    """tests/golden/run_short_g96.npz holds the reference's own 24 monthly records of this configuration.  A mean with
    non-negative normalised weights cannot move further than the fields did, so every product lies within
    max |engine field - reference field| of the mirror applied to the REFERENCE's record (+ 1 ulp for the product's
    own rounding); the field difference is measured here from run() of a twin engine -- no new tolerance."""
    from conftest import load_golden
    g = load_golden("run_short_g96.npz")["monthly"].reshape(2, 12, 5, 48, 96)
    plan = diag.Plan(96, 48, regions_for(96, 48))
    ea, eb = engine.Engine(inputs, params), engine.Engine(inputs, params)
    for e in (ea, eb):
        e.flux_correction(1)
    mon, _ = ea.run(2, 680.0)
    res = eb.run_diag(2, 680.0, plan)
    moved = np.abs(mon[0].astype(np.float64) - g.astype(np.float64)).max(axis=(-2, -1))  # [year][month][var]
    days = np.asarray(abi.JDAY_MON, np.float64)
    for y in range(2):
        reg, zon, ann = diag.reduce_reference(g[y], plan.weights)
        ulp = lambda ref: np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        d_reg = np.abs(res.regions[0, y].astype(np.float64) - reg)
        d_zon = np.abs(res.zonal[0, y].astype(np.float64) - zon)
        d_ann = np.abs(res.annual[0, y].astype(np.float64) - ann)
        moved_year = (moved[y] * days[:, None]).sum(axis=0) / 365.0  # [var]: the annual mean is itself such a mean
        print(f"year {y}: fields moved <= {moved[y].max(axis=0)}; regions {d_reg.max(axis=(0, 2))} zonal {d_zon.max(axis=(0, 2))} "
              f"annual {d_ann.max(axis=(1, 2))} (per variable)")
        assert (d_reg <= moved[y][:, :, None] + ulp(reg)).all()
        assert (d_zon <= moved[y][:, :, None] + ulp(zon)).all()
        assert (d_ann <= moved_year[:, None, None] + ulp(ann)).all()
    ea.close(); eb.close(); plan.close()


def test_tool_prints_one_json_line():
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "run_diag.py"), "4", "2", "--compare", "--passes", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["members"] == 4 and res["finite"] is True
    assert list(res["warming_last_minus_first_year_K"]) == ["globe", "land", "ocean", "glacier", "NH", "SH", "tropics", "Arctic", "Antarctic"]
    lo, hi = res["warming_last_minus_first_year_K"]["globe"]
    assert hi > lo, "1120 ppm warms more than 280 ppm"
    assert res["run_diag"]["ensemble_years_per_s"] > 0 and res["run_device_out"]["ensemble_years_per_s"] > 0
    assert res["products_bytes_per_ensemble_year"] < res["monthly_bytes_per_ensemble_year"] / 8
