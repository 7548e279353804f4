"""GPU: budget output through the plans -- diag and clim plans with a variable count, the combination stage
(csrc/greb_fluxes.hip) and the four reduced runs over the budget records -- against the numpy mirrors.

The yardsticks.  clim, ens, lin and the combination stage: bit-equal to clim.reference / ens.reference / lin.reference /
budget.combine_reference, as in their state tests.  diag: the fp64 mirror diag.reduce_reference under the rule of
tests/test_gpu_diag.py::within_one_ulp, with one derived addition because budget terms have both signs and their sums may
cancel:

    |got - ref| <= ulp32(ref) + n * 2^-52 * (sum |w x| / sum w)

n the number of addends -- the points of the grid for a region, nx for a zonal mean, 12 for the annual map (day weights).
That is twice the standard bound n * 2^-53 * sum |terms| of an fp64 sum, once for the device's and once for the mirror's;
sum |w x| / sum w is the same mirror applied to |x|."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from greb_climate_model_amd import abi, budget, clim, diag, engine, ens, lin, workload

pytestmark = pytest.mark.gpu

STD = budget.combo(budget.STANDARD)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, names, label):
    """The products `names` of two Results: both None, or equal shape and equal bits."""
    for name in names:
        g, r = getattr(got, name), getattr(ref, name)
        assert (g is None) == (r is None), (label, name)
        if g is None:
            continue
        g, r = np.asarray(g), np.asarray(r)
        assert g.dtype == np.float32 and g.shape == r.shape, (label, name, g.dtype, g.shape, r.shape)
        bad = bits(g) != bits(r)
        print(f"{label} {name}: {int(bad.sum())} of {bad.size} values differ from the mirror")
        assert not bad.any(), (label, name, int(bad.sum()), g[bad][:4], r[bad][:4])


def budget_like(shape, seed):
    """fp32 records of both signs and mixed magnitude with zeros of both signs in them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 3, shape)).astype(np.float32)
    x[rng.random(shape) < 0.05] = 0.0
    x[rng.random(shape) < 0.05] = -0.0
    return x


# ---------------------------------------------------------------- diag plans with a variable count
def synth_signed(n, nv, ny, nx, seed):
    """[n][12][nv][ny][nx]: every variable with its own magnitude and offset, both signs, the last variable's record of
    month 3 exactly zero -- as budget terms are (a switched-off process is a field of zeros)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 12, nv, ny, nx), dtype=np.float32)
    scale = (10.0 ** rng.integers(-7, 3, nv)).astype(np.float32)
    x += rng.uniform(-1.5, 1.5, nv).astype(np.float32)[:, None, None]  # a mean of up to 1.5 standard deviations
    x *= scale[:, None, None]
    x[:, 3, nv - 1] = 0.0
    assert x.dtype == np.float32 and (x < 0).any() and (x > 0).any()
    return x


def regions_for(nx, ny, seed=5):
    lat = np.broadcast_to(diag.latitudes(ny)[:, None], (ny, nx))
    return {"NH": (lat > 0).astype(np.float32), "tropics": (np.abs(lat) < 30).astype(np.float32),
            "fractional": np.random.default_rng(seed).uniform(0.0, 1.0, (ny, nx)).astype(np.float32)}


def within_bound(got, ref64, abs64, n, label):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref64.shape == abs64.shape, (label, got.dtype, got.shape, ref64.shape)
    bound = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64) + n * 2.0 ** -52 * abs64
    err = np.abs(got.astype(np.float64) - ref64)
    print(f"{label}: max |device - mirror| / bound = {(err / bound).max():.3f} over {err.size} values")
    assert (err <= bound).all(), (label, float((err / bound).max()))


def diag_against_mirror(res, x, weights, label):
    """res: regions [n]..., zonal, annual (numpy, or None); x [n][12][V][ny][nx]."""
    ny, nx = x.shape[-2:]
    for k in range(x.shape[0]):
        ref, mag = diag.reduce_reference(x[k], weights), diag.reduce_reference(np.abs(x[k]), weights)
        for i, (name, n) in enumerate((("regions", ny * nx), ("zonal", nx), ("annual", 12))):
            if getattr(res, name) is not None:
                within_bound(getattr(res, name)[k], ref[i], mag[i], n, f"{label} member {k} {name}")


def diag_to_host(res):
    import torch
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.cpu().numpy()
    return diag.Result(f(res.regions), f(res.zonal), f(res.annual), None, res.names)


@pytest.mark.parametrize("nv", [1, 13, 16])
@pytest.mark.parametrize("nx,ny,n", [(96, 48, 1), (96, 48, 3), (100, 37, 1), (100, 37, 3), (384, 192, 1)])
def test_diag_reduce_dev_with_a_variable_count(nx, ny, n, nv):
    """96 x 48: a partial last band (48 rows in bands of 10); 100 x 37: 25 groups of four per row; 384 x 192: two rows per band,
    96 bands.  Repeated: the same bits; a member alone: the bits it has in the batch."""
    import torch
    r = regions_for(nx, ny)
    plan = diag.Plan(nx, ny, r, n_vars=nv)
    x = synth_signed(n, nv, ny, nx, seed=100 * nv + nx + n)
    xd = torch.from_numpy(x).cuda()
    res = diag_to_host(diag.reduce_dev(plan, xd))
    assert res.regions.shape == (n, 12, nv, 4) and res.zonal.shape == (n, 12, nv, ny) and res.annual.shape == (n, nv, ny, nx)
    diag_against_mirror(res, x, plan.weights, f"{nx}x{ny} n={n} V={nv}")
    assert not res.regions[:, 3, nv - 1].any() and not res.zonal[:, 3, nv - 1].any()  # the record of zeros
    again = diag_to_host(diag.reduce_dev(plan, xd))
    one = diag_to_host(diag.reduce_dev(plan, xd[n - 1:].contiguous()))
    for name in ("regions", "zonal", "annual"):
        assert np.array_equal(bits(getattr(again, name)), bits(getattr(res, name))), name
        assert np.array_equal(bits(getattr(one, name)[0]), bits(getattr(res, name)[n - 1])), name
    with pytest.raises(engine.GrebError) as ei:  # the tensor's count is the plan's
        diag.reduce_dev(plan, torch.zeros((1, 12, nv + 1, ny, nx), device="cuda"))
    assert ei.value.code == -1
    plan.close()


# ---------------------------------------------------------------- clim plans with a variable count
CLIM_NAMES = ("mean", "seasons", "trend", "mean_resp", "seasons_resp")


@pytest.mark.parametrize("nv", [1, 13])
@pytest.mark.parametrize("nx,ny", [(12, 5), (96, 48)])
def test_clim_dev_with_a_variable_count(nx, ny, nv):
    import torch
    control = [-1, 0, 2]
    years = [synth_signed(3, nv, ny, nx, seed=7 * nv + nx + k) for k in range(3)]
    plan = clim.Plan(nx, ny, 3, control=control, n_vars=nv)
    for k, x in enumerate(years):
        clim.add_year_dev(plan, torch.from_numpy(x).cuda(), k)
    got = clim.finish_dev(plan, 3)
    torch.cuda.synchronize()
    got = clim.Result(*[getattr(got, n).cpu().numpy() for n in CLIM_NAMES])
    assert got.mean.shape == (3, 12, nv, ny, nx) and got.seasons_resp.shape == (3, 5, nv, ny, nx)
    same_bits(got, clim.reference(years, control), CLIM_NAMES, f"clim {nx}x{ny} V={nv}")
    assert np.isnan(got.mean_resp[0]).all() and not got.mean_resp[2].any()  # no control; its own control
    plan.close()


# ---------------------------------------------------------------- the combination stage
@pytest.mark.parametrize("n,ny,nx", [(1, 1, 4), (2, 5, 12), (3, 48, 96)], ids=["np4", "np60", "96x48x3"])
def test_combine_dev_against_the_mirror(n, ny, nx):
    """np = 4: one lane per (member, month); np = 60: lanes of one record in two wavefront rows; 96 x 48 with 3 members: 162
    workgroups, the last one partly idle.  The three standard rows and a row of one term."""
    import torch
    rows = dict(budget.STANDARD)
    rows["rain_alone"] = {"dq_rain": 1}
    cb = budget.combo(rows)
    b = budget_like((n, 12, abi.NBUDGET, ny, nx), seed=n + nx)
    got = budget.combine_dev(cb, torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ref = budget.combine_reference(cb, b)
    assert got.shape == ref.shape == (n, 12, 4, ny, nx)
    bad = bits(got) != bits(ref)
    print(f"combine {n}x{ny}x{nx}: {int(bad.sum())} of {bad.size} values differ from the mirror")
    assert not bad.any(), (got[bad][:4], ref[bad][:4])
    assert np.array_equal(bits(got[:, :, 3]), bits(b[:, :, abi.B_DQ_RAIN]))  # a copy, -0.0 included
    assert np.signbit(got[:, :, 3][got[:, :, 3] == 0]).any()
    scaled = budget.combine_dev(np.float32(-0.3) * np.eye(13, dtype=np.float32)[[12, 0]], torch.from_numpy(b).cuda()).cpu().numpy()
    assert np.array_equal(bits(scaled[:, :, 0]), bits(np.float32(-0.3) * b[:, :, 12]))
    assert np.array_equal(bits(scaled[:, :, 1]), bits(np.float32(-0.3) * b[:, :, 0]))


# ---------------------------------------------------------------- the four reduced runs
@pytest.fixture(scope="module")
def spun(inputs, params):
    """One flux-correction year of the 96x48 engine: its corrections and spun-up state, which every engine below starts from."""
    e = engine.Engine(inputs, params)
    e.flux_correction(1)
    out = e.get_corrections(0)
    e.close()
    return out


def primed(inputs, params, spun, n, **kw):
    e = engine.Engine(inputs, params, n_members=n, **kw)
    e.set_corrections(*spun)
    return e


def same_engine_state(a, b, yr_a, yr_b, label=""):
    assert np.array_equal(yr_a, yr_b), f"{label}: yearly differs"
    for m in range(a.nm):
        assert np.array_equal(a.state(m), b.state(m)), f"{label}: state of member {m} differs"


CO2_3x2 = np.array([[340.0, 350.0], [680.0, 700.0], [1020.0, 1000.0]], np.float32)
ENS_GROUP, ENS_CONTROL, ENS_PROBS = [-1, 0, 0], [-1, 0, 0], [0.0, 0.5, 1.0]
LIN_W = np.array([[1 / 3, 1 / 3, 1 / 3], [0.0, -1.0, 1.0]])
LIN_D = np.array([[1.0, 0.0], [1.0, -0.5], [1.0, 0.5]])
CLIM_CONTROL = [-1, 0, 0]
ENS_NAMES, LIN_NAMES = ("mean", "var", "min", "max", "quant"), ("coef", "rss")


@pytest.fixture(scope="module")
def twin_runs(inputs, params, spun):
    """Engine A: run_budget over two years; engine R: run() over the same.  What the reduced runs are held to."""
    a, r = primed(inputs, params, spun, 3), primed(inputs, params, spun, 3)
    _, bud, yr_a = a.run_budget(2, CO2_3x2, want_monthly=False)
    mon, yr_r = r.run(2, CO2_3x2)
    assert np.array_equal(yr_a, yr_r)
    state = [r.state(m) for m in range(3)]
    a.close(); r.close()
    return bud, yr_r, state


@pytest.mark.parametrize("records", ["budget", STD], ids=["terms", "standard_rows"])
def test_reduced_budget_runs_against_run_budget(inputs, params, spun, twin_runs, records):
    bud, yearly, state = twin_runs
    names = budget.record_names(records)
    V = len(names)
    assert V == (13 if isinstance(records, str) else 3)
    x = bud if isinstance(records, str) else budget.combine_reference(records, bud)  # [3][2][12][V][48][96]
    nx, ny = inputs.nx, inputs.ny

    def check_engine(e, res, label):
        assert np.array_equal(res.yearly, yearly), f"{label}: yearly is not run()'s"
        for m in range(3):
            assert np.array_equal(e.state(m), state[m]), f"{label}: state of member {m} is not run()'s"
        assert res.vars == names

    # diag
    dplan = diag.Plan(nx, ny, regions_for(nx, ny), n_vars=V)
    eb = primed(inputs, params, spun, 3)
    rd = eb.run_diag(2, CO2_3x2, dplan, records=records)
    assert rd.regions.shape == (3, 2, 12, V, 4) and rd.zonal.shape == (3, 2, 12, V, ny) and rd.annual.shape == (3, 2, V, ny, nx)
    for y in range(2):
        diag_against_mirror(diag.Result(rd.regions[:, y], rd.zonal[:, y], rd.annual[:, y], None, rd.names), x[:, y],
                            dplan.weights, f"run_budget_diag V={V} year {y}")
    check_engine(eb, rd, "diag")
    assert eb.describe()["budget_runs"] == 1
    # clim: one period of both years
    cplan = clim.Plan(nx, ny, 3, control=CLIM_CONTROL, n_vars=V)
    ec = primed(inputs, params, spun, 3)
    rc = ec.run_clim(2, CO2_3x2, cplan, [(0, 2)], records=records)
    assert rc.mean.shape == (3, 1, 12, V, ny, nx) and rc.seasons.shape == (3, 1, 5, V, ny, nx)
    same_bits(clim.Result(*[getattr(rc, n)[:, 0] for n in CLIM_NAMES]), clim.reference([x[:, 0], x[:, 1]], CLIM_CONTROL),
              CLIM_NAMES, f"run_budget_clim V={V}")
    check_engine(ec, rc, "clim")
    # ens
    splan = ens.Plan(nx, ny, 3, ENS_GROUP, control=ENS_CONTROL, probs=ENS_PROBS)
    es = primed(inputs, params, spun, 3)
    rs = es.run_ens(2, CO2_3x2, splan, records=records)
    assert rs.mean.shape == (1, 2, 12, V, ny, nx) and rs.quant.shape == (1, 2, 3, 12, V, ny, nx)
    for y in range(2):
        same_bits(ens.Result(*[getattr(rs, n)[:, y] for n in ENS_NAMES]), ens.reference(x[:, y], ENS_GROUP, ENS_CONTROL, ENS_PROBS),
                  ENS_NAMES, f"run_budget_ens V={V} year {y}")
    check_engine(es, rs, "ens")
    # lin
    lplan = lin.Plan(nx, ny, 3, LIN_W, design=LIN_D)
    el = primed(inputs, params, spun, 3)
    rl = el.run_lin(2, CO2_3x2, lplan, records=records)
    assert rl.coef.shape == (2, 2, 12, V, ny, nx) and rl.rss.shape == (2, 12, V, ny, nx)
    for y in range(2):
        same_bits(lin.Result(rl.coef[:, y], rl.rss[y]), lin.reference(x[:, y], LIN_W, design=LIN_D), LIN_NAMES,
                  f"run_budget_lin V={V} year {y}")
    check_engine(el, rl, "lin")

    # one call of two years == two calls of one year, bit for bit
    e2 = primed(inputs, params, spun, 3)
    parts = [e2.run_diag(1, CO2_3x2[:, y:y + 1], dplan, records=records) for y in range(2)]
    for name in ("regions", "zonal", "annual", "yearly"):
        assert np.array_equal(bits(np.concatenate([getattr(p, name) for p in parts], axis=1)), bits(getattr(rd, name))), name
    same_engine_state(eb, e2, rd.yearly[:, 1:], parts[1].yearly, "diag 1 + 1")
    e2.close()
    e2 = primed(inputs, params, spun, 3)
    parts = [e2.run_ens(1, CO2_3x2[:, y:y + 1], splan, records=records) for y in range(2)]
    for name in ENS_NAMES + ("yearly",):  # (the year axis is 1 in all of them)
        assert np.array_equal(bits(np.concatenate([getattr(p, name) for p in parts], axis=1)), bits(getattr(rs, name))), name
    e2.close()
    e2 = primed(inputs, params, spun, 3)
    parts = [e2.run_lin(1, CO2_3x2[:, y:y + 1], lplan, records=records) for y in range(2)]
    assert np.array_equal(bits(np.concatenate([p.coef for p in parts], axis=1)), bits(rl.coef))
    assert np.array_equal(bits(np.concatenate([p.rss for p in parts], axis=0)), bits(rl.rss))
    same_engine_state(el, e2, rl.yearly[:, 1:], parts[1].yearly, "lin 1 + 1")
    e2.close()
    e1, e2 = primed(inputs, params, spun, 3), primed(inputs, params, spun, 3)  # clim: two periods of one year each
    whole = e1.run_clim(2, CO2_3x2, cplan, [(0, 1), (1, 1)], records=records)
    parts = [e2.run_clim(1, CO2_3x2[:, y:y + 1], cplan, [(0, 1)], records=records) for y in range(2)]
    for name in CLIM_NAMES + ("yearly",):
        got = np.concatenate([getattr(p, name) for p in parts], axis=1)
        assert np.array_equal(bits(got), bits(getattr(whole, name))), name
    same_engine_state(e1, e2, whole.yearly[:, 1:], parts[1].yearly, "clim 1 + 1")
    same_engine_state(e1, ec, whole.yearly, rc.yearly, "clim periods")
    for e in (eb, ec, es, el, e1, e2):
        e.close()
    for p in (dplan, cplan, splan, lplan):
        p.close()


def test_run_budget_ens_five_years_reuse_both_output_slots(inputs, params, spun):
    """One call of five years: the statistics of years 2, 3 and 4 are made in an output slot an earlier year's must have
    left first, and every year's budget records are made where the year before's were.  The CO2 differs every year and
    between the members.  Then run_budget and run on both engines: the reduced runs left nothing behind."""
    co2 = np.array([[340.0, 400.0, 480.0, 560.0, 680.0], [1020.0, 900.0, 800.0, 700.0, 600.0]], np.float32)
    plan = ens.Plan(inputs.nx, inputs.ny, 2, [0, 0], probs=[0.25, 1.0])
    ea, eb = primed(inputs, params, spun, 2), primed(inputs, params, spun, 2)
    _, bud, yr_a = ea.run_budget(5, co2, want_monthly=False)
    res = eb.run_ens(5, co2, plan, records=STD)
    x = budget.combine_reference(STD, bud)
    for y in range(5):
        same_bits(ens.Result(*[getattr(res, n)[:, y] for n in ENS_NAMES]), ens.reference(x[:, y], [0, 0], probs=[0.25, 1.0]),
                  ENS_NAMES, f"run_budget_ens year {y} of 5")
    assert not np.array_equal(x[:, 0], x[:, 2]) and not np.array_equal(x[:, 1], x[:, 3]), "the years differ"
    same_engine_state(ea, eb, yr_a, res.yearly, "after five years")
    mon_a, bud_a, yr_a = ea.run_budget(1, [[500.0], [900.0]])
    mon_b, bud_b, yr_b = eb.run_budget(1, [[500.0], [900.0]])
    assert np.array_equal(bits(bud_a), bits(bud_b)) and np.array_equal(bits(mon_a), bits(mon_b)) and np.array_equal(yr_a, yr_b)
    mon_a, yr_a = ea.run(1, 450.0)
    mon_b, yr_b = eb.run(1, 450.0)
    assert np.array_equal(bits(mon_a), bits(mon_b))
    same_engine_state(ea, eb, yr_a, yr_b, "after run_budget and run")
    ea.close(); eb.close(); plan.close()


def _diag_twins(ea, eb, nx, ny, label):
    """run_budget on ea, run_budget_diag on eb, one year of one member."""
    plan = diag.Plan(nx, ny, regions_for(nx, ny), n_vars=3)
    _, bud, yr_a = ea.run_budget(1, 680.0, want_monthly=False)
    res = eb.run_diag(1, 680.0, plan, records=STD)
    x = budget.combine_reference(STD, bud)
    diag_against_mirror(diag.Result(res.regions[:, 0], res.zonal[:, 0], res.annual[:, 0], None, res.names), x[:, 0], plan.weights, label)
    same_engine_state(ea, eb, yr_a, res.yearly, label)
    plan.close()


def test_run_budget_diag_any_grid_g96(inputs, params, spun):
    ea, eb = (primed(inputs, params, spun, 1, multilaunch=True) for _ in range(2))
    assert eb.describe()["engine"] == "latitude bands"
    _diag_twins(ea, eb, 96, 48, "latitude bands")
    ea.close(); eb.close()


def test_run_budget_diag_row_strips_g192x48():
    nx, ny = 192, 48
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 3, ipy=max(2, (3 * ny) // 4))
    ea, eb = engine.Engine(inp, p), engine.Engine(inp, p)
    assert eb.describe()["engine"] == "row strips"
    ea.flux_correction(1)
    eb.set_corrections(*ea.get_corrections(0))
    _diag_twins(ea, eb, nx, ny, "row strips")
    ea.close(); eb.close()


def test_plans_of_the_wrong_variable_count_are_refused(inputs, params, spun):
    e, twin = primed(inputs, params, spun, 1), primed(inputs, params, spun, 1)
    d5, d13 = diag.Plan(96, 48), diag.Plan(96, 48, n_vars=13)
    with pytest.raises(engine.GrebError) as ei:
        e.run_diag(1, 680.0, d5, records="budget")
    assert ei.value.code == -1 and "n_vars = 5" in str(ei.value) and "13 variables" in str(ei.value), str(ei.value)
    with pytest.raises(engine.GrebError) as ei:
        e.run_diag(1, 680.0, d13)
    assert ei.value.code == -1 and "n_vars = 13" in str(ei.value) and "5 variables" in str(ei.value), str(ei.value)
    with pytest.raises(engine.GrebError) as ei:
        e.run_diag(1, 680.0, d13, records=STD)
    assert ei.value.code == -1 and "n_vars = 13" in str(ei.value) and "3 variables" in str(ei.value), str(ei.value)
    assert e.describe()["budget_runs"] == 0
    mon_a, yr_a = e.run(1, 680.0)  # the refused calls left the engine alone
    mon_b, yr_b = twin.run(1, 680.0)
    assert np.array_equal(bits(mon_a), bits(mon_b))
    same_engine_state(e, twin, yr_a, yr_b, "after the refusals")
    e.close(); twin.close(); d5.close(); d13.close()


def test_tool_prints_one_json_line():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "run_fluxes.py"), "4", "1", "--compare"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    assert res["members"] == 4 and res["years"] == 1 and res["finite"] is True
    assert res["fluxes"] == ["surface_net", "atmos_net"]
    assert res["regions"] == ["globe", "land", "ocean", "glacier", "NH", "SH", "tropics", "Arctic", "Antarctic"]
    assert res["ensemble_years_per_s"][0] > 0 and res["bytes_from_device"] < res["bytes_of_full_budget"] / 1000
    c = res["compare"]
    dev = np.asarray(c["device"], np.float64)
    host, host_abs = np.asarray(c["host"], np.float64), np.asarray(c["host_abs"], np.float64)
    assert dev.shape == host.shape == host_abs.shape == (4, 1, 12, 2, 9) and c["points"] == 96 * 48
    assert np.array_equal(dev, dev.astype(np.float32).astype(np.float64))
    within_bound(dev.astype(np.float32), host, host_abs, c["points"], "tools/run_fluxes.py device against host")
