"""GPU: the budget output (greb_engine_run_budget): monthly means of the thirteen flux terms of the update.

1. run_budget leaves what run leaves: monthly, yearly and every member's state, bit for bit (fused, any-grid, row strips).
2. The thirteen fields against tests/budget_mirror.py (the oracle's routines stepped from Python, itself held to
   Oracle.run bit for bit in tests/test_budget_cpu.py), from the same spun-up state and corrections, one scenario year.
3. Closure of the atmosphere's and the deep ocean's budget from delivered numbers alone.
4. A member's switches zero the terms of the processes they switch off; a member equals its one-member engine.
5. Call patterns: split calls, run / run_budget alternating, budget-only, device-out.
6. Errors.
Every case: 1 flux-correction year + 1 or 2 scenario years on the synthetic workload (5 where staging slots are to be reused)."""
import numpy as np
import pytest

import budget_mirror

pytestmark = pytest.mark.gpu

CO2 = 680.0

# Test 2: largest |engine - mirror| allowed per term over the 12 months of one scenario year at 96x48.  Each bound is four
# times the largest FAST difference measured on an MI355X (tools/run_budget.py --compare, profiles/budget_parity_numbers.txt),
# rounded up to one significant digit: the factor allows for box-to-box differences in OCML code paths and for the
# trajectory divergence of a longer run.  No W/m2 bound may exceed 1.1e-2 W/m2 -- the flux that moves the thinnest column
# (land, 4.8e6 J/m2K) by the field tolerance of 1e-4 K in one 43 200 s step.
W_M2_CAP = 1.1e-2
MEASURED = {  # name: (STRICT, FAST) largest |engine - mirror| on an MI355X (profiles/budget_parity_numbers.txt)
    "sw": (1.221e-03, 1.221e-03), "LW_surf": (1.282e-03, 2.258e-03), "LWair_down": (2.518e-04, 3.891e-04),
    "LW_abs": (1.022e-03, 1.801e-03), "Q_sens": (4.646e-03, 9.220e-03), "Q_lat": (1.274e-03, 2.018e-03),
    "Q_lat_air": (1.602e-04, 1.678e-04), "dq_eva": (2.114e-13, 3.337e-13), "dq_rain": (2.842e-14, 2.842e-14),
    "dT_ocean": (1.010e-07, 1.006e-07), "dTo": (2.282e-08, 2.619e-08), "dTa_crcl": (3.594e-05, 7.629e-05),
    "dq_crcl": (8.052e-09, 1.338e-08)}
# Q_sens: four times its FAST maximum would be 4e-2 W/m2, above the cap, so its bound IS the cap and the measured 9.2e-3
# sits 16 % under it.  The finding behind it: Q_sens = ct_sens (Tair - Tsurf) multiplies a temperature difference by
# 22.5 W/m2K: 9.2e-3 W/m2 is a monthly-mean Tair - Tsurf that differs by 4e-4 K at the worst point after a year of two
# trajectories.  That is a pointwise maximum of the size DESIGN.md section 5 records for the five standard records
# themselves (up to 6.7e-4 K), while the cap was derived from their RMS tolerance of 1e-4 K.
BOUNDS = {"sw": 5e-3, "LW_surf": 1e-2, "LWair_down": 2e-3, "LW_abs": 8e-3, "Q_sens": W_M2_CAP, "Q_lat": 9e-3,
          "Q_lat_air": 7e-4, "dq_eva": 2e-12, "dq_rain": 2e-13, "dT_ocean": 5e-7, "dTo": 2e-7, "dTa_crcl": 4e-4,
          "dq_crcl": 6e-8}


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


def states(e):
    return np.stack([e.state(m) for m in range(e.nm)])


# ------------------------------------------------------------------------------------------------ 1. same run
def _same_run(eng_mod, inp, p, co2, engine_name, **kw):
    out = []
    for budget in (True, False):
        e = eng_mod.Engine(inp, p, n_members=len(co2), **kw)
        assert e.describe()["engine"] == engine_name, e.describe()
        yf = e.flux_correction(1)
        if budget:
            mon, bud, yr = e.run_budget(1, np.asarray(co2, np.float32)[:, None])
            assert e.describe()["budget_runs"] == 1
            assert bud.shape == (len(co2), 1, 12, 13, inp.ny, inp.nx) and np.isfinite(bud).all()
            assert np.abs(bud).reshape(len(co2), 12, 13, -1).max(axis=-1).min() > 0, "a term is zero everywhere"
            assert not np.array_equal(bud[0], bud[1])  # (the members differ in CO2)
        else:
            mon, yr = e.run(1, np.asarray(co2, np.float32)[:, None])
            assert e.describe()["budget_runs"] == 0
        out.append((mon, yr, yf, states(e)))
        e.close()
    for name, a, b in zip(("monthly", "yearly", "flux yearly", "state"), *out):
        assert np.array_equal(a, b), (name, float(np.abs(a.astype(np.float64) - b).max()))


@pytest.mark.parametrize("strict", [False, True])
def test_run_budget_is_the_same_run_fused(eng_mod, params, inputs, strict):
    _same_run(eng_mod, inputs, params, [340.0, CO2], "fused member kernel", strict=strict)


@pytest.mark.parametrize("strict", [False, True])
def test_run_budget_is_the_same_run_any_grid_g96(eng_mod, params, inputs, strict):
    _same_run(eng_mod, inputs, params, [340.0, CO2], "latitude bands", strict=strict, multilaunch=True)


def test_run_budget_is_the_same_run_row_strips_g192x48(eng_mod):
    from greb_climate_model_amd import abi, workload
    nx, ny = 192, 48
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 3, ipy=max(2, (3 * ny) // 4))
    _same_run(eng_mod, inp, p, [340.0, CO2], "row strips")


# ------------------------------------------------------------------------------------------------ 2. against the mirror
@pytest.fixture(scope="module")
def mirror(oracle_lib, inputs, params):
    """Computed once, shared, never changed: the start (the oracle's flux-correction year) and the mirror's year."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    monthly, budget, state = budget_mirror.run_year(o, start, CO2)
    o.close()
    for a in (monthly, budget, state, start.corr, start.state5):
        a.setflags(write=False)
    return start, monthly, budget, state


@pytest.mark.parametrize("strict", [True, False])
def test_budget_against_the_mirror(eng_mod, params, inputs, mirror, strict):
    from greb_climate_model_amd import abi
    start, _, want, _ = mirror
    e = eng_mod.Engine(inputs, params, strict=strict)
    e.set_corrections(start.corr, start.state5)
    _, bud, _ = e.run_budget(1, CO2)
    e.close()
    d = np.abs(bud[0, 0].astype(np.float64) - want).reshape(12, abi.NBUDGET, -1).max(axis=(0, 2))
    scale = np.abs(want).reshape(12, abi.NBUDGET, -1).max(axis=(0, 2))
    for i, name in enumerate(abi.BUDGET_NAMES):
        print(f"budget vs mirror {'STRICT' if strict else 'FAST'} {name:>10s}: max |difference| {d[i]:.3e}  (largest |value| {scale[i]:.3e})  bound {BOUNDS[name]:.0e}")
    for i, name in enumerate(abi.BUDGET_NAMES):
        if i <= abi.B_Q_LAT_AIR:
            assert BOUNDS[name] <= W_M2_CAP, name
        assert d[i] < BOUNDS[name], (name, d[i], BOUNDS[name])


# ------------------------------------------------------------------------------------------------ 3. closure
@pytest.mark.parametrize("strict", [False, True])
def test_atmosphere_and_ocean_close_their_budget(eng_mod, params, inputs, strict):
    """From delivered numbers only, fp64 on the host, per member and point, over one scenario year:
      Ta_end - Ta_start = sum_m n_m [dTa_crcl + dt / cap_air (2 LWair_down - LW_abs + Q_lat_air - Q_sens)]_m
      To_end - To_start = sum_m n_m [dTo]_m + sum_t ToF[t]
    Bound 0.1 K: 730 steps x ulp(320 K) = 3.05e-5 K x three roundings per step (update, step sum, monthly division)
    = 0.07 K; a missing, doubled or wrongly signed 1 W/m2 term shows as 730 x 43 200 / cap_air = 5 K."""
    from greb_climate_model_amd import abi
    co2 = [340.0, CO2]
    e = eng_mod.Engine(inputs, params, n_members=2, strict=strict)
    e.flux_correction(1)
    before = states(e).astype(np.float64)
    _, bud, _ = e.run_budget(1, np.asarray(co2, np.float32)[:, None])
    after = states(e).astype(np.float64)
    corr = [e.get_corrections(m)[0].astype(np.float64) for m in range(2)]
    e.close()
    n = 2.0 * np.asarray(abi.JDAY_MON, np.float64)[:, None, None]
    cap_air = float(params.cp_air) * float(params.rho_air) * float(params.d_air)
    k = float(params.dt) / cap_air
    for m in range(2):
        b = bud[m, 0].astype(np.float64)  # [12][13][ny][nx]
        heat = 2.0 * b[:, abi.B_LWAIR_DOWN] - b[:, abi.B_LW_ABS] + b[:, abi.B_Q_LAT_AIR] - b[:, abi.B_Q_SENS]
        dTa = (n * (b[:, abi.B_DTA_CRCL] + k * heat)).sum(axis=0)
        dTo = (n * b[:, abi.B_DTO]).sum(axis=0) + corr[m][2].sum(axis=0)
        ra = np.abs(after[m, 1] - before[m, 1] - dTa).max()
        ro = np.abs(after[m, 2] - before[m, 2] - dTo).max()
        print(f"closure {'STRICT' if strict else 'FAST'} member {m}: atmosphere {ra:.3e} K, deep ocean {ro:.3e} K "
              f"(largest change {np.abs(after[m, 1] - before[m, 1]).max():.2f} / {np.abs(after[m, 2] - before[m, 2]).max():.2f} K)")
        assert ra < 0.1 and ro < 0.1, (m, ra, ro)


# ------------------------------------------------------------------------------------------------ 4. switches
SWITCHES = ("0", "NO_HYDRO | NO_DEEP_OCEAN", "NO_CIRCULATION")
_mixed = {}


def switch_words():
    from greb_climate_model_amd import abi
    return [0, abi.X_NO_HYDRO | abi.X_NO_DEEP_OCEAN, abi.X_NO_CIRCULATION]


def mixed_engine(eng_mod, inputs, params, strict):
    """Three members with different switches in one engine, 1 + 1 year: (monthly, budget), computed once per mode."""
    if strict not in _mixed:
        e = eng_mod.Engine(inputs, params, members=[{"switches": s} for s in switch_words()], strict=strict)
        e.flux_correction(1)
        mon, bud, _ = e.run_budget(1, CO2)
        e.close()
        _mixed[strict] = (mon, bud)
    return _mixed[strict]


@pytest.mark.parametrize("strict", [False, True])
def test_switched_off_processes_deliver_exact_zeros(eng_mod, params, inputs, strict):
    from greb_climate_model_amd import abi
    off = {1: (abi.B_Q_LAT, abi.B_Q_LAT_AIR, abi.B_DQ_EVA, abi.B_DQ_RAIN, abi.B_DT_OCEAN, abi.B_DTO),
           2: (abi.B_DTA_CRCL, abi.B_DQ_CRCL)}
    _, bud = mixed_engine(eng_mod, inputs, params, strict)
    for m in range(3):
        for t in range(abi.NBUDGET):
            zero = not bud[m, 0, :, t].any()
            assert zero == (t in off.get(m, ())), (SWITCHES[m], abi.BUDGET_NAMES[t], "zero" if zero else "not zero")


@pytest.mark.parametrize("m", [0, 1, 2], ids=["no_switches", "no_hydro_no_deep_ocean", "no_circulation"])
@pytest.mark.parametrize("strict", [False, True])
def test_member_budget_equals_its_one_member_engine(eng_mod, params, inputs, strict, m):
    """Each member of the mixed engine against the homogeneous one-member engine with its switches, np.array_equal.

    The member without switches runs the switch-aware instantiation of the kernels in the mixed engine and the default
    one in its own engine.  In FAST arithmetic the two once differed in the last bits (budget terms by up to 6.7e-4 W/m2,
    the five standard records by up to 9.2e-5): the vapour-diffusion-only switch was a run-time select inside the
    transport update and changed how the compiler fused the multiply-adds around it.  The switch-aware FAST kernels now
    take a copy of the sub-step loop in which that switch is the constant false (greb_member.hip: Circ::substeps), so a
    member without it is transported by the code the default instantiation has."""
    from greb_climate_model_amd import abi
    mon, bud = mixed_engine(eng_mod, inputs, params, strict)
    one = eng_mod.Engine(inputs, params, strict=strict)
    one.set_experiment(switch_words()[m])
    one.flux_correction(1)
    mon1, b1, _ = one.run_budget(1, CO2)
    one.close()
    d = np.abs(bud[m, 0].astype(np.float64) - b1[0, 0]).reshape(12, abi.NBUDGET, -1).max(axis=(0, 2))
    print(f"{'STRICT' if strict else 'FAST'} member {SWITCHES[m]}: monthly records "
          f"{'equal' if np.array_equal(mon[m], mon1[0]) else 'DIFFER by up to %.3e' % np.abs(mon[m].astype(np.float64) - mon1[0]).max()}; "
          "budget max |difference| per term: " + ", ".join(f"{n} {x:.2e}" for n, x in zip(abi.BUDGET_NAMES, d)))
    assert np.array_equal(bud[m], b1[0]), (SWITCHES[m], float(d.max()))


# ------------------------------------------------------------------------------------------------ 5. call pattern
@pytest.fixture(scope="module")
def spun_up(eng_mod, params, inputs):
    """Corrections and state after one flux-correction year (FAST, fused), for engines that only differ in how they are called."""
    e = eng_mod.Engine(inputs, params)
    e.flux_correction(1)
    corr, st = e.get_corrections(0)
    e.close()
    return corr, st


def _engine(eng_mod, inputs, params, spun_up, n=2):
    e = eng_mod.Engine(inputs, params, n_members=n)
    e.set_corrections(*spun_up)
    return e


LEVELS = np.asarray([[340.0], [CO2]], np.float32)


def test_split_calls_equal_one_call(eng_mod, params, inputs, spun_up):
    a = _engine(eng_mod, inputs, params, spun_up)
    m1, b1, y1 = a.run_budget(1, LEVELS)
    m2, b2, y2 = a.run_budget(1, LEVELS)
    sa = states(a)
    a.close()
    b = _engine(eng_mod, inputs, params, spun_up)
    m, bud, y = b.run_budget(2, np.repeat(LEVELS, 2, axis=1))
    sb = states(b)
    b.close()
    assert np.array_equal(np.concatenate([b1, b2], axis=1), bud)
    assert np.array_equal(np.concatenate([m1, m2], axis=1), m) and np.array_equal(np.concatenate([y1, y2], axis=1), y)
    assert np.array_equal(sa, sb)
    assert not np.array_equal(bud[:, 0], bud[:, 1])


def test_run_and_run_budget_alternate(eng_mod, params, inputs, spun_up):
    a = _engine(eng_mod, inputs, params, spun_up)
    a.run_budget(1, LEVELS); a.run(1, LEVELS)
    _, b3, _ = a.run_budget(1, LEVELS)
    a.close()
    b = _engine(eng_mod, inputs, params, spun_up)
    b.run(2, np.repeat(LEVELS, 2, axis=1))
    _, want, _ = b.run_budget(1, LEVELS)
    b.close()
    assert np.array_equal(b3, want)


def test_budget_only_and_device_out_equal_the_host_form(eng_mod, params, inputs, spun_up):
    import torch
    Y = 2
    co2 = np.repeat(LEVELS, Y, axis=1)
    a = _engine(eng_mod, inputs, params, spun_up)
    mon, bud, yr = a.run_budget(Y, co2)
    a.close()
    b = _engine(eng_mod, inputs, params, spun_up)
    none, only, yr_b = b.run_budget(Y, co2, want_monthly=False)
    b.close()
    assert none is None and np.array_equal(only, bud) and np.array_equal(yr_b, yr)
    for with_monthly in (True, False):
        c = _engine(eng_mod, inputs, params, spun_up)
        dbud = torch.full(bud.shape, float("nan"), dtype=torch.float32, device="cuda")
        dmon = torch.full(mon.shape, float("nan"), dtype=torch.float32, device="cuda") if with_monthly else None
        _, _, yr_c = c.run_budget(Y, co2, budget_dev_ptr=dbud.data_ptr(), monthly_dev_ptr=dmon.data_ptr() if with_monthly else None)
        torch.cuda.synchronize()
        c.close()
        assert np.array_equal(dbud.cpu().numpy(), bud) and np.array_equal(yr_c, yr), with_monthly
        if with_monthly:
            assert np.array_equal(dmon.cpu().numpy(), mon)


def _one_member(eng_mod, inputs, params):
    e = eng_mod.Engine(inputs, params)
    e.flux_correction(1)
    return e


RAMP = np.asarray([[340.0, 400.0, 480.0, 560.0, CO2]], np.float32)  # five years: every staging slot is written again, in both parities


def test_five_budget_years_host_device_out_and_run(eng_mod, params, inputs):
    """One member, five years whose CO2 differs: the host-delivered records (each year leaves from a staging slot that
    year y + 2 writes again) are the ones the kernels write straight into device arrays, and run()'s."""
    import torch
    a = _one_member(eng_mod, inputs, params)
    mon, bud, yr = a.run_budget(5, RAMP)
    sa = states(a)
    a.close()
    assert not any(np.array_equal(bud[:, y], bud[:, y + 1]) for y in range(4))
    c = _one_member(eng_mod, inputs, params)
    dbud = torch.full(bud.shape, float("nan"), dtype=torch.float32, device="cuda")
    dmon = torch.full(mon.shape, float("nan"), dtype=torch.float32, device="cuda")
    _, _, yr_c = c.run_budget(5, RAMP, budget_dev_ptr=dbud.data_ptr(), monthly_dev_ptr=dmon.data_ptr())
    torch.cuda.synchronize()
    sc = states(c)
    c.close()
    assert np.array_equal(dbud.cpu().numpy(), bud) and np.array_equal(dmon.cpu().numpy(), mon)
    assert np.array_equal(yr_c, yr) and np.array_equal(sc, sa)
    d = _one_member(eng_mod, inputs, params)
    mon_d, yr_d = d.run(5, RAMP)
    sd = states(d)
    d.close()
    assert np.array_equal(mon_d, mon) and np.array_equal(yr_d, yr) and np.array_equal(sd, sa)
    b = _one_member(eng_mod, inputs, params)
    none, only, yr_b = b.run_budget(5, RAMP, want_monthly=False)
    b.close()
    assert none is None and np.array_equal(only, bud) and np.array_equal(yr_b, yr)


def test_five_run_years_pinned_pageable_and_device_out(eng_mod, params, inputs):
    """run() of one member over the same five years: delivered into a pinned buffer (true DMA), into a pageable one (staged
    by the runtime) and written by the kernels into a device array -- identical records, yearly values and state."""
    import torch
    shape = (1, 5, 12, 5, inputs.ny, inputs.nx)
    pinned = torch.full(shape, float("nan"), dtype=torch.float32).pin_memory()
    assert pinned.is_pinned()
    pageable = np.full(shape, np.nan, np.float32)
    dev = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    got = []
    for kw in ({"out": pinned.numpy()}, {"out": pageable}, {"monthly_dev_ptr": dev.data_ptr()}):
        e = _one_member(eng_mod, inputs, params)
        _, yr = e.run(5, RAMP, **kw)
        torch.cuda.synchronize()
        got.append((yr, states(e)))
        e.close()
    assert np.isfinite(pageable).all() and not any(np.array_equal(pageable[:, y], pageable[:, y + 1]) for y in range(4))
    assert np.array_equal(pinned.numpy(), pageable) and np.array_equal(dev.cpu().numpy(), pageable)
    for yr, st in got[1:]:
        assert np.array_equal(yr, got[0][0]) and np.array_equal(st, got[0][1])


# ------------------------------------------------------------------------------------------------ 6. errors
def test_null_budget_is_invalid_and_the_engine_runs_on(eng_mod, params, inputs, spun_up):
    from greb_climate_model_amd import abi
    e = _engine(eng_mod, inputs, params, spun_up, n=1)
    co2 = np.full((1, 1), CO2, np.float32)
    mon = np.empty((1, 1, 12, 5, inputs.ny, inputs.nx), np.float32)
    rc = eng_mod.lib().greb_engine_run_budget(e.h, 1, abi.fptr(co2), abi.fptr(mon), None, None, 0)
    assert rc == -1
    assert "budget" in eng_mod.lib().greb_engine_last_error(e.h).decode()
    with pytest.raises(eng_mod.GrebError) as ei:
        eng_mod._check(eng_mod.lib().greb_engine_run_budget(e.h, 0, abi.fptr(co2), None, abi.fptr(mon), None, 0), e.h)
    assert ei.value.code == -1
    _, bud, _ = e.run_budget(1, CO2)  # the clock did not move: this is the first scenario year
    e.close()
    f = _engine(eng_mod, inputs, params, spun_up, n=1)
    _, want, _ = f.run_budget(1, CO2)
    f.close()
    assert np.array_equal(bud, want)


def test_run_budget_before_any_flux_correction_behaves_as_run(eng_mod, params, inputs):
    a = eng_mod.Engine(inputs, params)
    mon_a, bud, yr_a = a.run_budget(1, CO2)
    sa = a.state(0)
    a.close()
    b = eng_mod.Engine(inputs, params)
    mon_b, yr_b = b.run(1, CO2)
    sb = b.state(0)
    b.close()
    assert np.array_equal(mon_a, mon_b) and np.array_equal(yr_a, yr_b) and np.array_equal(sa, sb)
    assert np.isfinite(bud).all()
