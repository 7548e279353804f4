"""GPU: per-member forcing (greb_engine_set_forcing_tables, greb_engine_set_member_forcing): regional and seasonal CO2,
insolation tables and scale, in the scenario phase.

1. Neutral forcing through the forcing-aware kernels equals the unforced engine, bit for bit.
2. Complementary patterns give bit-identical members, which differ from the globally forced one.
3. A forced run against tests/forcing_mirror.py (the oracle's routines stepped from Python, held to Oracle.run bit for bit
   in tests/test_forcing_cpu.py): monthly records, console values and four budget terms.
4. run, run_budget and run_diag are the same run under forcing; two one-year calls equal one two-year call.
5. Cases 1 and 2 on the latitude bands (96x48, multilaunch) and on the row strips (192x48).
6. A forced member with a switch beside an unforced member without: each equals its one-member engine.
7. Errors: every validation rule, a rejected call changes nothing, clearing returns to the default kernels, the
   flux-correction phase ignores forcing.
Every case is 96x48 unless named: one flux-correction year (or set_corrections from a shared spun-up state), one or two
scenario years, at most four members."""
import ctypes as C

import numpy as np
import pytest

import budget_mirror
import forcing_mirror
from conftest import rms, yearly_close
from test_gpu_budget import BOUNDS  # the bounds of the budget terms against the mirror: imported, not copied
from test_gpu_members import TOL    # RMS of a monthly-mean field: Tsurf, Tair, Tocean [K], q [kg/kg], albedo

pytestmark = pytest.mark.gpu

CO2 = 680.0
MODES = [False, True]  # strict
ids = lambda s: "strict" if s else "fast"


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


def states(e):
    return np.stack([e.state(m) for m in range(e.nm)])


def same(got, want, label):
    for name, a, b in zip(("monthly", "yearly", "state"), got, want):
        assert np.array_equal(a, b), (label, name, float(np.abs(np.asarray(a, np.float64) - b).max()))


# ------------------------------------------------------------------------------------------------ the engines and their yardsticks
KINDS = {"fused": (dict(), "fused member kernel"), "bands": (dict(multilaunch=True), "latitude bands"),
         "strips192": (dict(), "row strips")}
_inputs192 = {}
_unforced = {}


def kind_inputs(kind, inputs, params):
    if kind != "strips192":
        return inputs, params
    if not _inputs192:
        from greb_climate_model_amd import abi, workload
        _inputs192["x"] = (workload.make_inputs(192, 48), abi.default_params(ipx=189, ipy=36))
    return _inputs192["x"]


def unforced(eng_mod, inputs, params, kind, strict):
    """Computed once per engine kind and mode, shared, never changed: the corrections and state after one flux-correction
    year of a one-member engine, and its unforced scenario year at 680 ppm (monthly, yearly, state)."""
    k = (kind, strict)
    if k not in _unforced:
        inp, p = kind_inputs(kind, inputs, params)
        e = eng_mod.Engine(inp, p, strict=strict, **KINDS[kind][0])
        assert e.describe()["engine"] == KINDS[kind][1], e.describe()
        yf = e.flux_correction(1)
        corr, st = e.get_corrections(0)
        mon, yr = e.run(1, CO2)
        out = dict(corr=corr, state=st, flux_yearly=yf, run=(mon[0], yr[0], e.state(0)))
        e.close()
        for a in (corr, st, yf) + out["run"]:
            a.setflags(write=False)
        _unforced[k] = out
    return _unforced[k]


def forced_engine(eng_mod, inputs, params, kind, strict, n, start, space=None, season=None, solar=None, forcing=None):
    inp, p = kind_inputs(kind, inputs, params)
    e = eng_mod.Engine(inp, p, n_members=n, strict=strict, **KINDS[kind][0])
    e.set_corrections(start["corr"], start["state"])
    e.set_forcing_tables(space, season, solar)
    e.set_member_forcing(forcing)
    return e


def hemispheres(ny, nx):
    lat = (np.arange(ny) + 0.5) * 180.0 / ny - 90.0
    nh = np.broadcast_to((lat > 0)[:, None], (ny, nx)).astype(np.float32)
    return np.stack([nh, np.float32(1) - nh])


# ------------------------------------------------------------------------------------------------ the mirror (CPU, once)
@pytest.fixture(scope="module")
def mirror(oracle_lib, inputs, params):
    """Computed once, shared, never changed.  From the oracle's flux-correction year: two scenario years (340, then 680 ppm)
    under forcing_mirror.case3; one year at 680 ppm unforced and one with 680 ppm in the northern hemisphere only (ref 340)."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    f3 = forcing_mirror.case3(inputs)[3]
    y1 = forcing_mirror.run_year(o, start, 340.0, f3, inputs.sw_solar)
    y2 = forcing_mirror.run_year(o, forcing_mirror.next_start(start, y1[2]), 680.0, f3, inputs.sw_solar)
    plain = forcing_mirror.run_year(o, start, CO2, forcing_mirror.Forcing(), inputs.sw_solar)
    nh = forcing_mirror.run_year(o, start, CO2, forcing_mirror.Forcing(hemispheres(inputs.ny, inputs.nx)[0], None, 340.0), inputs.sw_solar)
    o.close()
    out = dict(start=dict(corr=start.corr, state=start.state5), monthly=np.stack([y1[0], y2[0]]), budget=np.stack([y1[1], y2[1]]),
               yearly=np.stack([y1[4], y2[4]]), state=y2[2],
               december_response=rms(nh[0][11, 0], plain[0][11, 0]))  # RMS over the grid of the December Tsurf difference
    for a in (out["monthly"], out["budget"], out["yearly"], out["state"], start.corr, start.state5):
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ 1. neutral forcing
def neutral_case(eng_mod, inputs, params, kind, strict):
    """Three members at 680 ppm: none; pattern 1 of 2 (all-ones space and season, co2_ref 123); solar table 1 of 2 (a copy of
    the engine's, scale 1).  All three run the forcing-aware kernels and equal the unforced one-member engine."""
    inp, _ = kind_inputs(kind, inputs, params)
    ref = unforced(eng_mod, inputs, params, kind, strict)
    ones = np.ones((2, inp.ny, inp.nx), np.float32)
    e = forced_engine(eng_mod, inputs, params, kind, strict, 3, ref, ones, np.ones((2, 730), np.float32), np.stack([inp.sw_solar] * 2),
                      [{}, {"co2_pattern": 1, "co2_ref": 123.0}, {"solar_table": 1, "solar_scale": 1.0}])
    d = e.describe()
    assert d["forcing"] == {"patterns": 2, "solar_tables": 2, "forced_members": 2} and d["correction_sets"] == 1, d
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    for m in range(3):
        same((mon[m], yr[m], st[m]), ref["run"], f"{kind} {ids(strict)} neutral member {m}")


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_neutral_forcing_equals_the_unforced_engine(eng_mod, params, inputs, strict):
    """If FAST differs here, the cause is in how the forcing-aware instantiation is contracted: to be fixed there."""
    neutral_case(eng_mod, inputs, params, "fused", strict)


# ------------------------------------------------------------------------------------------------ 2. complementary patterns
def complementary_case(eng_mod, inputs, params, kind, strict, bar):
    """A = (NH pattern, 680, ref 340), B = (SH pattern, 340, ref 680), G = 680 everywhere without forcing.  A and B are the
    same sum with swapped operands: bit-identical.  G differs from them by more than `bar` in December Tsurf (RMS)."""
    inp, _ = kind_inputs(kind, inputs, params)
    ref = unforced(eng_mod, inputs, params, kind, strict)
    e = forced_engine(eng_mod, inputs, params, kind, strict, 3, ref, hemispheres(inp.ny, inp.nx), None, None,
                      [{"co2_pattern": 0, "co2_ref": 340.0}, {"co2_pattern": 1, "co2_ref": 680.0}, {}])
    assert e.describe()["forcing"]["forced_members"] == 2
    mon, yr = e.run(1, np.asarray([[680.0], [340.0], [680.0]], np.float32))
    st = states(e)
    e.close()
    same((mon[0], yr[0], st[0]), (mon[1], yr[1], st[1]), f"{kind} {ids(strict)} complementary members")
    same((mon[2], yr[2], st[2]), ref["run"], f"{kind} {ids(strict)} unforced member beside them")
    d = rms(mon[0, 0, 11, 0], mon[2, 0, 11, 0])
    print(f"{kind} {ids(strict)}: December Tsurf, NH-only 680 ppm against global 680 ppm: RMS {d:.4f} K (bar {bar:.4f} K)")
    assert d > bar, (d, bar)
    sh, nh = mon[0, 0, 11, 0][: inp.ny // 2], mon[0, 0, 11, 0][inp.ny // 2:]
    g = mon[2, 0, 11, 0]
    assert rms(sh, g[: inp.ny // 2]) > rms(nh, g[inp.ny // 2:])  # the hemisphere kept at 340 ppm is the one that moved


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_complementary_patterns(eng_mod, params, inputs, mirror, strict):
    complementary_case(eng_mod, inputs, params, "fused", strict, 0.5 * mirror["december_response"])


# ------------------------------------------------------------------------------------------------ 3. against the mirror
_case3 = {}


def case3_engine(eng_mod, inputs, params, mirror, strict):
    space, season, solar, _ = forcing_mirror.case3(inputs)
    return forced_engine(eng_mod, inputs, params, "fused", strict, 1, mirror["start"], space, season, solar,
                         [{"co2_pattern": 0, "co2_ref": 298.0, "solar_table": 0, "solar_scale": 1.02}])


CO2_2Y = np.asarray([[340.0, 680.0]], np.float32)


def case3_budget_run(eng_mod, inputs, params, mirror, strict):
    """run_budget over the two years of case 3: (monthly, budget, yearly, state), computed once per mode."""
    if strict not in _case3:
        e = case3_engine(eng_mod, inputs, params, mirror, strict)
        mon, bud, yr = e.run_budget(2, CO2_2Y)
        _case3[strict] = (mon[0], bud[0], yr[0], e.state(0))
        e.close()
    return _case3[strict]


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_forced_run_against_the_mirror(eng_mod, params, inputs, mirror, strict):
    """Measured on an MI355X (profiles/forcing_parity_numbers.txt), the larger of the two years.
    Monthly records, RMS: STRICT Tsurf 1.9e-05, Tair 1.8e-05, Tocean 5.1e-06 K, q 2.5e-09, albedo 2.8e-07; FAST 1.7e-05,
    1.6e-05, 5.8e-06 K, 3.2e-09, 2.3e-07.  Budget terms, max |difference| in W/m2: STRICT sw 2.0e-03, LW_surf 2.6e-03,
    LWair_down 5.2e-04, LW_abs 2.1e-03; FAST 1.9e-03, 3.8e-03, 8.5e-04, 3.3e-03.  Console values: global mean within
    6.1e-05 (STRICT) and 2.7e-04 (FAST) of the mirror's, the point value within 3.1e-05."""
    from greb_climate_model_amd import abi
    mon, bud, yr, _ = case3_budget_run(eng_mod, inputs, params, mirror, strict)
    tag = ids(strict).upper()
    for y in range(2):
        for i, tol in enumerate(TOL):
            r = rms(mon[y, :, i], mirror["monthly"][y, :, i])
            print(f"forced vs mirror {tag} year {y} field {i}: RMS {r:.3e} (bar {tol:.0e})")
            assert r < tol, (y, i, r)
    print(f"forced vs mirror {tag} yearly: engine {yr.tolist()} mirror {mirror['yearly'].tolist()}")
    yearly_close(yr, mirror["yearly"], strict)
    for name in ("sw", "LW_surf", "LWair_down", "LW_abs"):
        t = abi.BUDGET_NAMES.index(name)
        d = float(np.abs(bud[:, :, t].astype(np.float64) - mirror["budget"][:, :, t]).max())
        print(f"forced vs mirror {tag} budget {name:>10s}: max |difference| {d:.3e} (bound {BOUNDS[name]:.0e})")
        assert d < BOUNDS[name], (name, d)
    # the forcing is in there: the mirror's unforced December differs by far more than the bars
    assert rms(mon[1, 11, 0], mirror["monthly"][1, 11, 0]) < 1e-4 < 0.1 * mirror["december_response"]


# ------------------------------------------------------------------------------------------------ 4. same run
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_run_run_budget_and_run_diag_are_the_same_run(eng_mod, params, inputs, mirror, strict):
    from greb_climate_model_amd import abi, diag
    mon_b, _, yr_b, st_b = case3_budget_run(eng_mod, inputs, params, mirror, strict)
    e = case3_engine(eng_mod, inputs, params, mirror, strict)
    mon, yr = e.run(2, CO2_2Y)
    st = e.state(0)
    e.close()
    same((mon[0], yr[0], st), (mon_b, yr_b, st_b), f"{ids(strict)} run against run_budget")
    e = case3_engine(eng_mod, inputs, params, mirror, strict)
    plan = diag.Plan(inputs.nx, inputs.ny)
    res = e.run_diag(2, CO2_2Y, plan, abi.D_ANNUAL)
    st_d = e.state(0)
    e.close(); plan.close()
    assert np.array_equal(res.yearly[0], yr[0]) and np.array_equal(st_d, st)
    ann = diag.reduce_reference(mon[0])[2]  # [2][5][ny][nx], fp64
    ulp = np.spacing(np.abs(ann).astype(np.float32)).astype(np.float64)
    err = np.abs(res.annual[0].astype(np.float64) - ann) / ulp
    print(f"{ids(strict)} run_diag annual maps under forcing: max |device - mirror of run's records| = {err.max():.3f} ulp")
    assert err.max() <= 1.0
    e = case3_engine(eng_mod, inputs, params, mirror, strict)
    m1, y1 = e.run(1, CO2_2Y[:, :1])
    m2, y2 = e.run(1, CO2_2Y[:, 1:])
    st_2 = e.state(0)
    e.close()
    same((np.concatenate([m1, m2], axis=1)[0], np.concatenate([y1, y2], axis=1)[0], st_2), (mon[0], yr[0], st),
         f"{ids(strict)} two one-year calls against one two-year call")


# ------------------------------------------------------------------------------------------------ 5. other engines
@pytest.mark.parametrize("kind,strict", [("bands", False), ("bands", True), ("strips192", False)],
                         ids=["bands-fast", "bands-strict", "strips192-fast"])
def test_neutral_forcing_other_engines(eng_mod, params, inputs, kind, strict):
    neutral_case(eng_mod, inputs, params, kind, strict)


@pytest.mark.parametrize("kind,strict", [("bands", False), ("bands", True), ("strips192", False)],
                         ids=["bands-fast", "bands-strict", "strips192-fast"])
def test_complementary_patterns_other_engines(eng_mod, params, inputs, mirror, kind, strict):
    """(192x48 is the same workload refined in longitude: the 96x48 mirror's response is its bar too.)"""
    complementary_case(eng_mod, inputs, params, kind, strict, 0.5 * mirror["december_response"])


# ------------------------------------------------------------------------------------------------ 6. mixed with switches
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_forced_member_with_a_switch_beside_a_plain_member(eng_mod, params, inputs, strict):
    from greb_climate_model_amd import abi
    nh = hemispheres(inputs.ny, inputs.nx)[:1]
    forced = {"co2_pattern": 0, "co2_ref": 340.0, "solar_scale": 1.02}

    def one(e):
        yf = e.flux_correction(1)
        mon, yr = e.run(1, CO2)
        out = [(mon[m], yr[m], e.state(m), yf[m]) for m in range(e.nm)]
        e.close()
        return out

    e = eng_mod.Engine(inputs, params, members=[{"switches": abi.X_NO_HYDRO}, {}], strict=strict)
    e.set_forcing_tables(nh)
    e.set_member_forcing([forced, {}])
    d = e.describe()
    assert d["forcing"]["forced_members"] == 1 and d["member_switches"] == "per member" and d["correction_sets"] == 2, d
    both = one(e)
    a = eng_mod.Engine(inputs, params, strict=strict)
    a.set_experiment(abi.X_NO_HYDRO)
    a.set_forcing_tables(nh)
    a.set_member_forcing([forced])
    alone = one(a)[0]
    plain = unforced(eng_mod, inputs, params, "fused", strict)
    same(both[0][:3], alone[:3], f"{ids(strict)} forced NO_HYDRO member")
    assert np.array_equal(both[0][3], alone[3])
    same(both[1][:3], plain["run"], f"{ids(strict)} plain member beside it")
    assert np.array_equal(both[1][3], plain["flux_yearly"][0])
    assert rms(both[0][0][0, 11, 0], both[1][0][0, 11, 0]) > 1e-2  # (December Tsurf: the two members are different runs)


# ------------------------------------------------------------------------------------------------ 7. errors
def _rejected(eng_mod, e, rc, *words):
    assert rc == -1, rc
    msg = eng_mod.lib().greb_engine_last_error(e.h).decode()
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_errors_leave_the_engine_as_it_was(eng_mod, params, inputs, strict):
    from greb_climate_model_amd import abi
    L = eng_mod.lib()
    ny, nx = inputs.ny, inputs.nx
    ref = unforced(eng_mod, inputs, params, "fused", strict)
    hemi = hemispheres(ny, nx)
    solar = np.ascontiguousarray(np.stack([inputs.sw_solar] * 2), np.float32)
    good = [{"co2_pattern": 1, "co2_ref": 340.0, "solar_table": 1, "solar_scale": 1.01}]

    def engine():
        return forced_engine(eng_mod, inputs, params, "fused", strict, 1, ref, hemi, None, solar, good)

    e = engine()
    tables = lambda n_p, sp, se, n_s, so: L.greb_engine_set_forcing_tables(e.h, n_p, None if sp is None else abi.fptr(sp),
                                                                            None if se is None else abi.fptr(se), n_s,
                                                                            None if so is None else abi.fptr(so))

    def member(**kw):
        f = (abi.GrebMemberForcing * 1)()
        f[0].co2_pattern, f[0].co2_ref, f[0].solar_table, f[0].solar_scale = -1, 340.0, -1, 1.0
        for k, v in kw.items():
            setattr(f[0], k, v)
        return L.greb_engine_set_member_forcing(e.h, f)

    big = np.ones((17, ny, nx), np.float32)
    _rejected(eng_mod, e, tables(17, big, None, 0, None), "n_patterns", "17")
    _rejected(eng_mod, e, tables(-1, None, None, 0, None), "n_patterns", "-1")
    _rejected(eng_mod, e, tables(0, None, None, 17, solar), "n_solar", "17")
    for bad, word in ((np.nan, "nan"), (1.5, "1.5"), (-0.25, "-0.25"), (np.inf, "inf")):
        w = hemi.copy(); w[1, 7, 5] = bad
        _rejected(eng_mod, e, tables(2, w, None, 0, None), "co2_space", "pattern 1", "row 7", "column 5", word)
        s = np.ones((2, 730), np.float32); s[0, 364] = bad
        _rejected(eng_mod, e, tables(2, hemi, s, 0, None), "co2_season", "pattern 0", "step 365", word)
    for bad, word in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        t = solar.copy(); t[1, 729, 3] = bad
        _rejected(eng_mod, e, tables(0, None, None, 2, t), "sw_solar", "table 1", "step 730", "row 3", word)
    _rejected(eng_mod, e, tables(1, hemi[:1], None, 2, solar), "member 0", "co2_pattern 1")   # fewer tables than a member names
    _rejected(eng_mod, e, tables(2, hemi, None, 1, solar[:1]), "member 0", "solar_table 1")
    _rejected(eng_mod, e, member(co2_pattern=2), "member 0", "co2_pattern 2")
    _rejected(eng_mod, e, member(co2_pattern=-2), "member 0", "co2_pattern -2")
    _rejected(eng_mod, e, member(solar_table=2), "member 0", "solar_table 2")
    for bad, word in ((0.0, "co2_ref 0"), (-5.0, "co2_ref -5"), (np.nan, "co2_ref nan"), (np.inf, "co2_ref inf")):
        _rejected(eng_mod, e, member(co2_pattern=0, co2_ref=bad), "member 0", word)
    for bad, word in ((-0.5, "solar_scale -0.5"), (np.nan, "solar_scale nan"), (np.inf, "solar_scale inf")):
        _rejected(eng_mod, e, member(solar_scale=bad), "member 0", word)
    with pytest.raises(eng_mod.GrebError):
        e.set_member_forcing([{"co2_pattern": 0, "scale": 1.0}])
    assert e.describe()["forcing"] == {"patterns": 2, "solar_tables": 2, "forced_members": 1}
    got = e.run(1, CO2) + (e.state(0),)
    # ... equals the run of an engine that never made the rejected calls
    f = engine()
    want = f.run(1, CO2) + (f.state(0),)
    f.close()
    same(got, want, f"{ids(strict)} after the rejected calls")
    assert not np.array_equal(got[0][0], ref["run"][0])  # (and that run was forced)
    # clearing returns to the default kernels; tables may then shrink, and the indices are validated against the new ones
    e.set_member_forcing(None)
    assert e.describe()["forcing"] == {"patterns": 2, "solar_tables": 2, "forced_members": 0}
    e.set_forcing_tables(hemi[:1])
    assert e.describe()["forcing"] == {"patterns": 1, "solar_tables": 0, "forced_members": 0}
    _rejected(eng_mod, e, member(co2_pattern=1), "member 0", "co2_pattern 1")
    _rejected(eng_mod, e, member(solar_table=0), "member 0", "solar_table 0")
    e.set_corrections(ref["corr"], ref["state"])
    mon, yr = e.run(1, CO2)  # the second scenario year of this engine's clock: the year's records are those of a first year
    same((mon[0], yr[0], e.state(0)), ref["run"], f"{ids(strict)} cleared forcing")
    e.close()


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_flux_correction_ignores_forcing(eng_mod, params, inputs, strict):
    ref = unforced(eng_mod, inputs, params, "fused", strict)
    space, season, solar, _ = forcing_mirror.case3(inputs)
    e = eng_mod.Engine(inputs, params, n_members=2, strict=strict)
    e.set_forcing_tables(space, season, solar)
    e.set_member_forcing([{"co2_pattern": 0, "co2_ref": 298.0, "solar_table": 0, "solar_scale": 1.02}, {"solar_scale": 0.9}])
    assert e.describe()["forcing"]["forced_members"] == 2 and e.describe()["correction_sets"] == 1
    yf = e.flux_correction(1)
    for m in range(2):
        corr, st = e.get_corrections(m)
        assert np.array_equal(corr, ref["corr"]) and np.array_equal(st, ref["state"]) and np.array_equal(yf[m], ref["flux_yearly"][0]), m
    e.close()
