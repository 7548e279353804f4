"""GPU: prescribed SST per member (greb_engine_set_sst_tables, greb_engine_set_member_sst): anomaly patterns, nudging weights
and seasons, in the scenario phase.

1. A member with an all-ones anomaly and amp 1 equals a member with GREB_X_SST_PLUS1 in the same engine, bit for bit.
2. Weight 0 at amp 123 through the forcing-aware kernels equals the unforced one-member engine, bit for bit.
3. A patch, a basin weight with a buffer and a season that changes sign, at 680 ppm, against tests/sst_mirror.py (held to
   Oracle.run under the switch bit for bit in tests/test_sst_cpu.py): monthly records and console values.
4. Locality of the hook: what it leaves alone follows the mirror; the response over the patch against the far hemisphere.
5. run, run_budget and run_diag are the same run; a prescribed member on a boundary set is held to that set's tclim.
6. A prescribed member beside a plain member: each equals its one-member engine.
7. Errors: every validation rule, a rejected call changes nothing, clearing returns to the default kernels, the
   flux-correction phase ignores all of it, the "forcing" object of describe() is untouched.
Cases 1 and 2 also on the latitude bands (96x48, multilaunch) and on the row strips (192x48).  Every case: one
flux-correction year (or set_corrections from a shared spun-up state), one scenario year, at most four members."""
import dataclasses
import os

import numpy as np
import pytest

import budget_mirror
import sst_mirror
from conftest import rms, yearly_close
from test_gpu_members import TOL  # RMS of a monthly-mean field: Tsurf, Tair, Tocean [K], q [kg/kg], albedo -- imported, not copied

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CO2 = 680.0
MODES = [False, True]  # strict
ids = lambda s: "strict" if s else "fast"
ALL_KINDS = [("fused", False), ("fused", True), ("bands", False), ("bands", True), ("strips192", False)]
KIND_IDS = ["fused-fast", "fused-strict", "bands-fast", "bands-strict", "strips192-fast"]
BASIN = (-20.0, 20.0, 150.0, 260.0)  # the tropical Pacific of cases 3 and 4


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
    year of a one-member engine, and its plain scenario year at 680 ppm (monthly, yearly, state)."""
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


def sst_engine(eng_mod, inputs, params, kind, strict, n, start, anom, weight=None, season=None, sst=None, **kw):
    inp, p = kind_inputs(kind, inputs, params)
    e = eng_mod.Engine(inp, p, n_members=n, strict=strict, **KINDS[kind][0], **kw)
    e.set_corrections(start["corr"], start["state"])
    e.set_sst_tables(anom, weight, season)
    e.set_member_sst(sst)
    return e


# ------------------------------------------------------------------------------------------------ the mirror (CPU, once)
def far_side(inp, lat0, lon0):
    """[ny][nx] bool: the hemisphere facing away from (lat0, lon0) -- more than 90 degrees of great circle from it."""
    from greb_climate_model_amd import forcing
    lat = np.deg2rad((np.arange(inp.ny) + 0.5) * 180.0 / inp.ny - 90.0)[:, None]
    lon = np.deg2rad(forcing.longitudes(inp.nx))[None, :]
    c = np.sin(lat) * np.sin(np.deg2rad(lat0)) + np.cos(lat) * np.cos(np.deg2rad(lat0)) * np.cos(lon - np.deg2rad(lon0))
    return c < 0


def response_ratio(december_member, december_control, patch, far):
    """RMS over the patch of the December Tsurf difference to the control, over its RMS over the far hemisphere."""
    d = np.asarray(december_member, np.float64) - december_control
    return float(np.sqrt((d[patch] ** 2).mean()) / np.sqrt((d[far] ** 2).mean()))


@pytest.fixture(scope="module")
def mirror(oracle_lib, inputs, params):
    """Computed once, shared, never changed.  From the oracle's flux-correction year, one scenario year each at 680 ppm:
    case 3 (sst_mirror.case3); case 4 -- case 3's patch at amp 2 with weight 1 on the basin only, its control at amp 0, and
    the year without any hook; and case 5 -- case 3 on a boundary set with its own tclim, from that set's own spin-up."""
    from greb_climate_model_amd import forcing
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    args = (inputs.tclim, inputs.z_topo, inputs.sw_solar)
    anom, weight, season, s3 = sst_mirror.case3(inputs)
    c3 = sst_mirror.run_year(o, start, CO2, s3, *args)
    basin = forcing.basin_weight(inputs, BASIN, 0.0)
    member = sst_mirror.run_year(o, start, CO2, sst_mirror.Sst(anom, basin, None, 2.0), *args)
    control = sst_mirror.run_year(o, start, CO2, sst_mirror.Sst(anom, basin, None, 0.0), *args)
    plain = sst_mirror.run_year(o, start, CO2, None, *args)
    o.close()
    tclim2 = warmer_tclim(inputs)
    o2 = oracle_lib.Oracle(dataclasses.replace(inputs, tclim=tclim2), params)
    o2.flux_correction(1)
    start2 = budget_mirror.MirrorStart(o2)
    c5 = sst_mirror.run_year(o2, start2, CO2, s3, tclim2, inputs.z_topo, inputs.sw_solar)
    o2.close()
    out = dict(start=dict(corr=start.corr, state=start.state5), case3=c3, member=member, control=control, plain=plain,
               start2=dict(corr=start2.corr, state=start2.state5), case5=c5, basin=basin)
    for y in (c3, member, control, plain, c5):
        for a in y:
            a.setflags(write=False)
    for a in (start.corr, start.state5, start2.corr, start2.state5, basin):
        a.setflags(write=False)
    return out


def warmer_tclim(inputs):
    """A boundary set's own tclim: the workload's plus 0.5 K at the equator falling to 0 at the poles."""
    lat = np.deg2rad((np.arange(inputs.ny) + 0.5) * 180.0 / inputs.ny - 90.0)
    return np.ascontiguousarray(np.asarray(inputs.tclim, np.float32) + (0.5 * np.cos(lat)).astype(np.float32)[None, :, None])


# ------------------------------------------------------------------------------------------------ 1. equals the switch
@pytest.mark.parametrize("kind,strict", ALL_KINDS, ids=KIND_IDS)
def test_all_ones_anomaly_equals_the_switch(eng_mod, params, inputs, kind, strict):
    """Members: the switch; pattern 0 (anomaly 1 everywhere) at amp 1; pattern 1 (anomaly 0.5, season 2) at amp 1 -- a product
    that is exact; none.  No weight table."""
    from greb_climate_model_amd import abi
    inp, p = kind_inputs(kind, inputs, params)
    ref = unforced(eng_mod, inputs, params, kind, strict)
    ones = np.ones((2, inp.ny, inp.nx), np.float32)
    ones[1] = 0.5
    season = np.ones((2, 730), np.float32)
    season[1] = 2.0
    e = sst_engine(eng_mod, inputs, params, kind, strict, 4, ref, ones, None, season,
                   [{}, {"pattern": 0, "amp": 1.0}, {"pattern": 1}, {}])
    e.set_member_experiments([abi.X_SST_PLUS1, 0, 0, 0])
    d = e.describe()
    assert d["sst"] == {"patterns": 2, "prescribed_members": 2} and d["forcing"]["forced_members"] == 0, d
    assert d["kernel_family"]["scenario"] == "forcing" and d["kernel_family"]["flux_correction"] != "forcing", d
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    label = f"{kind} {ids(strict)}"
    same((mon[1], yr[1], st[1]), (mon[0], yr[0], st[0]), label + " all-ones pattern against the switch")
    same((mon[2], yr[2], st[2]), (mon[0], yr[0], st[0]), label + " 0.5 x 2 pattern against the switch")
    same((mon[3], yr[3], st[3]), ref["run"], label + " plain member beside them")
    assert rms(mon[0, 0, 11, 0], mon[3, 0, 11, 0]) > 0.1  # (December Tsurf: the switch is another run)


# ------------------------------------------------------------------------------------------------ 2. neutral
@pytest.mark.parametrize("kind,strict", ALL_KINDS, ids=KIND_IDS)
def test_weight_zero_equals_the_unforced_engine(eng_mod, params, inputs, kind, strict):
    """Two members: weight 0 everywhere at amp 123; none.  Both run the forcing-aware kernels and equal the plain engine.
    If FAST differs here, the cause is in how the blend is contracted: to be fixed there."""
    inp, p = kind_inputs(kind, inputs, params)
    ref = unforced(eng_mod, inputs, params, kind, strict)
    rng = np.random.default_rng(3)
    anom = rng.standard_normal((1, inp.ny, inp.nx)).astype(np.float32)
    e = sst_engine(eng_mod, inputs, params, kind, strict, 2, ref, anom, np.zeros_like(anom), None, [{"pattern": 0, "amp": 123.0}, {}])
    assert e.describe()["sst"] == {"patterns": 1, "prescribed_members": 1}
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    for m in range(2):
        same((mon[m], yr[m], st[m]), ref["run"], f"{kind} {ids(strict)} neutral member {m}")


# ------------------------------------------------------------------------------------------------ 3. against the mirror
_case3 = {}


def case3_engine(eng_mod, inputs, params, mirror, strict):
    anom, weight, season, _ = sst_mirror.case3(inputs)
    return sst_engine(eng_mod, inputs, params, "fused", strict, 1, mirror["start"], anom, weight, season, [{"pattern": 0, "amp": 2.0}])


def case3_run(eng_mod, inputs, params, mirror, strict):
    if strict not in _case3:
        e = case3_engine(eng_mod, inputs, params, mirror, strict)
        mon, yr = e.run(1, CO2)
        _case3[strict] = (mon[0], yr[0], e.state(0))
        e.close()
    return _case3[strict]


def against_mirror(tag, mon, yr, want, strict, lines=None):
    for i, tol in enumerate(TOL):
        r = rms(mon[0, :, i], want[0][:, i])
        line = f"{tag} field {i}: RMS {r:.3e} (bar {tol:.0e})"
        print(line)
        if lines is not None:
            lines.append(line)
        assert r < tol, (tag, i, r)
    print(f"{tag} yearly: engine {yr.tolist()} mirror {want[3].tolist()}")
    yearly_close(yr[0], want[3], strict)


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_prescribed_run_against_the_mirror(eng_mod, params, inputs, mirror, strict):
    """The measured RMS of every field is printed and written to profiles/sst_parity_numbers.txt."""
    mon, yr, _ = case3_run(eng_mod, inputs, params, mirror, strict)
    lines = []
    against_mirror(f"prescribed SST vs mirror {ids(strict).upper()}", mon, yr, mirror["case3"], strict, lines)
    # the hook is in there: the mirror's plain December differs by far more than the bars
    assert rms(mirror["case3"][0][11, 0], mirror["plain"][0][11, 0]) > 1e-2
    path = os.path.join(ROOT, "profiles", "sst_parity_numbers.txt")
    try:  # (a record for the repository, not part of the check; a read-only tree keeps the committed one)
        old = [l for l in open(path).read().splitlines() if not l.startswith(f"prescribed SST vs mirror {ids(strict).upper()}")] if os.path.exists(path) else \
            ["# prescribed SST (a 30-degree patch at amp 2, basin weight with a 15-degree buffer, a season that changes sign) at 680 ppm against",
             "# tests/sst_mirror.py, 96x48 fused member kernel, one scenario year: RMS of the monthly records per field",
             "# (tests/test_gpu_sst.py::test_prescribed_run_against_the_mirror)"]
        open(path, "w").write("\n".join(old + lines) + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------ 4. locality
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_the_hook_is_local_and_the_response_is_not(eng_mod, params, inputs, mirror, strict):
    """Two members with weight 1 on the tropical Pacific only: the patch at amp 2, and its control at amp 0.
    After ONE run year the member's land-point Ts differs from the control's -- the atmosphere carries the anomaly ashore
    within weeks (the mirror: up to 6e-3 K) -- so equality of what the hook does not touch is NOT expected, and not asserted.
    What is exact: at ocean points where the weight and the anomaly are 0 the hook does nothing, so there the member follows
    the mirror's member, whose hook does nothing there either, within TOL.  (The mirror's year WITHOUT any hook is no
    yardstick for those points: the mirror's own member is 1.6e-2 K RMS away from it there, the far field of the response;
    the distance is printed.)  And the response is where the patch is: the December Tsurf difference to the control has an
    RMS over the patch many times its RMS over the far hemisphere -- the ratio is the mirror's, matched within 10 %."""
    anom = sst_mirror.case3(inputs)[0]
    basin = mirror["basin"]
    e = sst_engine(eng_mod, inputs, params, "fused", strict, 2, mirror["start"], anom, basin, None,
                   [{"pattern": 0, "amp": 2.0}, {"pattern": 0, "amp": 0.0}])
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    ocean = np.asarray(inputs.z_topo) < 0
    land_diff = float(np.abs(st[0, 0][~ocean].astype(np.float64) - st[1, 0][~ocean]).max())
    print(f"{ids(strict)}: land-point Ts, member against control after one year: max |difference| {land_diff:.3e} K (not expected to be 0)")
    untouched = ocean & (basin == 0) & (anom == 0)
    assert untouched.sum() > 1000
    for i, tol in enumerate(TOL):
        r = rms(mon[0, 0, :, i][:, untouched], mirror["member"][0][:, i][:, untouched])
        away = rms(mirror["member"][0][:, i][:, untouched], mirror["plain"][0][:, i][:, untouched])
        print(f"{ids(strict)} untouched ocean field {i}: engine against the mirror's member RMS {r:.3e} (bar {tol:.0e}); "
              f"the mirror's member against the mirror's plain year {away:.3e}")
        assert r < tol, (i, r)
    for i, tol in enumerate(TOL):  # the control too is the mirror's
        assert rms(mon[1, 0, :, i], mirror["control"][0][:, i]) < tol, i
    lat = (np.arange(inputs.ny) + 0.5) * 180.0 / inputs.ny - 90.0
    from greb_climate_model_amd import forcing
    j, i0 = np.unravel_index(int(np.argmax(anom)), anom.shape)
    patch, far = anom > 0.5, far_side(inputs, lat[j], forcing.longitudes(inputs.nx)[i0])
    want = response_ratio(mirror["member"][0][11, 0], mirror["control"][0][11, 0], patch, far)
    got = response_ratio(mon[0, 0, 11, 0], mon[1, 0, 11, 0], patch, far)
    print(f"{ids(strict)}: December Tsurf response, RMS over the patch / RMS over the far hemisphere: engine {got:.1f}, mirror {want:.1f}")
    assert want > 5.0, want  # (several times: the mirror's own number, on the CPU)
    assert abs(got - want) <= 0.1 * want, (got, want)


# ------------------------------------------------------------------------------------------------ 5. same run; a set's own tclim
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_run_run_budget_and_run_diag_are_the_same_run(eng_mod, params, inputs, mirror, strict):
    from greb_climate_model_amd import abi, diag
    mon, yr, st = case3_run(eng_mod, inputs, params, mirror, strict)
    e = case3_engine(eng_mod, inputs, params, mirror, strict)
    mon_b, _, yr_b = e.run_budget(1, CO2)
    st_b = e.state(0)
    e.close()
    same((mon_b[0], yr_b[0], st_b), (mon, yr, st), f"{ids(strict)} run_budget against run")
    e = case3_engine(eng_mod, inputs, params, mirror, strict)
    plan = diag.Plan(inputs.nx, inputs.ny)
    res = e.run_diag(1, CO2, plan, abi.D_ANNUAL)
    st_d = e.state(0)
    e.close(); plan.close()
    assert np.array_equal(res.yearly[0], yr) and np.array_equal(st_d, st)
    ann = diag.reduce_reference(mon)[2]  # [1][5][ny][nx], fp64
    ulp = np.spacing(np.abs(ann).astype(np.float32)).astype(np.float64)
    assert (np.abs(res.annual[0].astype(np.float64) - ann) / ulp).max() <= 1.0


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_a_member_on_a_boundary_set_is_held_to_that_sets_tclim(eng_mod, params, inputs, mirror, strict):
    """Member 0 on the engine's own data, member 1 on a set with its own tclim, both with case 3's pattern at amp 2: member 1
    against the mirror started from that set (its own spin-up, its own tclim in the hook), member 0 equal to case 3's run."""
    anom, weight, season, _ = sst_mirror.case3(inputs)
    e = eng_mod.Engine(inputs, params, n_members=2, strict=strict)
    s = e.add_boundary_set(tclim=warmer_tclim(inputs))
    e.set_member_boundary([0, s])
    e.set_corrections(mirror["start"]["corr"], mirror["start"]["state"], 0)
    e.set_corrections(mirror["start2"]["corr"], mirror["start2"]["state"], 1)
    e.set_sst_tables(anom, weight, season)
    e.set_member_sst([{"pattern": 0, "amp": 2.0}] * 2)
    d = e.describe()
    assert d["kernel_family"]["scenario"] == "boundary" and d["sst"]["prescribed_members"] == 2, d
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    against_mirror(f"prescribed SST on a set vs mirror {ids(strict).upper()}", mon[1], yr[1], mirror["case5"], strict)
    same((mon[0], yr[0], st[0]), case3_run(eng_mod, inputs, params, mirror, strict), f"{ids(strict)} member on set 0 beside it")
    # (held to ITS tclim: against the mirror of the engine's own tclim the bars would not hold)
    assert rms(mon[1, 0, :, 0], mirror["case3"][0][:, 0]) > 100 * TOL[0]


# ------------------------------------------------------------------------------------------------ 6. beside a plain member
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_prescribed_member_beside_a_plain_member(eng_mod, params, inputs, mirror, strict):
    anom, weight, season, _ = sst_mirror.case3(inputs)
    e = sst_engine(eng_mod, inputs, params, "fused", strict, 2, mirror["start"], anom, weight, season, [{}, {"pattern": 0, "amp": 2.0}])
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    same((mon[1], yr[1], st[1]), case3_run(eng_mod, inputs, params, mirror, strict), f"{ids(strict)} prescribed member")
    p = eng_mod.Engine(inputs, params, strict=strict)
    p.set_corrections(mirror["start"]["corr"], mirror["start"]["state"])
    pm, py = p.run(1, CO2)
    ps = p.state(0)
    assert p.describe()["kernel_family"]["scenario"] == "default"
    p.close()
    same((mon[0], yr[0], st[0]), (pm[0], py[0], ps), f"{ids(strict)} plain member beside it")


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
    a3, w3, s3, _ = sst_mirror.case3(inputs)
    anom = np.ascontiguousarray(np.stack([np.ones_like(a3), a3]))
    weight = np.ascontiguousarray(np.stack([w3, w3]))
    season = np.ascontiguousarray(np.stack([s3, s3]))
    good = [{"pattern": 1, "amp": 2.0}]
    forcing_before = None

    def engine():
        return sst_engine(eng_mod, inputs, params, "fused", strict, 1, ref, anom, weight, season, good)

    e = engine()
    forcing_before = e.describe()["forcing"]
    assert forcing_before == {"patterns": 0, "solar_tables": 0, "forced_members": 0}
    ptr = lambda x: None if x is None else abi.fptr(x)
    tables = lambda n, a, w, s: L.greb_engine_set_sst_tables(e.h, n, ptr(a), ptr(w), ptr(s))

    def member(**kw):
        f = (abi.GrebMemberSst * 1)()
        f[0].pattern, f[0].amp = -1, 1.0
        for k, v in kw.items():
            setattr(f[0], k, v)
        return L.greb_engine_set_member_sst(e.h, f)

    big = np.ones((1025, 5, 12), np.float32)  # (rejected before anything of it is read)
    _rejected(eng_mod, e, tables(1025, big, None, None), "n_patterns", "1025")
    _rejected(eng_mod, e, tables(-1, None, None, None), "n_patterns", "-1")
    _rejected(eng_mod, e, tables(2, None, weight, season), "anom is NULL")
    for bad, word in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
        a = anom.copy(); a[1, 7, 5] = bad
        _rejected(eng_mod, e, tables(2, a, None, None), "anom", "pattern 1", "row 7", "column 5", word)
        s = season.copy(); s[0, 364] = bad
        _rejected(eng_mod, e, tables(2, anom, None, s), "season", "pattern 0", "step 365", word)
    for bad, word in ((np.nan, "nan"), (1.5, "1.5"), (-0.25, "-0.25"), (np.inf, "inf")):
        w = weight.copy(); w[1, 7, 5] = bad
        _rejected(eng_mod, e, tables(2, anom, w, None), "weight", "pattern 1", "row 7", "column 5", word)
    _rejected(eng_mod, e, tables(1, anom[:1], None, None), "member 0", "pattern 1")  # fewer patterns than a member names
    _rejected(eng_mod, e, member(pattern=2), "member 0", "pattern 2")
    _rejected(eng_mod, e, member(pattern=-2), "member 0", "pattern -2")
    for bad, word in ((np.nan, "amp nan"), (np.inf, "amp inf")):
        _rejected(eng_mod, e, member(pattern=0, amp=bad), "member 0", word)
    with pytest.raises(eng_mod.GrebError):
        e.set_member_sst([{"pattern": 0, "amplitude": 1.0}])
    with pytest.raises(eng_mod.GrebError):
        e.set_member_sst([{}, {}])
    with pytest.raises(eng_mod.GrebError):
        e.set_sst_tables(anom[:, :-1])
    with pytest.raises(eng_mod.GrebError):
        e.set_sst_tables(anom, weight[:1])
    d = e.describe()
    assert d["sst"] == {"patterns": 2, "prescribed_members": 1} and d["forcing"] == forcing_before, d
    got = e.run(1, CO2) + (e.state(0),)
    # ... equals the run of an engine that never made the rejected calls
    f = engine()
    want = f.run(1, CO2) + (f.state(0),)
    f.close()
    same(got, want, f"{ids(strict)} after the rejected calls")
    assert not np.array_equal(got[0][0], ref["run"][0])  # (and that run was prescribed)
    # clearing returns to the default kernels; tables may then shrink, and the indices are validated against the new ones
    e.set_member_sst(None)
    d = e.describe()
    assert d["sst"] == {"patterns": 2, "prescribed_members": 0} and d["kernel_family"]["scenario"] == "default", d
    e.set_sst_tables(anom[:1])
    assert e.describe()["sst"] == {"patterns": 1, "prescribed_members": 0}
    _rejected(eng_mod, e, member(pattern=1), "member 0", "pattern 1")
    e.set_corrections(ref["corr"], ref["state"])
    mon, yr = e.run(1, CO2)  # the second scenario year of this engine's clock: the year's records are those of a first year
    same((mon[0], yr[0], e.state(0)), ref["run"], f"{ids(strict)} cleared SST")
    e.set_sst_tables(None)
    assert e.describe()["sst"] == {"patterns": 0, "prescribed_members": 0} and e.describe()["forcing"] == forcing_before
    e.close()


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_flux_correction_ignores_prescribed_sst(eng_mod, params, inputs, strict):
    ref = unforced(eng_mod, inputs, params, "fused", strict)
    anom, weight, season, _ = sst_mirror.case3(inputs)
    e = eng_mod.Engine(inputs, params, n_members=2, strict=strict)
    e.set_sst_tables(anom, weight, season)
    e.set_member_sst([{"pattern": 0, "amp": 2.0}, {}])
    d = e.describe()
    assert d["sst"]["prescribed_members"] == 1 and d["correction_sets"] == 1 and d["forcing"]["forced_members"] == 0, d
    yf = e.flux_correction(1)
    for m in range(2):
        corr, st = e.get_corrections(m)
        assert np.array_equal(corr, ref["corr"]) and np.array_equal(st, ref["state"]) and np.array_equal(yf[m], ref["flux_yearly"][0]), m
    e.close()
