"""GPU: boundary sets (greb_engine_add_boundary_set, greb_engine_set_member_boundary) -- members of one engine on different
boundary data, in both phases.

1. The ten pinned experiments of the upstream deconstruction as ONE engine (original.run_deconstruction) against
   tests/golden/logexp_g96.npz, and bit for bit against original.run_original of each experiment.
2. A member on a set equals the engine created on those fields, bit for bit (STRICT and FAST, fused kernel): corrections,
   console values, monthly records, state; run, run_budget and run_diag are the same run; 1 + 1 years equal 2 years.
3. A set of copies of the engine's own fields changes nothing; correction sets are shared while the members' sets agree.
4. The response use: spin up on shared data, then move one member to another set without touching its state.
5. Cases 2 on the latitude bands (96x48, multilaunch) and the row strips (192x48) with a set the transport kernels do not
   read; a set they do read is GREB_E_UNSUPPORTED there.
6. Errors: every validation rule; a rejected call changes nothing and consumes no set id.
Every case is one flux-correction year (or set_corrections from a shared spun-up state) and one or two scenario years of
at most ten members."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from conftest import load_golden, rms
from test_gpu_forcing import KINDS, kind_inputs
from test_gpu_logexp import PINNED, TOL  # the pinned experiments and the RMS bounds of a monthly-mean field: imported, not copied

pytestmark = pytest.mark.gpu

CO2 = 680.0
MODES = [False, True]  # strict
ids = lambda s: "strict" if s else "fast"
NINE = ("z_topo", "glacier", "tclim", "qclim", "uclim", "vclim", "mldclim", "cldclim", "swetclim")


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


def same(got, want, label):
    for name in want:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and np.array_equal(a, b), (label, name, float(np.abs(a.astype(np.float64) - b).max()))


# ------------------------------------------------------------------------------------------------ the sets and the yardsticks
def overrides(inp, name):
    """set1: what the transport reads -- topography cut at 1 m, zonal wind halved, meridional wind rolled by 8 longitudes
    (asymmetric: a kernel that still reads an engine-wide wind or weight pointer cannot pass); set2: every other field."""
    if name == "set1":
        return dict(z_topo=np.where(inp.z_topo > 1.0, np.float32(1.0), inp.z_topo).astype(np.float32),
                    uclim=(inp.uclim * np.float32(0.5)).astype(np.float32), vclim=np.roll(inp.vclim, 8, axis=-1).copy())
    if name == "set2":
        return dict(cldclim=np.full_like(inp.cldclim, 0.7), qclim=np.full_like(inp.qclim, 0.0052), mldclim=np.full_like(inp.mldclim, 50.0),
                    glacier=np.zeros_like(inp.glacier), swetclim=(inp.swetclim * np.float32(0.5)).astype(np.float32),
                    tclim=(inp.tclim + np.float32(1.0)).astype(np.float32))
    assert name == "plain"
    return {}


def merged(inp, name):
    return dataclasses.replace(inp, **overrides(inp, name))


_alone = {}


def alone(eng_mod, inputs, params, kind, strict, name):
    """Computed once per engine kind, mode and set, shared, never changed: a one-member engine CREATED on the merged fields
    -- its flux-correction year (console values, corrections, state) and its scenario year at 680 ppm."""
    k = (kind, strict, name)
    if k not in _alone:
        inp, p = kind_inputs(kind, inputs, params)
        e = eng_mod.Engine(merged(inp, name), p, strict=strict, **KINDS[kind][0])
        assert e.describe()["engine"] == KINDS[kind][1], e.describe()
        yf = e.flux_correction(1)
        corr, st = e.get_corrections(0)
        mon, yr = e.run(1, CO2)
        out = dict(flux_yearly=yf[0], corr=corr, spun_up=st, monthly=mon[0], yearly=yr[0], state=e.state(0))
        e.close()
        for a in out.values():
            a.setflags(write=False)
        _alone[k] = out
    return _alone[k]


def member(e, m, yf, mon, yr, spun):
    return dict(flux_yearly=yf[m], corr=spun[m][0], spun_up=spun[m][1], monthly=mon[m], yearly=yr[m], state=e.state(m))


def restore(e, spun):
    for m, (_, st) in enumerate(spun):
        e.set_corrections(None, st, member=m)


# ------------------------------------------------------------------------------------------------ 1. the deconstruction
@pytest.fixture(scope="module")
def deconstruction(eng_mod, inputs):
    from greb_climate_model_amd import original
    return original.run_deconstruction(inputs, PINNED, 1, 1, 2)


def test_pinned_deconstruction_in_one_engine_matches_the_original_variant(deconstruction):
    g = load_golden("logexp_g96.npz")
    for (ctrl, scen), log_exp in zip(deconstruction, PINNED):
        k = f"le{log_exp:02d}"
        scen = scen.reshape(24, 5, 48, 96)
        for i, tol in enumerate(TOL):
            a, b = rms(scen[-1, i], g[k + "_scen_last"][i]), rms(ctrl[-1, -1, i], g[k + "_ctrl_last"][i])
            c = np.abs(scen[:, i].astype(np.float64).mean((1, 2)) - g[k + "_scen_stats"][:, i, 0]).max()
            print(f"log_exp {log_exp} var {i}: scenario rms {a:.3g}, control rms {b:.3g}, monthly means {c:.3g} (bound {tol:g})")
            assert a < tol, (log_exp, "scenario", i)
            assert b < tol, (log_exp, "control", i)
            assert c < 3 * tol, (log_exp, i)


def test_deconstruction_uses_one_set_for_the_constant_mixed_layer(eng_mod, inputs):
    from greb_climate_model_amd import original
    keys = {le: tuple(sorted(original.experiment_overrides(inputs, le))) for le in PINNED}
    assert {le for le, k in keys.items() if k == ("mldclim",)} == {5, 6, 8, 9, 11}
    assert all(k == () for le, k in keys.items() if le not in (5, 6, 8, 9, 11))


@pytest.mark.parametrize("log_exp", PINNED)
def test_deconstruction_member_is_run_original_bit_for_bit(deconstruction, inputs, log_exp):
    from greb_climate_model_amd import original
    ctrl, scen = original.run_original(inputs, log_exp, 1, 1, 2)
    got_ctrl, got_scen = deconstruction[PINNED.index(log_exp)]
    same(dict(control=got_ctrl, scenario=got_scen), dict(control=ctrl, scenario=scen), f"log_exp {log_exp}")


# ------------------------------------------------------------------------------------------------ 2. a member on a set
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_member_on_a_set_equals_the_engine_created_on_those_fields(eng_mod, inputs, params, strict):
    from greb_climate_model_amd import abi, diag
    names = ["plain", "set1", "set2", "set1"]
    e = eng_mod.Engine(inputs, params, n_members=4, strict=strict)
    s1, s2 = e.add_boundary_set(**overrides(inputs, "set1")), e.add_boundary_set(**overrides(inputs, "set2"))
    assert (s1, s2) == (1, 2)
    assert e.describe()["correction_sets"] == 1 and e.describe()["kernel_family"]["scenario"] == "default"
    e.set_member_boundary([0, s1, s2, s1], reinit=True)
    d = e.describe()
    assert d["correction_sets"] == 4 and d["kernel_family"] == dict(flux_correction="boundary", scenario="boundary"), d
    assert d["boundary"] == dict(sets=2, members_on_sets=3, fields=[["z_topo", "uclim", "vclim"],
                                                                    ["glacier", "tclim", "qclim", "mldclim", "cldclim", "swetclim"]]), d
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(4)]
    mon, yr = e.run(1, CO2)
    got = [member(e, m, yf, mon, yr, spun) for m in range(4)]
    for m, name in enumerate(names):
        same(got[m], alone(eng_mod, inputs, params, "fused", strict, name), f"{ids(strict)} member {m} on {name}")
    same(got[3], got[1], "position independence")
    assert not np.array_equal(got[1]["monthly"], got[0]["monthly"]) and not np.array_equal(got[2]["monthly"], got[0]["monthly"])
    st = np.stack([g["state"] for g in got])
    # the same year through run_budget and run_diag
    restore(e, spun)
    mon_b, bud, yr_b = e.run_budget(1, CO2)
    same(dict(monthly=mon_b, yearly=yr_b, state=np.stack([e.state(m) for m in range(4)])), dict(monthly=mon, yearly=yr, state=st), "run_budget")
    assert np.isfinite(bud).all() and not np.array_equal(bud[1], bud[0]) and np.array_equal(bud[1], bud[3])
    restore(e, spun)
    plan = diag.Plan(inputs.nx, inputs.ny)
    res = e.run_diag(1, CO2, plan, abi.D_ANNUAL)
    plan.close()
    same(dict(yearly=res.yearly, state=np.stack([e.state(m) for m in range(4)])), dict(yearly=yr, state=st), "run_diag")
    assert np.isfinite(res.annual).all() and np.array_equal(res.annual[1], res.annual[3])
    # two one-year calls equal one two-year call
    restore(e, spun)
    mon2, yr2 = e.run(2, CO2)
    st2 = np.stack([e.state(m) for m in range(4)])
    restore(e, spun)
    mon_a, yr_a = e.run(1, CO2)
    mon_c, yr_c = e.run(1, CO2)
    same(dict(first=mon_a[:, 0], yearly_first=yr_a[:, 0], second=mon_c[:, 0], yearly_second=yr_c[:, 0],
              state=np.stack([e.state(m) for m in range(4)])),
         dict(first=mon2[:, 0], yearly_first=yr2[:, 0], second=mon2[:, 1], yearly_second=yr2[:, 1], state=st2), "1 + 1 years against 2")
    same(dict(first=mon_a[:, 0]), dict(first=mon[:, 0]), "the first year again")
    e.close()


# ------------------------------------------------------------------------------------------------ 3. the neutral set
def test_a_set_of_the_engines_own_fields_changes_nothing(eng_mod, inputs, params):
    want = alone(eng_mod, inputs, params, "fused", False, "plain")
    copies = {k: np.array(getattr(inputs, k), np.float32, copy=True) for k in NINE}
    e = eng_mod.Engine(inputs, params, n_members=3)
    s = e.add_boundary_set(**copies)
    e.set_member_boundary([0, s, s])
    d = e.describe()
    assert d["kernel_family"]["flux_correction"] == "boundary" and d["kernel_family"]["scenario"] == "boundary", d
    assert d["correction_sets"] == 3 and d["boundary"]["members_on_sets"] == 2 and d["boundary"]["fields"] == [list(NINE)], d
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(3)]
    mon, yr = e.run(1, CO2)
    for m in range(3):
        same(member(e, m, yf, mon, yr, spun), want, f"member {m} of [0, s, s]")
    # the default kernels again
    e.set_member_boundary(None)
    d = e.describe()
    assert d["kernel_family"] == dict(flux_correction="default", scenario="default") and d["boundary"]["members_on_sets"] == 0, d
    restore(e, spun)
    mon, yr = e.run(1, CO2)
    for m in range(3):
        same(dict(monthly=mon[m], yearly=yr[m], state=e.state(m)), {k: want[k] for k in ("monthly", "yearly", "state")}, f"member {m} after clearing")
    e.close()
    # members that all name the same set keep sharing one correction set
    e = eng_mod.Engine(inputs, params, n_members=3)
    s = e.add_boundary_set(**copies)
    e.set_member_boundary([s, s, s])
    d = e.describe()
    assert d["correction_sets"] == 1 and d["kernel_family"]["flux_correction"] == "boundary", d
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(3)]
    mon, yr = e.run(1, CO2)
    assert e.describe()["correction_sets"] == 1
    for m in range(3):
        same(member(e, m, yf, mon, yr, spun), want, f"member {m} of [s, s, s]")
    e.close()


# ------------------------------------------------------------------------------------------------ 4. the response use
def test_response_to_changed_boundary_data_after_a_shared_spin_up(eng_mod, inputs, params):
    plain = alone(eng_mod, inputs, params, "fused", False, "plain")
    e = eng_mod.Engine(inputs, params, n_members=2)
    e.add_boundary_set(**overrides(inputs, "set1"))
    s2 = e.add_boundary_set(**overrides(inputs, "set2"))
    yf = e.flux_correction(1)  # one shared correction set, on the engine's own data
    assert e.describe()["correction_sets"] == 1
    same(dict(flux_yearly=yf[1]), dict(flux_yearly=plain["flux_yearly"]), "spin-up")
    e.set_member_boundary([0, s2])  # no REINIT: the state stays
    assert e.describe()["correction_sets"] == 2
    for m in range(2):
        corr, st = e.get_corrections(m)
        same(dict(corr=corr, spun_up=st), dict(corr=plain["corr"], spun_up=plain["spun_up"]), f"member {m} keeps corrections and state")
    mon, yr = e.run(1, CO2)
    same(dict(monthly=mon[0], yearly=yr[0], state=e.state(0)), {k: plain[k] for k in ("monthly", "yearly", "state")}, "control member")
    # the changed member: an engine created on set 2's fields that takes over the plain engine's corrections and state
    r = eng_mod.Engine(merged(inputs, "set2"), params)
    r.set_corrections(plain["corr"], plain["spun_up"])
    mon_r, yr_r = r.run(1, CO2)
    same(dict(monthly=mon[1], yearly=yr[1], state=e.state(1)), dict(monthly=mon_r[0], yearly=yr_r[0], state=r.state(0)), "changed member")
    r.close()
    e.close()
    d = rms(mon[1, 0, 11, 0], mon[0, 0, 11, 0])
    print(f"response of December Tsurf to set 2 after one year: RMS {d:.4f} K")
    assert d > 0


# ------------------------------------------------------------------------------------------------ 5. the other engines
@pytest.mark.parametrize("kind,strict", [("bands", False), ("bands", True), ("strips192", False)], ids=lambda v: v if isinstance(v, str) else ids(v))
def test_sets_on_the_any_grid_engine(eng_mod, inputs, params, kind, strict):
    inp, p = kind_inputs(kind, inputs, params)
    e = eng_mod.Engine(inp, p, n_members=2, strict=strict, **KINDS[kind][0])
    assert e.describe()["engine"] == KINDS[kind][1]
    s1, s2 = e.add_boundary_set(**overrides(inp, "set1")), e.add_boundary_set(**overrides(inp, "set2"))
    for sets, field in (([0, s1], "z_topo"), ([s1, s1], "z_topo")):
        with pytest.raises(eng_mod.GrebError) as ei:
            e.set_member_boundary(sets, reinit=True)
        assert ei.value.code == -4 and field in str(ei.value) and "run_beside" in str(ei.value), str(ei.value)
    s3 = e.add_boundary_set(vclim=overrides(inp, "set1")["vclim"])
    with pytest.raises(eng_mod.GrebError) as ei:
        e.set_member_boundary([s3, 0])
    assert ei.value.code == -4 and "vclim" in str(ei.value), str(ei.value)
    d = e.describe()
    assert d["boundary"]["members_on_sets"] == 0 and d["kernel_family"]["scenario"] == "default" and d["correction_sets"] == 1, d
    e.set_member_boundary([0, s2], reinit=True)
    assert e.describe()["correction_sets"] == 2 and e.describe()["kernel_family"]["scenario"] == "boundary"
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(2)]
    mon, yr = e.run(1, CO2)
    for m, name in enumerate(("plain", "set2")):
        same(member(e, m, yf, mon, yr, spun), alone(eng_mod, inputs, params, kind, strict, name), f"{kind} {ids(strict)} member {m} on {name}")
    e.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_rejected_calls_change_nothing(eng_mod, inputs, params):
    from greb_climate_model_amd import abi
    plain = alone(eng_mod, inputs, params, "fused", False, "plain")
    e = eng_mod.Engine(inputs, params, n_members=2)
    e.set_corrections(plain["corr"], plain["spun_up"])
    L = eng_mod.lib()

    def rejected(call, code, *texts):
        with pytest.raises(eng_mod.GrebError) as ei:
            call()
        assert ei.value.code == code and all(t in str(ei.value) for t in texts), (texts, str(ei.value))

    def raw_add(fields_ptr, sid):
        rc = L.greb_engine_add_boundary_set(e.h, fields_ptr, sid)
        if rc:
            raise eng_mod.GrebError(rc, L.greb_engine_last_error(e.h).decode())

    sid = C.c_int(-7)
    rejected(lambda: raw_add(None, C.byref(sid)), -1, "`over` is NULL")
    rejected(lambda: raw_add(C.byref(abi.GrebFields()), C.byref(sid)), -1, "every field of `over` is NULL")
    f = abi.GrebFields()
    sol = np.ascontiguousarray(inputs.sw_solar, np.float32)
    f.sw_solar = abi.fptr(sol)
    f.glacier = abi.fptr(np.ascontiguousarray(inputs.glacier, np.float32))
    rejected(lambda: raw_add(C.byref(f), C.byref(sid)), -1, "sw_solar", "greb_engine_set_forcing_tables")
    assert sid.value == -7
    bad = np.array(inputs.cldclim, np.float32, copy=True)
    bad.reshape(-1)[[123457, 200000]] = [np.nan, np.inf]
    rejected(lambda: e.add_boundary_set(glacier=inputs.glacier, cldclim=bad), -1, "cldclim", "index 123457", "not finite")
    bad = np.array(inputs.z_topo, np.float32, copy=True)
    bad[3, 5] = -np.inf
    rejected(lambda: e.add_boundary_set(z_topo=bad), -1, "z_topo", f"index {3 * inputs.nx + 5}")
    assert e.describe()["boundary"]["sets"] == 0
    rejected(lambda: e.set_member_boundary([0, 1]), -1, "member 1", "set 1", "outside 0 ... 0")
    # a rejected add_boundary_set has consumed no set id
    assert e.add_boundary_set(glacier=np.zeros_like(inputs.glacier)) == 1
    rejected(lambda: e.set_member_boundary([2, 0]), -1, "member 0", "set 2")
    rejected(lambda: e.set_member_boundary([0, -1]), -1, "member 1", "set -1")
    ids2 = np.array([0, 1], np.int32)
    for flags in (2, 3, 0x80000000):
        rc = L.greb_engine_set_member_boundary(e.h, ids2.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint(flags))
        assert rc == -1 and "unknown flag bits" in L.greb_engine_last_error(e.h).decode(), (flags, rc)
    for k in range(2, abi.MAX_BOUNDARY_SETS + 1):
        assert e.add_boundary_set(glacier=np.full_like(inputs.glacier, 1.0 / k)) == k
    rejected(lambda: e.add_boundary_set(glacier=inputs.glacier), -1, "already has 16")
    d = e.describe()
    assert d["boundary"]["sets"] == 16 and d["boundary"]["members_on_sets"] == 0 and d["correction_sets"] == 1, d
    assert d["kernel_family"] == dict(flux_correction="default", scenario="default"), d
    mon, yr = e.run(1, CO2)
    for m in range(2):
        same(dict(monthly=mon[m], yearly=yr[m], state=e.state(m)), {k: plain[k] for k in ("monthly", "yearly", "state")}, f"member {m} after the rejected calls")
    # the sixteenth set is usable: an ice-free member beside the control
    e.set_corrections(plain["corr"], plain["spun_up"])
    e.set_member_boundary([0, 16])
    mon, yr = e.run(1, CO2)
    same(dict(monthly=mon[0], yearly=yr[0]), {k: plain[k] for k in ("monthly", "yearly")}, "control beside set 16")
    assert np.isfinite(mon[1]).all() and not np.array_equal(mon[1], mon[0])
    e.close()
