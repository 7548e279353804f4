"""GPU: the packed forcing records of the FAST fused 96x48 member kernel (greb_kernels.h: forcing record).

The kernel reads the boundary data of its point physics from one record per boundary set, made on the device when the
set's data is uploaded, with the wind-speed term of the latent heat flux finished.  Checked here: what the pack kernel
wrote (debug read-back), a run across the year boundary (step 1 reads the mixed-layer depth of step 730), the record route
against the array route of the any-grid engine on the same arithmetic, members on different sets and a set made after the
engine has run, and a plain member in the switch-aware, forcing and budget instantiations.

Two-member engines at most, one flux-correction and one scenario year each."""
import dataclasses

import numpy as np
import pytest

from conftest import load_golden, yearly_close
from test_gpu_boundary import CO2, alone, restore, same
from test_gpu_members import Result, bit_for_bit
from test_gpu_parity import _check_run
from test_gpu_variants import two_members

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


# ------------------------------------------------------------------------------------------------ read-back
ZERO_TOPO = ((10, 7), (30, 50), (5, 1))    # (row, longitude): z_topo exactly 0
ZERO_WIND = ((5, 1), (5, 93), (40, 22))    # u = v = 0 in every step: one in the first quad of a row, one in the last


def edge_inputs(inp):
    z = inp.z_topo.copy()
    u, v = inp.uclim.copy(), inp.vclim.copy()
    for k, i in ZERO_TOPO:
        z[k, i] = 0.0
    for k, i in ZERO_WIND:
        u[:, k, i] = 0.0
        v[:, k, i] = 0.0
    return dataclasses.replace(inp, z_topo=z, uclim=u, vclim=v)


def wind_fp64(u, v, z):
    w = np.sqrt(u.astype(np.float64) ** 2 + v.astype(np.float64) ** 2)
    return np.where(z > 0, np.sqrt(w * w + 4.0), np.where(z < 0, np.sqrt(w * w + 9.0), w))


def test_record_read_back(eng_mod, inputs, params):
    """Steps 1, 2 and 730 of the record of the engine's own data.  Copied fields: byte-equal to the uploaded arrays (z_ocean =
    3 x the largest mixed-layer depth is exact in fp32; wz_air = expf(-z_topo / z_air) is made by the host's libm, against
    numpy's to 5e-7: two roundings of two exp implementations).  Wind-speed term: 1e-6 relative to the float64 formula --
    three chained hardware square roots at <= 2 ulp and five roundings, about 5e-7."""
    inp = edge_inputs(inputs)
    assert (inp.z_topo < 0).any() and (inp.z_topo == 0).sum() >= len(ZERO_TOPO) and (inp.z_topo > 0).any()
    lay = eng_mod.forcing_record_layout()
    F = {n: i for i, n in enumerate(lay.names)}
    e = eng_mod.Engine(inp, params, n_members=2)
    d = e.describe()
    assert d["engine"] == "fused member kernel" and d["forcing_records"] == {"sets": 1, "bytes": lay.record_bytes}, d
    for step in (1, 2, 730):
        r = e.forcing_record(step)
        t, tm = step - 1, (step - 2) % 730
        for name, want in (("z_topo", inp.z_topo), ("glacier", inp.glacier), ("tclim", inp.tclim[t]), ("cldclim", inp.cldclim[t]),
                           ("mldclim", inp.mldclim[t]), ("mldclim_prev", inp.mldclim[tm]), ("swetclim", inp.swetclim[t]),
                           ("z_ocean", f32(3.0) * inp.mldclim.max(axis=0))):
            assert r[:, F[name], :].tobytes() == np.ascontiguousarray(want, f32).tobytes(), (step, name)
        assert np.allclose(r[:, F["wz_air"], :], np.exp(-inp.z_topo.astype(np.float64) / params.z_air), rtol=5e-7, atol=0), step
        got, want = r[:, F["wind_speed"], :].astype(np.float64), wind_fp64(inp.uclim[t], inp.vclim[t], inp.z_topo)
        err = np.abs(got - want)
        print(f"step {step}: wind-speed term, largest relative error {np.max(err / np.maximum(want, 1e-30)):.2e}")
        assert (err <= 1e-6 * want).all(), (step, float(np.max(err / np.maximum(want, 1e-30))))
        for k, i in ZERO_TOPO:  # neither offset where z_topo == 0
            plain = np.sqrt(float(inp.uclim[t, k, i]) ** 2 + float(inp.vclim[t, k, i]) ** 2)
            assert abs(got[k, i] - plain) <= 1e-6 * plain, (step, k, i)
        for k, i in ZERO_WIND:  # the offset alone (covered to 1e-6 above); exactly nothing where z_topo == 0 as well
            assert want[k, i] in (0.0, 2.0, 3.0) and (got[k, i] == 0.0) == (inp.z_topo[k, i] == 0), (step, k, i, got[k, i])
    assert e.forcing_record(1)[:, F["mldclim_prev"], :].tobytes() == e.forcing_record(730)[:, F["mldclim"], :].tobytes()
    with pytest.raises(eng_mod.GrebError):
        e.forcing_record(731)
    with pytest.raises(eng_mod.GrebError):
        e.forcing_record(1, set_id=1)
    e.close()
    s = eng_mod.Engine(inputs, params, strict=True)  # no record where no kernel reads one
    assert s.describe()["forcing_records"] == {"sets": 0, "bytes": 0}
    with pytest.raises(eng_mod.GrebError):
        s.forcing_record(1)
    s.close()


# ------------------------------------------------------------------------------------------------ the year boundary
def test_year_boundary(eng_mod, inputs, params):
    """One member through the flux-correction year (730 steps) and on into the scenario year: step 1 of a year reads the
    mixed-layer depth of step 730.  The scenario year against the reference's output under the bars of test_gpu_parity."""
    g = load_golden("run_short_g96.npz")
    e = eng_mod.Engine(inputs, params)
    yf = e.flux_correction(1)
    mon, yr = e.run(1, 680.0)
    assert np.isfinite(yf).all() and np.isfinite(mon).all() and np.isfinite(yr).all() and np.isfinite(e.state(0)).all()
    _check_run(mon[0].reshape(12, 5, 48, 96), g["monthly"][:12], "records")
    e.close()


# ------------------------------------------------------------------------------------------------ two routes, same bits
def test_record_route_equals_array_route(eng_mod, inputs, params):
    """A member without circulation runs point physics only.  In the fused engine it takes the record route, in the
    any-grid engine at 96x48 the array route (physics_step_kernel), both FAST with contraction off: the same operations
    on the same values, the wind-speed term hoisted on one side only.  State, monthly means and the yearly point value
    agree bit for bit.  The yearly GLOBAL MEAN is not bit-comparable between the two engines, and was not before the
    records (measured on the parent commit: 1.5175171 against 1.5175476 in the flux-correction year, 3.4735413 against
    3.4735107 in the scenario year, monthly means and state identical): the fused FAST kernel sums the 4 608 annual
    means by per-lane partials and a wavefront reduction, the any-grid engine in its own order.  It is held to the bar
    every FAST global mean is held to (conftest.yearly_close)."""
    from greb_climate_model_amd import abi
    members = [{"switches": abi.X_NO_CIRCULATION}]
    out = {}
    for kind, kw in (("fused member kernel", {}), ("latitude bands", dict(multilaunch=True))):
        e = eng_mod.Engine(edge_inputs(inputs), params, members=members, **kw)
        assert e.describe()["engine"] == kind, e.describe()
        assert (e.describe()["forcing_records"]["sets"] == 1) == (kind == "fused member kernel")
        out[kind] = Result(e).member(0)
        e.close()
    (mon, yr, yf, state), (mon_b, yr_b, yf_b, state_b) = out["fused member kernel"], out["latitude bands"]
    print(f"global mean, fused / bands: flux-correction year {yf[0, 0]!r} / {yf_b[0, 0]!r}, scenario year {yr[0, 0]!r} / {yr_b[0, 0]!r}")
    bit_for_bit((mon, yr[:, 1], yf[:, 1], state), (mon_b, yr_b[:, 1], yf_b[:, 1], state_b), "record route against array route")
    yearly_close(yr, yr_b)
    yearly_close(yf, yf_b)


# ------------------------------------------------------------------------------------------------ boundary sets
def wind_and_mld_sets(inp):
    """Two sets whose winds and mixed-layer depths differ from the engine's and from each other."""
    return (dict(uclim=(inp.uclim * f32(0.5)).astype(f32), mldclim=(inp.mldclim * f32(1.25)).astype(f32)),
            dict(vclim=np.roll(inp.vclim, 8, axis=-1).copy(), mldclim=np.full_like(inp.mldclim, 50.0)))


def test_members_on_different_sets_and_a_set_made_later(eng_mod, inputs, params):
    s1, s2 = wind_and_mld_sets(inputs)
    lay = eng_mod.forcing_record_layout()
    single = eng_mod.Engine(dataclasses.replace(inputs, **s1), params)
    want = Result(single).member(0)
    single.close()
    e = eng_mod.Engine(inputs, params, members=[{}, {}])
    e.set_member_boundary([e.add_boundary_set(**s1), e.add_boundary_set(**s2)], reinit=True)
    assert e.describe()["forcing_records"] == {"sets": 3, "bytes": 3 * lay.record_bytes}
    F = lay.names.index("mldclim")
    assert e.forcing_record(5, set_id=1)[:, F, :].tobytes() == s1["mldclim"][4].tobytes()
    assert e.forcing_record(5, set_id=2)[:, F, :].tobytes() == s2["mldclim"][4].tobytes()
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(2)]
    mon, yr = e.run(1, CO2)
    bit_for_bit((mon[0], yr[0], yf[0], e.state(0)), want, "member on set 1 against the engine built on set 1's data")
    assert not np.array_equal(mon[1], mon[0])
    # a set made after the engine has run, on set 1's data: the member moved to it, from member 0's spun-up state and
    # corrections, repeats member 0's year -- and member 0, moved to set 2 with member 1's, repeats member 1's
    later = e.add_boundary_set(**s1)
    assert e.describe()["forcing_records"]["sets"] == 4
    e.set_member_boundary([2, later])
    e.set_corrections(spun[1][0], spun[1][1], member=0)
    e.set_corrections(spun[0][0], spun[0][1], member=1)
    mon2, yr2 = e.run(1, CO2)
    assert np.array_equal(mon2[1], mon[0]) and np.array_equal(yr2[1], yr[0]), "the run after a member's set is replaced uses the new record"
    assert np.array_equal(mon2[0], mon[1]) and np.array_equal(yr2[0], yr[1])
    e.close()


# ------------------------------------------------------------------------------------------------ variants
@pytest.mark.parametrize("case", ["switch", "forced"])
def test_plain_member_in_another_instantiation(eng_mod, inputs, params, case):
    """A member without switches in a switch-aware launch (and in a forcing-aware one) is, bit for bit, what the default
    instantiation makes of it -- through run and through run_budget, the budget instantiation with its pre-pass."""
    want = alone(eng_mod, inputs, params, "fused", False, "plain")
    e = two_members(eng_mod, inputs, params, "fused", False, case)
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(2)]
    mon, yr = e.run(1, CO2)
    same(dict(flux_yearly=yf[0], corr=spun[0][0], spun_up=spun[0][1], monthly=mon[0], yearly=yr[0], state=e.state(0)), want, case + ": run")
    assert not np.array_equal(mon[1], mon[0]), case
    restore(e, spun)
    mon_b, bud, yr_b = e.run_budget(1, CO2)
    same(dict(monthly=mon_b[0], yearly=yr_b[0], state=e.state(0)), {k: want[k] for k in ("monthly", "yearly", "state")}, case + ": run_budget")
    assert np.isfinite(bud).all()
    e.close()
