"""GPU: every variant of the step kernels (greb_kernels.h: kVariants) launched through the one selection, on the fused
member kernel and on the latitude bands, FAST and STRICT.

A two-member engine whose member 1 carries a feature -- a switch, a forced pattern, a boundary set, or the last two
together -- and whose member 0 is plain takes, for BOTH members, the variant that feature selects; run_budget puts the
budget variant of it on top.  Member 0 then must be, bit for bit, the member of a one-member default engine: console
values and corrections of the flux-correction year, monthly records, console values and state of the scenario year.
A launch that picked a kernel built for another mask either faults or moves member 0.

                                 flux-correction year     run                        run_budget
  nothing                        FLUX                     0                          BUDGET
  switch                         FLUX|EXP                 EXP                        EXP|BUDGET
  forced                         FLUX                     EXP|FORCE                  EXP|BUDGET|FORCE
  on a set                       FLUX|EXP|BOUND           EXP|FORCE|BOUND            EXP|BUDGET|FORCE|BOUND
  forced + on a set              FLUX|EXP|BOUND           EXP|FORCE|BOUND            EXP|BUDGET|FORCE|BOUND

96x48 only; every case is one flux-correction year and two scenario years (the same year through run and run_budget) of two
members.  The yardstick is test_gpu_boundary's `alone(..., "plain")`: computed once per engine kind and mode, shared, never
changed."""
import numpy as np
import pytest

from test_gpu_boundary import CO2, alone, ids, overrides, restore, same
from test_gpu_forcing import KINDS, hemispheres

pytestmark = pytest.mark.gpu

MODES = [False, True]  # strict
ENGINES = ["fused", "bands"]
# feature of member 1 -> describe()["kernel_family"] as the engine reported it before the selection became one function
CASES = {
    "nothing": dict(flux_correction="default", scenario="default"),
    "switch": dict(flux_correction="switches", scenario="switches"),
    "forced": dict(flux_correction="default", scenario="forcing"),
    "on_a_set": dict(flux_correction="boundary", scenario="boundary"),
    "forced_on_a_set": dict(flux_correction="boundary", scenario="boundary"),
}


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


def two_members(eng_mod, inputs, params, kind, strict, case):
    from greb_climate_model_amd import abi
    members = [{}, {"switches": abi.X_NO_ICE}] if case == "switch" else [{}, {}]
    e = eng_mod.Engine(inputs, params, strict=strict, members=members, **KINDS[kind][0])
    assert e.describe()["engine"] == KINDS[kind][1], e.describe()
    if "forced" in case:
        e.set_forcing_tables(hemispheres(inputs.ny, inputs.nx))
        e.set_member_forcing([{}, {"co2_pattern": 0, "co2_ref": 340.0}])
    if "on_a_set" in case:  # a field the transport kernels of the bands do not read
        e.set_member_boundary([0, e.add_boundary_set(cldclim=overrides(inputs, "set2")["cldclim"])], reinit=True)
    return e


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("kind", ENGINES)
def test_plain_member_beside_a_feature_is_the_default_engine(eng_mod, inputs, params, kind, strict, case):
    want = alone(eng_mod, inputs, params, kind, strict, "plain")
    label = f"{kind} {ids(strict)} {case}"
    e = two_members(eng_mod, inputs, params, kind, strict, case)
    assert e.describe()["kernel_family"] == CASES[case], (label, e.describe())
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(2)]
    mon, yr = e.run(1, CO2)
    same(dict(flux_yearly=yf[0], corr=spun[0][0], spun_up=spun[0][1], monthly=mon[0], yearly=yr[0], state=e.state(0)), want, label + ": run")
    if case != "nothing":  # the feature acts: member 1 is another run
        assert not np.array_equal(mon[1], mon[0]), label
    restore(e, spun)
    mon_b, bud, yr_b = e.run_budget(1, CO2)
    same(dict(monthly=mon_b[0], yearly=yr_b[0], state=e.state(0)), {k: want[k] for k in ("monthly", "yearly", "state")}, label + ": run_budget")
    assert np.array_equal(mon_b[1], mon[1]) and np.isfinite(bud).all(), label
    assert np.array_equal(bud[1], bud[0]) == (case == "nothing"), label
    e.close()
