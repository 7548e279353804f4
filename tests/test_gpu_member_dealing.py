"""GPU: the deal of member-year chunks (greb_member.hip: a launch of more members than workgroups cuts every member's steps
into chunks and deals (member, chunk) items to the workgroups from a ready queue) changes no bit of any result.  The
yardstick is the same engine with dealing off -- workgroup b integrates member b for the whole launch.  One flux-correction
year, then two scenario years; the members differ in kappa and da_ice, so each has its own row tables and its own
correction set and the flux-correction year is dealt as well.  Compared byte for byte: monthly records, yearly values, the
state and the corrections of every member; with budget output the budget records too.  A workgroup that gave up waiting
for an item would make the run fail with GREB_E_STATE (engine.GrebError): the status word reads clean when it returns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (members, workgroups): 3 on 2 -- a workgroup takes chunks of different members and a member's chunks run on different
# workgroups; 1 on 2 -- one workgroup waits in the pop while the other computes, and the run ends through the index beyond
# the capacity; 5 on 5 -- nobody waits.  The last two only deal because they are forced to.
CASES = {"3on2": (3, 2), "1on2": (1, 2), "5on5": (5, 5)}
_reference = {}


def _members(n):
    return [{"kappa": 8e5 * (1.0 + 0.04 * m), "da_ice": 0.25 + 0.01 * m} for m in range(n)]


def _run(inputs, params, n, strict, budget, dealing):
    from greb_climate_model_amd import engine
    e = engine.Engine(inputs, params, members=_members(n), strict=strict)
    try:
        if dealing is None:
            e.set_dealing(workgroups=-1)
        else:
            e.set_dealing(workgroups=dealing, force=True)
        out = {"flux_yearly": e.flux_correction(1)}
        co2 = np.linspace(340.0, 700.0, 2 * n, dtype=np.float32).reshape(n, 2)
        if budget:
            out["monthly"], out["budget"], out["yearly"] = e.run_budget(2, co2)
        else:
            out["monthly"], out["yearly"] = e.run(2, co2)
        for m in range(n):
            out[f"corr{m}"], out[f"state{m}"] = e.get_corrections(m)
        launches = e.describe()["dealing"]["dealt_launches"]
    finally:
        e.close()
    return out, launches


def _check(inputs, params, case, strict, budget):
    n, wg = CASES[case]
    key = (n, strict, budget)
    if key not in _reference:  # the run with dealing off, once per (members, arithmetic, output)
        _reference[key], launches = _run(inputs, params, n, strict, budget, None)
        assert launches == 0
    ref = _reference[key]
    got, launches = _run(inputs, params, n, strict, budget, wg)
    assert launches == 3, launches  # the flux-correction year and both scenario years went through the queue
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert got[k].tobytes() == ref[k].tobytes(), (case, k, int((got[k] != ref[k]).sum()))
    assert np.isfinite(ref["monthly"]).all() and float(np.abs(ref["monthly"][:, 1] - ref["monthly"][:, 0]).max()) > 0.0


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
@pytest.mark.parametrize("case", list(CASES))
def test_dealt_years_are_the_undealt_years_byte_for_byte(inputs, params, case, strict):
    _check(inputs, params, case, strict, budget=False)


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_dealt_years_with_budget_output(inputs, params, strict):
    _check(inputs, params, "3on2", strict, budget=True)


@pytest.mark.parametrize("schedule", ["equal", "quarters"])
def test_the_other_chunk_schedules_give_the_same_bytes(inputs, params, schedule):
    """Ten equal chunks, or the first half cut in two, instead of the halving schedule: other cuts, the same results."""
    from greb_climate_model_amd import abi, engine
    ref = _reference.get((3, False, False)) or _run(inputs, params, 3, False, False, None)[0]
    e = engine.Engine(inputs, params, members=_members(3))
    try:
        e.set_dealing(workgroups=2, schedule={"equal": abi.CHUNKS_EQUAL, "quarters": abi.CHUNKS_QUARTERS}[schedule])
        e.flux_correction(1)
        monthly, yearly = e.run(2, np.linspace(340.0, 700.0, 6, dtype=np.float32).reshape(3, 2))
        assert e.describe()["dealing"]["dealt_launches"] == 3
    finally:
        e.close()
    assert monthly.tobytes() == ref["monthly"].tobytes() and yearly.tobytes() == ref["yearly"].tobytes()
