"""GPU: what the output plans (csrc/greb_plans.cpp) and the member setters (csrc/greb_members.cpp) share.

One plan handle serves its _dev entry point on a torch tensor first -- there its per-device entry is made -- and the
engine's run_* on the same device afterwards, where the entry is found; both must give, bit for bit, what two fresh
plans give that are used once each.  After close() a new plan of the same kind works again.  And a setter that is
refused between two runs leaves nothing behind.  96 x 48, 3 members, 2 years."""
import numpy as np
import pytest

from greb_climate_model_amd import clim, diag, engine, ens

pytestmark = pytest.mark.gpu

NM, YEARS = 3, 2
CO2 = [[400.0] * YEARS, [800.0] * YEARS, [600.0] * YEARS]


def same_bits(got, ref, names, label):
    for name in names:
        g, r = getattr(got, name), getattr(ref, name)
        assert (g is None) == (r is None), (label, name)
        if g is None:
            continue
        g, r = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in (g, r))
        assert g.dtype == np.float32 and g.shape == r.shape, (label, name, g.shape, r.shape)
        bad = g.view(np.uint32) != r.view(np.uint32)
        print(f"{label} {name}: {int(bad.sum())} of {bad.size} values differ")
        assert not bad.any(), (label, name, int(bad.sum()))


@pytest.fixture(scope="module")
def years_dev(inputs, params):
    """The records of the two scenario years, each a torch tensor [3][12][5][48][96] on the GPU."""
    import torch
    e = engine.Engine(inputs, params, n_members=NM)
    monthly, _ = e.run(YEARS, CO2)
    e.close()
    return [torch.from_numpy(np.ascontiguousarray(monthly[:, y])).cuda() for y in range(YEARS)]


def check_kind(inputs, params, make_plan, on_tensor, on_engine, names, label):
    """on_tensor(plan) and on_engine(engine, plan) of ONE plan against those of two fresh plans used once each; then the
    plan is closed and a new one works.  Returns the fresh plan's products of the tensor."""
    import torch
    shared, fresh_t, fresh_e = make_plan(), make_plan(), make_plan()
    ea, eb = (engine.Engine(inputs, params, n_members=NM) for _ in range(2))
    got_t = on_tensor(shared)             # the per-device entry is made here ...
    got_e = on_engine(ea, shared)         # ... and found here
    ref_t, ref_e = on_tensor(fresh_t), on_engine(eb, fresh_e)
    torch.cuda.synchronize()
    same_bits(got_t, ref_t, names, f"{label} _dev, shared plan")
    same_bits(got_e, ref_e, names + ("yearly",), f"{label} run, shared plan")
    for x in (shared, fresh_t, fresh_e, ea, eb):
        x.close()
    assert shared.h is None
    again = make_plan()
    got = on_tensor(again)
    torch.cuda.synchronize()
    same_bits(got, ref_t, names, f"{label} _dev, a new plan after close")
    return again, ref_t


def test_diag_plan_serves_tensor_then_engine(inputs, params, years_dev):
    import torch
    regions = {k: v for k, v in diag.standard_regions(inputs).items() if k in ("land", "ocean")}
    names = ("regions", "zonal", "annual")
    plan, ref3 = check_kind(inputs, params, lambda: diag.Plan(96, 48, regions), lambda p: diag.reduce_dev(p, years_dev[0]),
                            lambda e, p: e.run_diag(YEARS, CO2, p), names, "diag")
    # a larger member batch on the same plan: the partial sums' array regrows while nothing may still read the old one
    six = torch.cat([years_dev[0], years_dev[1]]).contiguous()
    got6 = diag.reduce_dev(plan, six)
    once = diag.Plan(96, 48, regions)
    ref6 = diag.reduce_dev(once, six)
    torch.cuda.synchronize()
    same_bits(got6, ref6, names, "diag _dev, 6 members after 3")
    for name in names:  # ... and its first three members are the three of before
        assert np.array_equal(getattr(got6, name)[:NM].cpu().numpy().view(np.uint32), getattr(ref3, name).cpu().numpy().view(np.uint32)), name
    plan.close(), once.close()


def test_clim_plan_serves_tensor_then_engine(inputs, params, years_dev):
    def on_tensor(p):
        for k, x in enumerate(years_dev):
            clim.add_year_dev(p, x, k)
        return clim.finish_dev(p, YEARS)
    plan, _ = check_kind(inputs, params, lambda: clim.Plan(96, 48, NM, control=[-1, 0, 0]), on_tensor,
                         lambda e, p: e.run_clim(YEARS, CO2, p, [(0, YEARS)]), clim.PRODUCTS, "clim")
    plan.close()


def test_ens_plan_serves_tensor_then_engine(inputs, params, years_dev):
    plan, _ = check_kind(inputs, params, lambda: ens.Plan(96, 48, NM, [0, 0, 0], control=[1, 1, 1], probs=(0.1, 0.5)),
                         lambda p: ens.reduce_dev(p, years_dev[0]), lambda e, p: e.run_ens(YEARS, CO2, p), ens.PRODUCTS, "ens")
    plan.close()


def test_refused_setters_leave_the_engine_alone(inputs, params):
    """set_member_experiments, set_forcing_tables and set_member_forcing, each refused with an argument error between two
    one-year runs: the second year is that of an engine that was never refused."""
    co2 = [c[:1] for c in CO2]
    ea, eb = (engine.Engine(inputs, params, n_members=NM) for _ in range(2))
    first_a, first_b = ea.run(1, co2), eb.run(1, co2)
    assert np.array_equal(first_a[0].view(np.uint32), first_b[0].view(np.uint32))
    refused = ((lambda: ea.set_member_experiments([0, 0x100, 0]), "unknown switch bits"),
               (lambda: ea.set_forcing_tables(np.full((1, 48, 96), 2.0, np.float32)), "not in [0, 1]"),
               (lambda: ea.set_member_forcing([{}, {"co2_pattern": 5}, {}]), "co2_pattern 5 is outside"))
    for call, words in refused:
        with pytest.raises(engine.GrebError) as ei:
            call()
        assert ei.value.code == -1 and words in str(ei.value), ei.value
    (mon_a, yr_a), (mon_b, yr_b) = ea.run(1, co2), eb.run(1, co2)
    bad = mon_a.view(np.uint32) != mon_b.view(np.uint32)
    print(f"second year after the refusals: {int(bad.sum())} of {bad.size} values differ from the untouched twin")
    assert not bad.any() and np.array_equal(yr_a.view(np.uint32), yr_b.view(np.uint32))
    for m in range(NM):
        assert np.array_equal(ea.state(m).view(np.uint32), eb.state(m).view(np.uint32)), m
    assert ea.describe()["forcing"] == eb.describe()["forcing"] and ea.describe()["member_switches"] == "uniform"
    ea.close(), eb.close()
