"""GPU: the crossing output (csrc/greb_cross.hip) against cross.reference, the numpy statement of its products.

Every comparison with the mirror is for EQUAL int32 values and EQUAL fp32 BITS: device and mirror perform the same IEEE
operations (for a season: fp64 multiply, add, divide and one conversion to fp32; for `rel`: one fp32 subtraction; then
comparisons) in the same order on the same fp32 data -- the kernels are built without contraction of a multiply into the
add behind it -- so there is nothing for a tolerance to cover.

The data: positive fp32 of physical magnitude, drawn anew for every year, so that at every point the years decide an
event differently.  Each event's threshold is the median of the mirror's own quantity over members, years and points; a
year then hits with probability one half, and with n years a (member, point) pair never hits, or always hits, with
probability 2^-n.  At 1 % of the elements the record is overwritten by the threshold itself (month selectors without
`rel`), so that q == thr is decided, in both directions.  classes() asserts the mix ON THE MIRROR, before any device call:
per event at least 1 % of the pairs never hit, 1 % always hit and -- from two years on: with one year `first` is 0 or -1
and `stay` equals it, whatever the data -- 1 % have first > 0 and 1 % have stay != first."""
import numpy as np
import pytest
import torch  # before the library is loaded (a plan loads it), as the other GPU tests import it at the top of each test:
              # the process then has ONE HIP runtime, the one torch brings

from greb_climate_model_amd import abi, budget, cross, engine

pytestmark = pytest.mark.gpu

LO = np.array([220.0, 220.0, 271.0, 1e-3, 0.05], np.float32)  # Tsurf, Tair, Tocean [K], q [kg/kg], albedo
HI = np.array([310.0, 300.0, 303.0, 2e-2, 0.80], np.float32)
CONTROL = [-1, 0, 0, 1, -1, 4, 6]
GROUP = [0, 1, 1, 2, -1, 2, 2]
MAPS = cross.PRODUCTS[:6]
E = cross.Event
C_ = cross
# (var, sel, dir, rel); var is taken modulo the variable count.  Sixteen events each; several share a variable and a selector.
SET_A = [(0, C_.ANN, +1, True), (0, C_.ANN, -1, True), (0, C_.ANN, +1, False), (4, C_.SEP, -1, False), (4, C_.SEP, +1, False),
         (1, C_.JAN, +1, False), (2, C_.FEB, -1, True), (3, C_.MAR, +1, False), (4, C_.APR, -1, False), (0, C_.MAY, +1, True),
         (1, C_.JUN, -1, False), (2, C_.DJF, +1, False), (3, C_.MAM, -1, True), (4, C_.JJA, +1, False), (1, C_.SON, -1, False),
         (2, C_.DEC, +1, True)]
SET_B = [(12, C_.JUL, +1, False), (3, C_.AUG, -1, False), (7, C_.OCT, +1, False), (7, C_.NOV, -1, False), (0, C_.ANN, -1, False),
         (12, C_.DJF, -1, False), (12, C_.JUL, -1, False), (5, C_.AUG, +1, False), (9, C_.SEP, +1, False), (10, C_.JAN, -1, False),
         (11, C_.MAM, +1, False), (6, C_.JJA, -1, False), (8, C_.SON, +1, False), (2, C_.DEC, -1, False), (7, C_.NOV, +1, False),
         (7, C_.OCT, -1, False)]
ONE = [(0, C_.ANN, +1, True)]


def test_the_event_sets_cover_what_they_should():
    both = SET_A + SET_B
    assert len(SET_A) == len(SET_B) == abi.CROSS_MAX_EVENTS
    assert {t[1] for t in both} == set(range(17)) and {t[2] for t in both} == {+1, -1} and {t[3] for t in both} == {True, False}
    for s in (SET_A, SET_B):
        keys = [(t[0], t[1]) for t in s]
        assert len(set(keys)) < len(keys), "several events share a variable and a selector"


def synth(years, n, nv, ny, nx, seed):
    """Strictly positive fp32 records of physical magnitude, [years][n][12][nv][ny][nx] (variable v as v % 5 of a state year)."""
    rng = np.random.default_rng(seed)
    x = rng.random((years, n, 12, nv, ny, nx), dtype=np.float32)
    v = np.arange(nv) % 5
    x *= (HI - LO)[v][:, None, None]
    x += LO[v][:, None, None]
    assert x.dtype == np.float32 and x.min() > 0
    return x


def shaped(template, x, control, seed=0):
    """The events of `template` with their thresholds, x being overwritten where q == thr is wanted (see the module's text).
    Without a member that has a control there is nothing a `rel` event could be decided on: it is taken as it is."""
    rng = np.random.default_rng(10_000 + seed)
    nv = x.shape[3]
    some_control = control is not None and any(c >= 0 for c in control)
    template = [(var % nv, sel, d, rel and some_control) for var, sel, d, rel in template]
    thr = {}
    for var, sel, d, rel in template:  # month selectors without `rel` first: their records are overwritten
        if sel < 12 and not rel and (var, sel, rel) not in thr:
            q = x[:, :, sel, var]  # a view
            t = np.float32(np.median(q))
            q[rng.random(q.shape) < 0.01] = t
            thr[(var, sel, rel)] = t
    for var, sel, d, rel in template:
        if (var, sel, rel) not in thr:
            q = np.stack([cross.quantity(xk, E(var, sel, 0.0, d, rel), control) for xk in x])
            thr[(var, sel, rel)] = np.float32(np.nanmedian(q))
    events = [E(var, sel, float(thr[(var, sel, rel)]), d, rel) for var, sel, d, rel in template]
    for ev in events:
        if ev.sel < 12 and not ev.rel:
            assert (x[:, :, ev.sel, ev.var] == np.float32(ev.thr)).mean() > 0.005, "q == thr is decided at 1 % of the elements"
    return events


def classes(ref, years, label):
    """The mix the module's text promises, on the mirror alone."""
    for e in range(ref.first.shape[1]):
        f, s, c = ref.first[:, e], ref.stay[:, e], ref.count[:, e]
        share = {"never": (f < 0).mean(), "always": (c == years).mean()}
        if years >= 2:
            share.update({"first > 0": (f > 0).mean(), "stay != first": (s != f).mean()})
        for k, v in share.items():
            assert v >= 0.01, (label, "event", e, k, float(v))


def same(got, ref, label, names=cross.PRODUCTS):
    for name in names:
        g, r = getattr(got, name), getattr(ref, name)
        assert (g is None) == (r is None), (label, name)
        if g is None:
            continue
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, (label, name, g.dtype, r.dtype, g.shape, r.shape)
        bad = g.view(np.uint32) != r.view(np.uint32)  # int32 values and fp32 bits alike (NaNs included)
        print(f"{label} {name}: {int(bad.sum())} of {bad.size} values differ")
        assert not bad.any(), (label, name, int(bad.sum()), g[bad][:4], r[bad][:4])


def on_device(plan, x):
    """The years x[0 ... ] through add_year_dev / finish_dev, back on the host."""
    frac = [cross.add_year_dev(plan, torch.from_numpy(np.ascontiguousarray(xk)).cuda(), k) for k, xk in enumerate(x)]
    res = cross.finish_dev(plan, len(x))
    torch.cuda.synchronize()
    maps = [None if getattr(res, n) is None else getattr(res, n).cpu().numpy() for n in MAPS]
    return cross.Result(*maps, None if frac[0] is None else np.stack([f.cpu().numpy() for f in frac]))


def pick(ref, what):
    """The mirror's products that `what` selects."""
    return cross.Result(*[getattr(ref, n) if on else None for n, on in zip(cross.PRODUCTS, cross.selected(what))])


def case(template, years, n, nv, ny, nx, seed, control=CONTROL, group=GROUP):
    control = None if control is None else list(control[:n])
    group = None if group is None else list(group[:n])
    x = synth(years, n, nv, ny, nx, seed)
    events = shaped(template, x, control, seed)
    return x, events, control, group, cross.reference(x, events, control, group)


# ---- the kernels against the mirror ----------------------------------------------------------------------------------
@pytest.mark.parametrize("years", [1, 2, 5])
@pytest.mark.parametrize("nx,ny,n", [(96, 48, 1), (96, 48, 3), (96, 48, 7), (100, 37, 1), (100, 37, 3), (100, 37, 7), (384, 192, 2)])
def test_products_against_the_mirror(nx, ny, n, years):
    """Sixteen events on five variables, a control map, groups, all six products."""
    x, events, control, group, ref = case(SET_A, years, n, 5, ny, nx, seed=nx + n + years)
    classes(ref, years, (nx, ny, n, years))
    plan = cross.Plan(nx, ny, n, events, control=control, group=group)
    assert plan.what == cross.ALL
    same(on_device(plan, x), ref, f"{nx}x{ny} n={n} years={years}")
    plan.close()


@pytest.mark.parametrize("nv,template,control", [(1, SET_B, None), (13, SET_B, None), (5, ONE, CONTROL), (13, ONE, None), (1, SET_A, CONTROL)])
def test_variable_counts_and_event_counts(nv, template, control):
    """1, 5 and 13 variables; 1 event and 16; with a control map and without one (and then without groups)."""
    nx, ny, n, years = 100, 37, 3, 2
    x, events, control, group, ref = case(template, years, n, nv, ny, nx, seed=nv + len(template), control=control,
                                          group=GROUP if control else None)
    classes(ref, years, (nv, len(template)))
    plan = cross.Plan(nx, ny, n, events, n_vars=nv, control=control, group=group)
    same(on_device(plan, x), ref, f"n_vars={nv}, {len(events)} events")
    plan.close()


def test_each_product_alone_gives_the_numbers_of_the_full_call():
    """Only the state words a product needs exist; the unselected pointers are NULL."""
    nx, ny, n, years = 100, 37, 3, 3
    x, events, control, group, ref = case(SET_A, years, n, 5, ny, nx, seed=21)
    classes(ref, years, "alone")
    for what in (abi.T_FIRST, abi.T_LAST, abi.T_STAY, abi.T_COUNT, abi.T_PEAK, abi.T_FRACTION, abi.T_STAY | abi.T_PEAK, cross.ALL):
        plan = cross.Plan(nx, ny, n, events, control=control, group=group, what=what)
        got = on_device(plan, x)
        assert [getattr(got, k) is not None for k in cross.PRODUCTS] == list(cross.selected(what)), what
        same(got, pick(ref, what), f"what={what}")
        plan.close()


def test_fraction_of_groups_of_one_two_and_five_members():
    """Nine members: groups of 1, 2 and 5, one member in none; two members are their own control (q = +0 throughout)."""
    nx, ny, n, years = 96, 48, 9, 3
    control, group = [0, 0, 0, 1, -1, 4, 6, 2, 8], [0, 2, 1, 2, 2, 1, 2, 2, -1]
    x, events, control, group, ref = case(SET_A, years, n, 5, ny, nx, seed=33, control=control, group=group)
    assert ref.fraction.shape == (years, 3, 16, ny, nx)
    for g, size in enumerate((1, 2, 5)):
        levels = np.unique(ref.fraction[:, g])
        assert set(levels) == {np.float32(np.float64(c) / np.float64(size)) for c in range(size + 1)}, (g, levels)
    own = ref.peak[[0, 8]][:, [0, 1]]  # the ANN response of a member that is its own control
    assert not own.any() and not np.signbit(own).any()
    plan = cross.Plan(nx, ny, n, events, control=control, group=group)
    same(on_device(plan, x), ref, "nine members")
    only = cross.Plan(nx, ny, n, events, control=control, group=group, what=abi.T_FRACTION)
    same(on_device(only, x), pick(ref, abi.T_FRACTION), "FRACTION alone")
    plan.close(); only.close()


def test_a_plan_is_reused_without_clearing():
    """Three years, finish, then two years of other data: what a fresh plan gives (year 0 stores the state)."""
    nx, ny, n = 100, 37, 3
    x, events, control, group, ref = case(SET_A, 3, n, 5, ny, nx, seed=41)
    y = synth(2, n, 5, ny, nx, seed=42)
    plan, fresh = (cross.Plan(nx, ny, n, events, control=control, group=group) for _ in range(2))
    same(on_device(plan, x), ref, "first period")
    again = on_device(plan, y)
    same(again, cross.reference(y, events, control, group), "second period against the mirror")
    same(again, on_device(fresh, y), "second period against a fresh plan")
    with pytest.raises(engine.GrebError) as ei:  # the years go in order
        cross.add_year_dev(plan, torch.from_numpy(y[0]).cuda(), 1)
    assert "k = 1, but 0 years" in str(ei.value)
    plan.close(); fresh.close()


def test_deterministic_and_independent_of_the_batch():
    """The same call twice gives the same bits; strangers appended to the batch, or standing between its members, do not
    change a member's maps."""
    nx, ny, n, years = 100, 37, 7, 3
    x, events, control, group, ref = case(SET_A, years, n, 5, ny, nx, seed=51)
    plan = cross.Plan(nx, ny, n, events, control=control, what=cross.MAPS)
    alone = on_device(plan, x)
    same(alone, pick(ref, cross.MAPS), "alone")
    same(on_device(plan, x), alone, "the same call again")
    more = synth(years, 4, 5, ny, nx, seed=52) * np.float32(1.5)
    x_app = np.concatenate([x, more], axis=1)
    app = cross.Plan(nx, ny, n + 4, events, control=control + [-1, 7, 8, 0], what=cross.MAPS)
    got = on_device(app, x_app)
    same(cross.Result(*[getattr(got, k)[:n] for k in MAPS]), alone, "appended", MAPS)
    at = [0, 7, 1, 2, 8, 3, 4, 9, 5, 10, 6]  # the plan's members in their order, strangers between them
    where = {m: i for i, m in enumerate(at)}
    ctl_all = control + [-1, 7, 8, 0]
    mix = cross.Plan(nx, ny, n + 4, events, control=[where[ctl_all[m]] if ctl_all[m] >= 0 else -1 for m in at], what=cross.MAPS)
    got = on_device(mix, np.ascontiguousarray(x_app[:, at]))
    rows = [where[m] for m in range(n)]
    same(cross.Result(*[getattr(got, k)[rows] for k in MAPS]), alone, "interleaved", MAPS)
    for p in (plan, app, mix):
        p.close()


def test_a_nan_in_one_member_stays_in_that_member():
    """Member 5 is nobody's control: a NaN in its records changes its own maps only, and where it lies it is a miss."""
    nx, ny, n, years = 100, 37, 7, 3
    x, events, control, group, ref = case(SET_A, years, n, 5, ny, nx, seed=61)
    x[1, 5, :, :, 7, 11] = np.nan  # year 1, every month and variable of one point
    plan = cross.Plan(nx, ny, n, events, control=control, what=cross.MAPS)
    got = on_device(plan, x)
    others = [m for m in range(n) if m != 5]
    same(cross.Result(*[getattr(got, k)[others] for k in MAPS]), cross.Result(*[getattr(ref, k)[others] for k in MAPS]), "the others", MAPS)
    same(got, pick(cross.reference(x, events, control), cross.MAPS), "with the NaN")
    assert not np.isnan(got.peak[5, :, 7, 11]).any() and (got.peak_year[5, :, 7, 11] != 1).all()  # years 0 and 2 are numbers
    assert (got.count[5, :, 7, 11] <= 2).all()
    plan.close()


def test_the_events_come_back_in_the_callers_order():
    nx, ny, n, years = 96, 48, 3, 2
    x, events, control, group, ref = case(SET_A, years, n, 5, ny, nx, seed=71)
    order = np.random.default_rng(72).permutation(len(events))
    plan = cross.Plan(nx, ny, n, [events[i] for i in order], control=control, group=group)
    got = on_device(plan, x)
    want = cross.Result(*[getattr(ref, k)[:, order] for k in MAPS], ref.fraction[:, :, order])
    same(got, want, "permuted events")
    plan.close()


# ---- run_cross on a real engine --------------------------------------------------------------------------------------
CONTROL4 = [-1, 0, 0, 0]
CO2_4x3 = np.asarray([[340.0, 340.0, 340.0], [680.0, 680.0, 680.0], [400.0, 560.0, 800.0], [340.0, 500.0, 1000.0]], np.float32)


def _engines(inputs, params, n):
    es = [engine.Engine(inputs, params, n_members=4) for _ in range(n)]
    for e in es:
        e.flux_correction(1)
    return es


def _same_engine_state(a, b, yr_a, yr_b):
    assert np.array_equal(yr_a, yr_b), "yearly differs"
    for m in range(a.nm):
        assert np.array_equal(a.state(m), b.state(m)), f"state of member {m} differs"


def _thresholds(template, x, control):
    """Per event the quantile (of the mirror's q over members, years and points) at which the mirror's FIRST holds -1 and the
    most different years: the events are decided by the run itself, not by the choice of the number."""
    events = []
    for var, sel, d, rel in template:
        q = np.stack([cross.quantity(xk, E(var, sel, 0.0, d, rel), control) for xk in x])
        best = None
        for p in (50, 40, 60, 30, 70, 20, 80):
            ev = E(var, sel, float(np.float32(np.nanpercentile(q, p))), d, rel)
            first = np.unique(cross.reference(x, [ev], control).first)
            if best is None or len(first) > best[0]:
                best = (len(first), ev)
        events.append(best[1])
    return events


RUN_EVENTS = [(0, C_.ANN, +1, True), (0, C_.ANN, +1, True), (4, C_.SEP, -1, False), (1, C_.JUL, +1, True), (3, C_.DJF, +1, False)]


def test_run_cross_against_run(inputs, params):
    """Twin engines: three years in one call against the mirror of run()'s records, then two and one with two plans on a
    third engine (each call's years count from 0)."""
    ea, eb, ec = _engines(inputs, params, 3)
    nx, ny = inputs.nx, inputs.ny
    mon, yr_a = ea.run(3, CO2_4x3)
    x = np.ascontiguousarray(np.moveaxis(mon, 1, 0))  # [years][member]...
    events = _thresholds(RUN_EVENTS, x, CONTROL4)
    events[1] = E(0, C_.ANN, events[0].thr * 1.5, +1, True)  # a second level of the same quantity
    group = [-1, 0, 0, 0]
    ref = cross.reference(x, events, CONTROL4, group)
    for e in range(len(events)):
        first = set(np.unique(ref.first[:, e]).tolist())
        assert -1 in first and len(first - {-1}) >= 2, (e, events[e], sorted(first))
    family = eb.describe()["kernel_family"]
    plan = cross.Plan(nx, ny, 4, events, control=CONTROL4, group=group)
    res = eb.run_cross(3, CO2_4x3, plan)
    assert res.vars == budget.STATE_NAMES and res.fraction.shape == (3, 1, len(events), ny, nx)
    same(res, ref, "run_cross, three years")
    assert eb.describe()["kernel_family"] == family == ea.describe()["kernel_family"]
    _same_engine_state(ea, eb, yr_a, res.yearly)
    maps = cross.Plan(nx, ny, 4, events, control=CONTROL4, what=cross.MAPS)  # no FRACTION: nothing leaves before the end
    r0, r1 = ec.run_cross(2, CO2_4x3[:, :2], plan), ec.run_cross(1, CO2_4x3[:, 2:], maps)
    same(r0, cross.reference(x[:2], events, CONTROL4, group), "2 + 1 years, first call")
    same(r1, pick(cross.reference(x[2:], events, CONTROL4), cross.MAPS), "2 + 1 years, second call")
    _same_engine_state(eb, ec, res.yearly[:, 2:], r1.yearly)
    again = ec.run_cross(1, 500.0, plan)  # the plan serves another period, on another engine state
    mon4, yr4 = ea.run(1, 500.0)
    same(again, cross.reference(np.moveaxis(mon4, 1, 0), events, CONTROL4, group), "the plan again")
    _same_engine_state(ea, ec, yr4, again.yearly)
    for o in (ea, eb, ec, plan, maps):
        o.close()


def test_run_cross_of_a_budget_combination_against_run_budget(inputs, params):
    """records = the surface net flux: against the mirror of run_budget's records, combined by budget.combine_reference."""
    ea, eb = _engines(inputs, params, 2)
    nx, ny = inputs.nx, inputs.ny
    cb = budget.combo({"surface_net": budget.SURFACE_NET})
    _, bud, yr_a = ea.run_budget(3, CO2_4x3, want_monthly=False)
    x = np.ascontiguousarray(np.moveaxis(budget.combine_reference(cb, bud), 1, 0))  # [3][4][12][1][ny][nx]
    events = _thresholds([(0, C_.ANN, +1, True), (0, C_.JUL, -1, False), (0, C_.DJF, +1, True)], x, CONTROL4)
    group = [0, 0, 1, 1]
    ref = cross.reference(x, events, CONTROL4, group)
    assert len(np.unique(ref.first)) >= 3
    plan = cross.Plan(nx, ny, 4, events, n_vars=1, control=CONTROL4, group=group)
    res = eb.run_cross(3, CO2_4x3, plan, records=cb)
    assert res.vars == ("surface_net",)
    same(res, ref, "run_cross of the surface net flux")
    _same_engine_state(ea, eb, yr_a, res.yearly)
    with pytest.raises(engine.GrebError) as ei:  # the plan of one variable does not fit the state records
        eb.run_cross(1, CO2_4x3[:, :1], plan)
    assert ei.value.code == -1 and "n_vars = 1" in str(ei.value) and "5 variables" in str(ei.value), ei.value
    for o in (ea, eb, plan):
        o.close()


def test_refused_calls_leave_the_engine_alone(inputs, params):
    ea, eb = _engines(inputs, params, 2)
    events = [E(0, C_.ANN, 0.5, +1, True), E(4, C_.SEP, 0.4, -1)]
    plan = cross.Plan(96, 48, 4, events, control=CONTROL4, group=[0, 0, 0, -1])
    other_grid, other_members = cross.Plan(100, 37, 4, events, control=CONTROL4), cross.Plan(96, 48, 5, events, control=CONTROL4 + [0])
    other_vars = cross.Plan(96, 48, 4, events, n_vars=6, control=CONTROL4)
    for bad, words in ((other_grid, ("100 x 37", "96 x 48")), (other_members, ("5 members", "has 4")),
                       (other_vars, ("n_vars = 6", "5 variables"))):
        with pytest.raises(engine.GrebError) as ei:
            ea.run_cross(2, CO2_4x3[:, :2], bad)
        assert ei.value.code == -1 and all(w in str(ei.value) for w in words), ei.value
    yearly = np.zeros((4, 2, 2), np.float32)
    co2 = np.ascontiguousarray(CO2_4x3[:, :2])
    assert engine.lib().greb_engine_run_cross(ea.h, 2, abi.fptr(co2), plan.h, *[None] * 7, abi.fptr(yearly)) == -1
    assert "run_cross: GREB_T_FIRST selected but `first` is NULL" in engine.lib().greb_engine_last_error(ea.h).decode()
    ra, rb = ea.run_cross(2, co2, plan), eb.run_cross(2, co2, plan)  # ... bit-identical to an untouched twin
    same(ra, rb, "after the refusals")
    _same_engine_state(ea, eb, ra.yearly, rb.yearly)
    for o in (ea, eb, other_grid, other_members, other_vars, plan):
        o.close()
