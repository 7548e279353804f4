"""GPU: the regression output (csrc/greb_reg.hip) against regress.reference, the numpy statement of its products.

Every comparison with the mirror is for EQUAL fp32 BITS and EQUAL NaN POSITIONS: device and mirror perform the same IEEE
operations in the same order on the same fp32 data -- the kernels are built without contraction of a multiply into the
add behind it -- so there is nothing for a tolerance to cover.  The mirror is fed the regional means diag.reduce_dev makes
over the same weights (the plan's index pass is that device code), and the INDEX it forms from them by the contract's
formula is what the device's INDEX is held to.

The data: positive fp32 of physical magnitude, drawn anew for every year.  At 1 % of the points every member keeps year
0's records over the years (a constant y: slope +0, R2 NaN).  From three members on, the last member is constant
throughout -- an index of its own records is constant: all NaN -- and one member has no control (with three members that
is the same member, so that more than half of every term's elements stay finite; with seven they are two members, and a
third is its own control: a zero series).  classes() asserts the mix ON THE MIRROR, before any device call."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded (a plan loads it), as the other GPU tests import it: the process then has ONE
              # HIP runtime, the one torch brings

from greb_climate_model_amd import abi, budget, cross, diag, engine, regress

pytestmark = pytest.mark.gpu

LO = np.array([220.0, 220.0, 271.0, 1e-3, 0.05], np.float32)  # Tsurf, Tair, Tocean [K], q [kg/kg], albedo
HI = np.array([310.0, 300.0, 303.0, 2e-2, 0.80], np.float32)
MAPS = regress.PRODUCTS[:3]
C_ = cross
# (var, sel, region, rel) and (var, sel, index, rel); var is spread over the variable count by spread()
INDICES8 = [(0, C_.ANN, 0, True), (0, C_.ANN, 0, False), (1, C_.DJF, 1, False), (2, C_.JUL, 2, True), (3, C_.OCT, 1, False),
            (4, C_.NOV, 0, False), (0, C_.JJA, 2, True), (1, C_.DEC, 0, False)]
TERMS16 = [(0, C_.ANN, 0, True), (0, C_.ANN, 1, False), (0, C_.ANN, 1, True), (4, C_.SEP, 0, True), (4, C_.SEP, 5, False),
           (1, C_.JAN, 2, False), (2, C_.FEB, 3, True), (3, C_.MAR, 4, False), (4, C_.APR, 5, False), (0, C_.MAY, 6, True),
           (1, C_.JUN, 7, False), (2, C_.DJF, 0, False), (3, C_.MAM, 1, True), (4, C_.JJA, 2, False), (1, C_.SON, 3, False),
           (2, C_.AUG, 4, True)]
INDEX1, TERM1 = [(0, C_.ANN, 0, True)], [(0, C_.ANN, 0, True)]
CONTROLS = {1: None, 2: [1, 0], 3: [1, 0, -1], 7: [-1, 0, 0, 1, 2, 5, 4]}


def test_the_sets_cover_what_they_should():
    assert len(INDICES8) == abi.REG_MAX_INDICES and len(TERMS16) == abi.REG_MAX_TERMS
    assert {t[1] for t in INDICES8 + TERMS16} == set(range(17))
    for s in (INDICES8, TERMS16):
        assert {t[3] for t in s} == {True, False}
    assert {t[2] for t in INDICES8} == {0, 1, 2} and {t[2] for t in TERMS16} == set(range(8))
    keys = [(t[0], t[1]) for t in TERMS16]
    assert len(set(keys)) < len(keys), "several terms share a variable and a selector"


def spread(var, nv):
    return (var * 5 + 2) % nv if nv > 5 else var % nv


def synth(years, n, nv, ny, nx, seed, shape_members=True):
    """Strictly positive fp32 records of physical magnitude, [years][n][12][nv][ny][nx] (variable v as v % 5 of a state year),
    with the constant points and the constant member of the module's text."""
    rng = np.random.default_rng(seed)
    x = rng.random((years, n, 12, nv, ny, nx), dtype=np.float32)
    v = np.arange(nv) % 5
    x *= (HI - LO)[v][:, None, None]
    x += LO[v][:, None, None]
    still = rng.random((ny, nx)) < 0.01
    x[1:, ..., still] = x[:1, ..., still]
    if shape_members and n >= 3:
        x[1:, n - 1] = x[:1, n - 1]
    assert x.dtype == np.float32 and x.min() > 0
    return x, still


def weights(ny, nx, seed):
    rng = np.random.default_rng(1000 + seed)
    lat = np.broadcast_to(diag.latitudes(ny)[:, None], (ny, nx))
    return {"north": np.ascontiguousarray(lat > 20, np.float32), "any": rng.random((ny, nx)).astype(np.float32)}


def device_regions(nx, ny, nv, w, x):
    """The fp32 regional means of every year as diag.reduce_dev makes them over the weights w: [years][n][12][nv][1 + len(w)]."""
    plan = diag.Plan(nx, ny, w, n_vars=nv)
    out = [diag.reduce_dev(plan, torch.tensor(xk).cuda(), abi.D_REGIONS).regions for xk in x]
    torch.cuda.synchronize()
    out = np.stack([r.cpu().numpy() for r in out])
    plan.close()
    return out


def classes(ref, years, n, still, indices, terms, control, label):
    """The mix the module's text promises, on the mirror alone."""
    if years < 2:
        assert all(np.isnan(getattr(ref, k)).all() for k in MAPS), (label, "one year: nothing to fit")
        return
    for t in range(ref.slope.shape[1]):
        s, r2 = ref.slope[:, t], ref.r2[:, t]
        assert np.isfinite(s).mean() >= 0.5, (label, "term", t, "finite", float(np.isfinite(s).mean()))
        assert (s > 0).any() and (s < 0).any(), (label, "term", t, "slopes of both signs")
        flat = np.isfinite(s) & np.isnan(r2)  # a constant y under an index that varies
        assert flat.any() and (s[flat] == 0).all() and not np.signbit(s[flat]).any(), (label, "term", t, "constant y")
        assert still.any() and flat[:, still].any()
        if n >= 3 and not indices[terms[t].index].rel:
            assert np.isnan(s[n - 1]).all(), (label, "term", t, "the constant member")
    plain = [j for j, ix in enumerate(indices) if not ix.rel]
    if n >= 3 and plain:
        assert (ref.index[n - 1][:, plain] == ref.index[n - 1][0, plain]).all(), (label, "the constant member's index")
    if control is not None and -1 in control and len(plain) < len(indices):
        none = control.index(-1)
        assert np.isnan(ref.index[none]).any() and not np.isnan(np.delete(ref.index, none, axis=0)).any(), (label, "no control")
        assert all(np.isnan(ref.slope[none, t]).all() for t, tm in enumerate(terms) if tm.rel), (label, "no control")
    if control is not None and n == 7:  # member 5 is its own control: +0 throughout
        assert not ref.index[5][:, [j for j in range(len(indices)) if j not in plain]].any(), (label, "own control")


def same(got, ref, label, names=regress.PRODUCTS):
    for name in names:
        g, r = getattr(got, name), getattr(ref, name)
        assert (g is None) == (r is None), (label, name)
        if g is None:
            continue
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.dtype == r.dtype == np.float32 and g.shape == r.shape, (label, name, g.dtype, r.dtype, g.shape, r.shape)
        gn, rn = np.isnan(g), np.isnan(r)
        bad = (gn != rn) | (~gn & ~rn & (g.view(np.uint32) != r.view(np.uint32)))
        print(f"{label} {name}: {int(bad.sum())} of {bad.size} values differ, {int(rn.sum())} NaN")
        assert not bad.any(), (label, name, int(bad.sum()), g[bad][:4], r[bad][:4])


def on_device(plan, x):
    """The years x[0 ... ] through add_year_dev / finish_dev, back on the host."""
    index = [regress.add_year_dev(plan, torch.tensor(xk).cuda(), k) for k, xk in enumerate(x)]
    res = regress.finish_dev(plan, len(x))
    torch.cuda.synchronize()
    maps = [None if getattr(res, n) is None else getattr(res, n).cpu().numpy() for n in MAPS]
    return regress.Result(*maps, None if index[0] is None else np.stack([i.cpu().numpy() for i in index], axis=1))


def pick(ref, what):
    """The mirror's products that `what` selects."""
    return regress.Result(*[getattr(ref, n) if on else None for n, on in zip(regress.PRODUCTS, regress.selected(what))])


def shaped(indices, terms, nv, control):
    """The templates as Index and Term lists; without a member that has a control, `rel` is dropped."""
    some = control is not None and any(c >= 0 for c in control)
    return ([regress.Index(spread(v, nv), s, r, rel and some) for v, s, r, rel in indices],
            [regress.Term(spread(v, nv), s, i, rel and some) for v, s, i, rel in terms])


@functools.lru_cache(maxsize=2)
def _case(key, years, n, nv, ny, nx, seed, with_control):
    indices, terms = {"full": (INDICES8, TERMS16), "one": (INDEX1, TERM1)}[key]
    control = CONTROLS[n] if with_control else None
    x, still = synth(years, n, nv, ny, nx, seed)
    w = weights(ny, nx, seed)
    indices, terms = shaped(indices, terms, nv, control)
    reg = device_regions(nx, ny, nv, w, x)
    ref = regress.reference(x, indices, terms, control, regions=reg)
    for a in (x, reg, ref.slope, ref.intercept, ref.r2, ref.index):
        a.setflags(write=False)  # shared among the tests: left unchanged
    classes(ref, years, n, still, indices, terms, control, (key, years, n, nv, ny, nx))
    return x, w, indices, terms, control, ref


def case(key, years, n, nv, ny, nx, seed, with_control=True):
    return _case(key, years, n, nv, ny, nx, seed, with_control)


def make(nx, ny, n, indices, terms, w, nv=5, control=None, what=None):
    return regress.Plan(nx, ny, n, indices, terms, regions=w, n_vars=nv, control=control, what=what)


# ---- the kernels against the mirror ----------------------------------------------------------------------------------
@pytest.mark.parametrize("years", [1, 2, 5])
@pytest.mark.parametrize("nx,ny,n", [(96, 48, 1), (96, 48, 3), (96, 48, 7), (100, 37, 1), (100, 37, 3), (100, 37, 7), (384, 192, 1),
                                     (384, 192, 2)])
def test_products_against_the_mirror(nx, ny, n, years):
    """Sixteen terms on eight indices over five variables and three regions, a control map, all four products."""
    x, w, indices, terms, control, ref = case("full", years, n, 5, ny, nx, seed=nx + n + years)
    plan = make(nx, ny, n, indices, terms, w, control=control)
    assert plan.what == regress.ALL
    same(on_device(plan, x), ref, f"{nx}x{ny} n={n} years={years}")
    plan.close()


@pytest.mark.parametrize("nv,key,with_control", [(1, "full", False), (13, "full", False), (5, "one", True), (13, "one", False),
                                                 (1, "full", True), (13, "full", True)])
def test_variable_counts_and_term_counts(nv, key, with_control):
    """1, 5 and 13 variables; one term on one index and 16 on 8; with a control map and without one."""
    nx, ny, n, years = 100, 37, 3, 2
    x, w, indices, terms, control, ref = case(key, years, n, nv, ny, nx, seed=nv + len(key), with_control=with_control)
    plan = make(nx, ny, n, indices, terms, w, nv=nv, control=control)
    same(on_device(plan, x), ref, f"n_vars={nv}, {len(terms)} terms, control={with_control}")
    plan.close()


def test_each_product_alone_gives_the_numbers_of_the_full_call():
    """Syy exists only with R2; the unselected pointers are NULL."""
    nx, ny, n, years = 100, 37, 3, 3
    x, w, indices, terms, control, ref = case("full", years, n, 5, ny, nx, seed=21)
    for what in (abi.R_SLOPE, abi.R_INTERCEPT, abi.R_R2, abi.R_INDEX, abi.R_SLOPE | abi.R_INDEX, regress.MAPS):
        plan = make(nx, ny, n, indices, terms, w, control=control, what=what)
        got = on_device(plan, x)
        assert [getattr(got, k) is not None for k in regress.PRODUCTS] == list(regress.selected(what)), what
        same(got, pick(ref, what), f"what={what}")
        plan.close()


def test_a_plan_is_reused_without_clearing():
    """Three years, finish, then two years of other data: what a fresh plan gives (year 0 stores the state)."""
    nx, ny, n = 100, 37, 3
    x, w, indices, terms, control, ref = case("full", 3, n, 5, ny, nx, seed=41)
    y, _ = synth(2, n, 5, ny, nx, seed=42)
    plan, fresh = (make(nx, ny, n, indices, terms, w, control=control) for _ in range(2))
    same(on_device(plan, x), ref, "first period")
    again = on_device(plan, y)
    same(again, regress.reference(y, indices, terms, control, regions=device_regions(nx, ny, 5, w, y)), "second period against the mirror")
    same(again, on_device(fresh, y), "second period against a fresh plan")
    with pytest.raises(engine.GrebError) as ei:  # the years go in order
        regress.add_year_dev(plan, torch.tensor(y[0]).cuda(), 1)
    assert "k = 1, but 0 years" in str(ei.value)
    plan.close(); fresh.close()


def test_deterministic_and_independent_of_the_batch():
    """The same call twice gives the same bits; strangers appended to the batch, or standing between its members, do not
    change a member's numbers."""
    nx, ny, n, years = 100, 37, 7, 3
    x, w, indices, terms, control, ref = case("full", years, n, 5, ny, nx, seed=51)
    plan = make(nx, ny, n, indices, terms, w, control=control)
    alone = on_device(plan, x)
    same(alone, ref, "alone")
    same(on_device(plan, x), alone, "the same call again")
    more, _ = synth(years, 4, 5, ny, nx, seed=52, shape_members=False)
    x_app = np.concatenate([x, more * np.float32(1.5)], axis=1)
    ctl_all = control + [-1, 7, 8, 0]
    app = make(nx, ny, n + 4, indices, terms, w, control=ctl_all)
    got = on_device(app, x_app)
    same(regress.Result(*[getattr(got, k)[:n] for k in regress.PRODUCTS]), alone, "appended")
    at = [0, 7, 1, 2, 8, 3, 4, 9, 5, 10, 6]  # the plan's members in their order, strangers between them
    where = {m: i for i, m in enumerate(at)}
    mix = make(nx, ny, n + 4, indices, terms, w, control=[where[ctl_all[m]] if ctl_all[m] >= 0 else -1 for m in at])
    got = on_device(mix, np.ascontiguousarray(x_app[:, at]))
    rows = [where[m] for m in range(n)]
    same(regress.Result(*[getattr(got, k)[rows] for k in regress.PRODUCTS]), alone, "interleaved")
    for p in (plan, app, mix):
        p.close()


def test_a_nan_year_poisons_its_element_only():
    """A NaN in one year of variable 0 at one point of member 2, which is nobody's control; the index is of variable 1."""
    nx, ny, n, years = 100, 37, 3, 3
    x, _ = synth(years, n, 2, ny, nx, seed=61, shape_members=False)
    w, control = weights(ny, nx, 61), [1, 0, 0]
    indices = [regress.Index(1, C_.JAN, 2), regress.Index(1, C_.ANN, 0, True)]
    terms = [regress.Term(0, C_.JAN, 0), regress.Term(0, C_.ANN, 1, True), regress.Term(1, C_.MAM, 0)]
    reg = device_regions(nx, ny, 2, w, x)
    clean = regress.reference(x, indices, terms, control, regions=reg)
    assert not np.isnan(clean.slope).any()
    x[1, 2, :, 0, 7, 11] = np.nan
    ref = regress.reference(x, indices, terms, control, regions=device_regions(nx, ny, 2, w, x))
    assert np.isnan(ref.slope).sum() == 2 and np.isnan(ref.slope[2, :2, 7, 11]).all() and not np.isnan(ref.index).any()
    plan = make(nx, ny, n, indices, terms, w, nv=2, control=control)
    same(on_device(plan, x), ref, "with the NaN")
    plan.close()


def test_the_terms_come_back_in_the_callers_order():
    nx, ny, n, years = 96, 48, 3, 2
    x, w, indices, terms, control, ref = case("full", years, n, 5, ny, nx, seed=71)
    rng = np.random.default_rng(72)
    order, iorder = rng.permutation(len(terms)), rng.permutation(len(indices))
    new_at = {int(old): new for new, old in enumerate(iorder)}
    t2 = [regress.Term(terms[i].var, terms[i].sel, new_at[terms[i].index], terms[i].rel) for i in order]
    plan = make(nx, ny, n, [indices[j] for j in iorder], t2, w, control=control)
    got = on_device(plan, x)
    want = regress.Result(*[getattr(ref, k)[:, order] for k in MAPS], ref.index[:, :, iorder])
    same(got, want, "permuted terms and indices")
    plan.close()


# ---- run_reg on a real engine ----------------------------------------------------------------------------------------
CONTROL4 = [-1, 0, 0, 0]
CO2_4x3 = np.asarray([[340.0, 340.0, 340.0], [680.0, 680.0, 680.0], [400.0, 560.0, 800.0], [340.0, 500.0, 1000.0]], np.float32)
RUN_INDICES = [regress.Index(0, C_.ANN, 0, True), regress.Index(1, C_.JJA, 1)]  # region 1: "north"
RUN_TERMS = [regress.Term(0, C_.ANN, 0, True), regress.Term(4, C_.SEP, 0, True), regress.Term(3, C_.ANN, 0, True),
             regress.Term(0, C_.DJF, 1), regress.Term(1, C_.JUL, 1, True)]


def _engines(inputs, params, n):
    es = [engine.Engine(inputs, params, n_members=4) for _ in range(n)]
    for e in es:
        e.flux_correction(1)
    return es


def _same_engine_state(a, b, yr_a, yr_b):
    assert np.array_equal(yr_a, yr_b), "yearly differs"
    for m in range(a.nm):
        assert np.array_equal(a.state(m), b.state(m)), f"state of member {m} differs"


def test_run_reg_against_run(inputs, params):
    """Twin engines: three years in one call against the mirror of run()'s records (fed diag.reduce_dev of those years),
    then the plan again for another period on another engine state."""
    ea, eb = _engines(inputs, params, 2)
    nx, ny = inputs.nx, inputs.ny
    w = {"north": weights(ny, nx, 0)["north"]}
    mon, yr_a = ea.run(3, CO2_4x3)
    x = np.ascontiguousarray(np.moveaxis(mon, 1, 0))  # [years][member]...
    ref = regress.reference(x, RUN_INDICES, RUN_TERMS, CONTROL4, regions=device_regions(nx, ny, 5, w, x))
    assert np.isnan(ref.slope[0, :3]).all() and np.isfinite(ref.slope[1:]).mean() > 0.9  # member 0 has no control
    assert (ref.slope[1:, 0] > 0).mean() > 0.9  # the local warming per degree of the global one
    family = eb.describe()["kernel_family"]
    plan = make(nx, ny, 4, RUN_INDICES, RUN_TERMS, w, control=CONTROL4)
    res = eb.run_reg(3, CO2_4x3, plan)
    assert res.vars == budget.STATE_NAMES and res.index.shape == (4, 3, 2)
    same(res, ref, "run_reg, three years")
    assert eb.describe()["kernel_family"] == family == ea.describe()["kernel_family"]
    _same_engine_state(ea, eb, yr_a, res.yearly)
    co2 = np.ascontiguousarray(CO2_4x3[:, ::-1])
    again = eb.run_reg(2, co2[:, :2], plan)  # the plan serves another period, on another engine state
    mon2, yr2 = ea.run(2, co2[:, :2])
    x2 = np.ascontiguousarray(np.moveaxis(mon2, 1, 0))
    same(again, regress.reference(x2, RUN_INDICES, RUN_TERMS, CONTROL4, regions=device_regions(nx, ny, 5, w, x2)), "the plan again")
    _same_engine_state(ea, eb, yr2, again.yearly)
    only = make(nx, ny, 4, RUN_INDICES, RUN_TERMS, w, control=CONTROL4, what=abi.R_SLOPE)  # one map, no INDEX series
    r1 = eb.run_reg(1, 500.0, only)
    assert r1.intercept is None and r1.index is None and np.isnan(r1.slope).all()  # one year: nothing to fit
    series = make(nx, ny, 4, RUN_INDICES, RUN_TERMS, w, control=CONTROL4, what=abi.R_INDEX)  # the INDEX series alone
    ea.run(1, 500.0)  # (the twin follows the call above); then three more years on both
    rs = eb.run_reg(3, CO2_4x3, series)
    mon3, yr3 = ea.run(3, CO2_4x3)
    x3 = np.ascontiguousarray(np.moveaxis(mon3, 1, 0))
    ref3 = regress.reference(x3, RUN_INDICES, RUN_TERMS, CONTROL4, regions=device_regions(nx, ny, 5, w, x3))
    assert rs.slope is None and rs.intercept is None and rs.r2 is None
    same(rs, pick(ref3, abi.R_INDEX), "run_reg, INDEX alone")
    _same_engine_state(ea, eb, yr3, rs.yearly)
    for o in (ea, eb, plan, only, series):
        o.close()


def test_run_reg_of_a_budget_combination_against_run_budget(inputs, params):
    """records = the surface net flux: against the mirror of run_budget's records, combined by budget.combine_reference."""
    ea, eb = _engines(inputs, params, 2)
    nx, ny = inputs.nx, inputs.ny
    cb = budget.combo({"surface_net": budget.SURFACE_NET})
    _, bud, yr_a = ea.run_budget(3, CO2_4x3, want_monthly=False)
    x = np.ascontiguousarray(np.moveaxis(budget.combine_reference(cb, bud), 1, 0))  # [3][4][12][1][ny][nx]
    indices = [regress.Index(0, C_.ANN, 0, True), regress.Index(0, C_.JUL)]
    terms = [regress.Term(0, C_.ANN, 0, True), regress.Term(0, C_.JUL, 1), regress.Term(0, C_.DJF, 0, True)]
    ref = regress.reference(x, indices, terms, CONTROL4, regions=device_regions(nx, ny, 1, {}, x))
    assert np.isfinite(ref.slope[1:]).mean() > 0.9
    plan = regress.Plan(nx, ny, 4, indices, terms, n_vars=1, control=CONTROL4)
    res = eb.run_reg(3, CO2_4x3, plan, records=cb)
    assert res.vars == ("surface_net",)
    same(res, ref, "run_reg of the surface net flux")
    _same_engine_state(ea, eb, yr_a, res.yearly)
    with pytest.raises(engine.GrebError) as ei:  # the plan of one variable does not fit the state records
        eb.run_reg(1, CO2_4x3[:, :1], plan)
    assert ei.value.code == -1 and "n_vars = 1" in str(ei.value) and "5 variables" in str(ei.value), ei.value
    for o in (ea, eb, plan):
        o.close()


def test_refused_calls_leave_the_engine_alone(inputs, params):
    ea, eb = _engines(inputs, params, 2)
    ix, tm = [regress.Index(0, C_.ANN, 0, True)], [regress.Term(0, C_.ANN, 0, True), regress.Term(4, C_.SEP)]
    plan = regress.Plan(96, 48, 4, ix, tm, control=CONTROL4)
    other_grid = regress.Plan(100, 37, 4, ix, tm, control=CONTROL4)
    other_members = regress.Plan(96, 48, 5, ix, tm, control=CONTROL4 + [0])
    other_vars = regress.Plan(96, 48, 4, ix, tm, n_vars=6, control=CONTROL4)
    for bad, words in ((other_grid, ("100 x 37", "96 x 48")), (other_members, ("5 members", "has 4")),
                       (other_vars, ("n_vars = 6", "5 variables"))):
        with pytest.raises(engine.GrebError) as ei:
            ea.run_reg(2, CO2_4x3[:, :2], bad)
        assert ei.value.code == -1 and all(w in str(ei.value) for w in words), ei.value
    yearly = np.zeros((4, 2, 2), np.float32)
    co2 = np.ascontiguousarray(CO2_4x3[:, :2])
    assert engine.lib().greb_engine_run_reg(ea.h, 2, abi.fptr(co2), plan.h, *[None] * 4, abi.fptr(yearly)) == -1
    assert "run_reg: GREB_R_SLOPE selected but `slope` is NULL" in engine.lib().greb_engine_last_error(ea.h).decode()
    ra, rb = ea.run_reg(2, co2, plan), eb.run_reg(2, co2, plan)  # ... bit-identical to an untouched twin
    same(ra, rb, "after the refusals")
    assert np.isfinite(ra.slope[1:]).mean() > 0.9
    _same_engine_state(ea, eb, ra.yearly, rb.yearly)
    for o in (ea, eb, other_grid, other_members, other_vars, plan):
        o.close()
