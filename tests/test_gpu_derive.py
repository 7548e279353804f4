"""GPU: derived records -- the derive stage (csrc/greb_derive.hip) against its numpy mirror derive.reference, and the seven
reduced runs over derived records against the same runs over the records themselves and against the plans' mirrors.

Equality here means the same bits, or NaN on both sides.  The arithmetic ops, SELECT and the locals are held to it
everywhere.  EXP, LOG and ATAN go through an fp64 library on either side; two such libraries may differ in the last fp64
bit, which changes the fp32 result only within about 2^-29 of a rounding boundary: every element within one fp32 ulp, and at
most a share of 1e-5 of the elements different at all (the expectation is below 0.01 elements per test)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from greb_climate_model_amd import abi, clim, cross, derive, diag, engine, ens, gram, lin, regress, workload

pytestmark = pytest.mark.gpu

NM, YEARS = 3, 2
CO2 = np.array([[340.0, 350.0], [680.0, 700.0], [1020.0, 1000.0]], np.float32)
CO2_5 = np.array([[340.0, 400.0, 480.0, 560.0, 680.0], [1020.0, 900.0, 800.0, 700.0, 600.0], [500.0, 520.0, 540.0, 560.0, 580.0]], np.float32)
ANN = cross.SELECTORS.index("ANN")
SHARE = 1e-5  # of the elements may differ where an fp64 library is involved


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing(got, ref):
    """Where two float32 arrays are not equal: different bits and not NaN on both sides."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    return (bits(got) != bits(ref)) & ~(np.isnan(got) & np.isnan(ref))


def assert_equal(got, ref, label):
    bad = differing(got, ref)
    print(f"{label}: {int(bad.sum())} of {bad.size} values differ from the mirror")
    assert not bad.any(), (label, int(bad.sum()), np.asarray(got)[bad][:4], np.asarray(ref)[bad][:4])


def special_records(shape, seed):
    """fp32 records of both signs within 1e-1 ... 1e1 in magnitude with 0, -0, +inf, -inf and NaN strewn in."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-1, 1, shape)).astype(np.float32)
    for k, v in enumerate((0.0, -0.0, np.inf, -np.inf, np.nan)):
        x[rng.random(shape) < 0.02] = v
    return x


def apply_to_host(prog, s, b=None):
    import torch
    out = derive.apply_dev(prog, torch.from_numpy(s).cuda(), None if b is None else torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------- 1. the arithmetic ops against the mirror
def every_op_program():
    """One output of exactly 64 instructions: a stack of exactly eight, every arithmetic op, SELECT, TEE and GET, a field;
    it names seven records, so the eighteen-record instantiation of the kernel runs it."""
    S, T, F, K = derive.STATE, derive.TERM, derive.FIELD, derive.CONST
    ins = [(S, 0, 0), (S, 1, 0), (S, 2, 0), (S, 3, 0), (S, 4, 0), (T, 0, 0), (T, 1, 0), (T, 12, 0)]  # eight values
    ins += [(op, 0, 0) for op in (derive.MUL, derive.DIV, derive.MIN, derive.MAX, derive.SUB, derive.ADD, derive.LT)]
    ins += [(derive.TEE, 0, 0), (S, 0, 0), (S, 1, 0), (derive.SELECT, 0, 0), (T, 5, 0), (derive.GE, 0, 0), (derive.TEE, 3, 0)]
    ins += [(S, 2, 0), (derive.ADD, 0, 0), (derive.NEG, 0, 0), (derive.ABS, 0, 0), (derive.SQRT, 0, 0), (derive.NEG, 0, 0), (F, 1, 0), (derive.MUL, 0, 0)]
    pushes = [(S, 3, 0), (T, 12, 0), (K, 0, 1.5), (derive.GET, 0, 0), (F, 0, 0), (S, 4, 0), (derive.GET, 3, 0), (K, 0, -0.25)]
    ops = [derive.ADD, derive.SUB, derive.MUL, derive.DIV, derive.MIN, derive.MAX]
    k = 0
    while len(ins) < 64:
        ins += [pushes[k % len(pushes)], (ops[k % len(ops)], 0, 0)]
        k += 1
    assert len(ins) == 64 and {i[0] for i in ins} >= set(range(derive.ADD, derive.SQRT + 1)) | {derive.SELECT, derive.TEE, derive.GET}
    return ins


def sixteen_outputs():
    a, q, al = derive.state("Tsurf"), derive.state("q"), derive.state("albedo")
    t = a - 273.15
    outs = {"copy": a, "tc": t, "sq": t * t + t, "ice": al >= 0.4, "lt": q < 0.5, "mn": derive.minimum(a, q), "mx": derive.maximum(q, al),
            "neg": -q, "abs": abs(t), "sqrt": derive.sqrt(al), "sel": derive.where(al, a / al, 0.0), "f": derive.field("f0") * q,
            "g": derive.field("f1") - derive.term("dq_crcl"), "const": derive.const(2.5), "tair": derive.state("Tair") / 3.0,
            "to": derive.state("Tocean") * derive.term("sw")}
    assert len(outs) == 16
    return outs


@pytest.mark.parametrize("nx,ny", [(24, 24), (96, 48)], ids=["np576", "np4608"])
def test_apply_dev_arithmetic_against_the_mirror(nx, ny):
    """np = 576: 5184 lanes, the last workgroup partly idle; np = 4608: 162 workgroups.  Three members."""
    s = special_records((NM, 12, 5, ny, nx), seed=nx)
    b = special_records((NM, 12, 13, ny, nx), seed=nx + 1)
    f = np.random.default_rng(nx + 2).uniform(-2, 2, (2, ny, nx)).astype(np.float32)
    f[0, 0, :4] = (0.0, -0.0, 1.0, -1.0)
    progs = {"every op, 64 instructions": derive.Program(["all"], [every_op_program()], f, ("f0", "f1")),
             "16 outputs": derive.program(sixteen_outputs(), fields={"f0": f[0], "f1": f[1]}),
             "1 output": derive.program({"tc": derive.celsius("Tsurf")}),
             "term 12 and state 4": derive.program({"ends": derive.term(12) * derive.state(4)})}
    assert progs["16 outputs"].n_out == 16 and progs["1 output"].n_out == 1
    for label, prog in progs.items():
        got = apply_to_host(prog, s, b if prog.uses_budget else None)
        ref = derive.reference(prog, s, b)
        assert got.shape == ref.shape == (NM, 12, prog.n_out, ny, nx)
        assert_equal(got, ref, f"{nx}x{ny} {label}")
        assert np.isnan(ref).any() and np.isfinite(ref).any()
        prog.close()
    one = progs["16 outputs"]
    got = apply_to_host(one, s, b)
    assert np.array_equal(bits(got[:, :, 0]), bits(s[:, :, 0]))  # a copy, -0.0 and the NaNs' bits included
    assert np.array_equal(bits(apply_to_host(one, s[2:], b[2:])[0]), bits(got[2]))  # a member alone: the bits it has in the batch
    one.close()


# ---------------------------------------------------------------- 2. the fp64 functions
def within_one_ulp_and_rare(got, ref, label):
    bad = differing(got, ref)
    allowed = int(SHARE * bad.size)
    print(f"{label}: {int(bad.sum())} of {bad.size} values differ from the mirror (allowed: {allowed})")
    assert int(bad.sum()) <= allowed, (label, int(bad.sum()), allowed)
    return bad


def test_exp_log_atan_against_the_mirror():
    rng = np.random.default_rng(11)
    shape = (5, 12, 48, 96)
    s = np.zeros((5, 12, 5, 48, 96), np.float32)
    s[:, :, 0] = rng.uniform(-100.0, 100.0, shape)                                # exp: under- and overflow at both ends
    s[:, :, 1] = np.abs(rng.standard_normal(shape)) * 10.0 ** rng.uniform(-6, 6, shape)  # log
    s[:, :, 2] = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)          # atan
    for v in range(3):
        for k, x in enumerate((0.0, -0.0, np.inf, -np.inf, np.nan, -1.0)):
            s[0, 0, v, 0, k] = x
    prog = derive.program({"exp": derive.exp(derive.state(0)), "log": derive.log(derive.state(1)), "atan": derive.atan(derive.state(2))})
    got, ref = apply_to_host(prog, s), derive.reference(prog, s)
    bad = within_one_ulp_and_rare(got, ref, "EXP, LOG, ATAN")
    if bad.any():  # within one fp32 ulp
        g, r = got[bad].astype(np.float64), ref[bad].astype(np.float64)
        assert (np.abs(g - r) <= np.spacing(np.abs(ref[bad])).astype(np.float64)).all(), (got[bad][:4], ref[bad][:4])
    assert not differing(got[0, 0, :, 0, :5], ref[0, 0, :, 0, :5]).any()  # of 0, -0, inf, -inf and NaN
    prog.close()


def physical_year(n, seed=3):
    rng = np.random.default_rng(seed)
    shape = (n, 12, 48, 96)
    t = rng.uniform(230.0, 315.0, shape).astype(np.float32)
    return np.stack([t, t - np.float32(2.0), rng.uniform(271.0, 300.0, shape).astype(np.float32),
                     rng.uniform(1e-4, 0.02, shape).astype(np.float32), rng.uniform(0.05, 0.7, shape).astype(np.float32)], axis=2)


def test_rel_humidity_and_wet_bulb_against_the_mirror(inputs, params):
    prog = derive.program({"rh": derive.rel_humidity(inputs, params), "tw": derive.wet_bulb(inputs, params)})
    compare = {derive.MIN, derive.MAX, derive.GE, derive.LT, derive.SELECT}
    assert not compare & {op for ins in prog.instructions for op, _, _ in ins}  # no comparison behind a function
    s = physical_year(5)
    got, ref = apply_to_host(prog, s), derive.reference(prog, s)
    assert np.isfinite(ref).all()
    bad = within_one_ulp_and_rare(got, ref, "rel_humidity, wet_bulb")
    if bad.any():
        assert (np.abs(got[bad].astype(np.float64) / ref[bad].astype(np.float64) - 1) <= 1e-5).all(), (got[bad][:4], ref[bad][:4])
    prog.close()


# ---------------------------------------------------------------- 3. identity through every plan
def regions_for(nx, ny, seed=5):
    lat = np.broadcast_to(diag.latitudes(ny)[:, None], (ny, nx))
    return {"NH": (lat > 0).astype(np.float32), "fractional": np.random.default_rng(seed).uniform(0.0, 1.0, (ny, nx)).astype(np.float32)}


def same_results(got, ref, label):
    """Two Results of one kind: every array equal element by element (same bits, or NaN on both sides)."""
    g, r = vars(got), vars(ref)
    assert set(g) == set(r)
    seen = 0
    for name in g:
        if name == "vars" or not isinstance(r[name], np.ndarray):
            assert isinstance(g[name], np.ndarray) == isinstance(r[name], np.ndarray), (label, name)
            continue
        a, c = g[name], r[name]
        assert a.dtype == c.dtype and a.shape == c.shape, (label, name, a.dtype, c.dtype, a.shape, c.shape)
        if a.dtype == np.float32:
            assert_equal(a, c, f"{label} {name}")
        else:
            assert np.array_equal(a, c, equal_nan=a.dtype.kind == "f"), (label, name)
        seen += 1
    assert seen >= 2, (label, sorted(g))


def same_engines(a, b, label):
    for m in range(a.nm):
        assert np.array_equal(bits(a.state(m)), bits(b.state(m))), f"{label}: state of member {m} differs"
    assert a.describe() == b.describe(), (label, a.describe(), b.describe())


def plan_kinds(nx, ny, nm, nv):
    """name -> (make the plan, run it on an engine over `records`)"""
    W = np.array([[1 / 3, 1 / 3, 1 / 3], [0.0, -1.0, 1.0]])[:, :nm] if nm == 3 else np.ones((1, nm))
    D = np.array([[1.0, 0.0], [1.0, -0.5], [1.0, 0.5]]) if nm == 3 else None
    ctl = [-1] + [0] * (nm - 1)
    return {
        "diag": (lambda: diag.Plan(nx, ny, regions_for(nx, ny), n_vars=nv), lambda e, p, co2, r: e.run_diag(co2.shape[1], co2, p, records=r)),
        "clim": (lambda: clim.Plan(nx, ny, nm, control=ctl, n_vars=nv),
                 lambda e, p, co2, r: e.run_clim(co2.shape[1], co2, p, [(0, co2.shape[1])], records=r)),
        "ens": (lambda: ens.Plan(nx, ny, nm, [0] * nm, control=[0] * nm, probs=(0.1, 0.5)),
                lambda e, p, co2, r: e.run_ens(co2.shape[1], co2, p, records=r)),
        "lin": (lambda: lin.Plan(nx, ny, nm, W, design=D), lambda e, p, co2, r: e.run_lin(co2.shape[1], co2, p, records=r)),
        "gram": (lambda: gram.Plan(nx, ny, nm, 12 * nv, gram.blocks_by_var(nv)), lambda e, p, co2, r: e.run_gram(co2.shape[1], co2, p, records=r)),
        "cross": (lambda: cross.Plan(nx, ny, nm, [cross.Event(0, ANN, 288.0), cross.Event(nv - 1, 6, 0.3, -1)], n_vars=nv, group=[0] * nm),
                  lambda e, p, co2, r: e.run_cross(co2.shape[1], co2, p, records=r)),
        "reg": (lambda: regress.Plan(nx, ny, nm, [regress.Index(0, ANN)], [regress.Term(nv - 1, ANN), regress.Term(0, 0)], n_vars=nv),
                lambda e, p, co2, r: e.run_reg(co2.shape[1], co2, p, records=r)),
    }


IDENTITY = derive.program({n: derive.state(n) for n in derive.STATE_NAMES})
TERMS = derive.program({n: derive.term(n) for n in abi.BUDGET_NAMES})


@pytest.mark.parametrize("kind", ["diag", "clim", "ens", "lin", "gram", "cross", "reg"])
def test_identity_program_gives_the_state_run(inputs, params, kind):
    make, run = plan_kinds(inputs.nx, inputs.ny, NM, 5)[kind]
    ea, eb = (engine.Engine(inputs, params, n_members=NM) for _ in range(2))
    pa, pb = make(), make()
    got, ref = run(ea, pa, CO2, IDENTITY), run(eb, pb, CO2, "state")
    assert got.vars == derive.STATE_NAMES
    same_results(got, ref, f"run_{kind} over the identity program")
    same_engines(ea, eb, kind)
    assert ea.describe()["budget_runs"] == 0
    for x in (ea, eb, pa, pb):
        x.close()


@pytest.mark.parametrize("kind", ["diag", "ens"])
def test_term_program_gives_the_budget_run(inputs, params, kind):
    make, run = plan_kinds(inputs.nx, inputs.ny, NM, 13)[kind]
    ea, eb = (engine.Engine(inputs, params, n_members=NM) for _ in range(2))
    pa, pb = make(), make()
    got, ref = run(ea, pa, CO2, TERMS), run(eb, pb, CO2, "budget")
    assert got.vars == abi.BUDGET_NAMES
    same_results(got, ref, f"run_{kind} over the thirteen terms")
    same_engines(ea, eb, kind)
    assert ea.describe()["budget_runs"] == 1
    for x in (ea, eb, pa, pb):
        x.close()


# ---------------------------------------------------------------- 4. non-linear, end to end
@pytest.fixture(scope="module")
def twin5(inputs, params):
    """run_budget over five years on a twin engine: state records [3][5][12][5][48][96], budget records, yearly, final states."""
    e = engine.Engine(inputs, params, n_members=NM)
    mon, bud, yearly = e.run_budget(5, CO2_5)
    state = [e.state(m) for m in range(NM)]
    e.close()
    return mon, bud, yearly, state


def within_bound(got, ref64, abs64, n, label):
    """tests/test_gpu_budget_reduced.py: |got - ref| <= ulp32(ref) + n * 2^-52 * (sum |w x| / sum w), the device's fp64 sum of
    n addends and the mirror's."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref64.shape == abs64.shape, (label, got.dtype, got.shape, ref64.shape)
    bound = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64) + n * 2.0 ** -52 * abs64
    err = np.abs(got.astype(np.float64) - ref64)
    print(f"{label}: max |device - mirror| / bound = {(err / bound).max():.3f} over {err.size} values")
    assert (err <= bound).all(), (label, float((err / bound).max()))


def check_left_as_run(e, res, twin, label):
    _, _, yearly, state = twin
    assert np.array_equal(res.yearly, yearly), f"{label}: yearly is not run()'s"
    for m in range(NM):
        assert np.array_equal(bits(e.state(m)), bits(state[m])), f"{label}: state of member {m} is not run()'s"


def test_ice_extent_through_run_diag(inputs, params, twin5):
    mon = twin5[0]
    t = float(np.float32(np.median(mon[:, :, :, 4])))
    prog = derive.program({"ice": derive.ice_cover(t)})
    x = derive.reference(prog, mon)  # [3][5][12][1][48][96]
    assert set(np.unique(x)) == {0.0, 1.0}
    per_month = x.reshape(NM, 5, 12, -1)
    assert (per_month.max(axis=-1) == 1).all() and (per_month.min(axis=-1) == 0).all()  # both values in every month
    plan = diag.Plan(inputs.nx, inputs.ny, regions_for(inputs.nx, inputs.ny), n_vars=1)
    e = engine.Engine(inputs, params, n_members=NM)
    res = e.run_diag(5, CO2_5, plan, records=prog)
    assert res.vars == ("ice",) and res.regions.shape == (NM, 5, 12, 1, 3)
    ny, nx = inputs.ny, inputs.nx
    for k in range(NM):
        for y in range(5):
            ref = diag.reduce_reference(x[k, y], plan.weights)
            for i, (name, n) in enumerate((("regions", ny * nx), ("zonal", nx), ("annual", 12))):
                within_bound(getattr(res, name)[k, y], ref[i], ref[i], n, f"ice extent member {k} year {y} {name}")  # (x >= 0: |x| = x)
    assert 0.05 < res.regions[..., 0].min() and res.regions[..., 0].max() < 0.95
    check_left_as_run(e, res, twin5, "run_diag over ice_cover")
    e.close(); plan.close(); prog.close()


def test_celsius_crossing_through_run_cross(inputs, params, twin5):
    mon = twin5[0]
    prog = derive.program({"tc": derive.celsius("Tsurf")})
    x = derive.reference(prog, mon)  # [3][5][12][1][48][96]
    years = [np.ascontiguousarray(x[:, y]) for y in range(5)]
    thr = float(np.float32(np.median(cross.quantity(years[0], cross.Event(0, ANN, 0.0)))))
    events = [cross.Event(0, ANN, thr), cross.Event(0, 0, thr, -1)]
    ref = cross.reference(np.stack(years), events, group=[0, 0, 0])
    assert (ref.first >= 0).any() and (ref.first < 0).any() and 0 < ref.fraction.mean() < 1  # hits and misses
    plan = cross.Plan(inputs.nx, inputs.ny, NM, events, n_vars=1, group=[0, 0, 0])
    e = engine.Engine(inputs, params, n_members=NM)
    res = e.run_cross(5, CO2_5, plan, records=prog)
    assert res.vars == ("tc",)
    for name in cross.PRODUCTS:
        g, r = getattr(res, name), getattr(ref, name)
        assert g.dtype == r.dtype and g.shape == r.shape, (name, g.dtype, r.dtype, g.shape, r.shape)
        if g.dtype == np.float32:
            assert_equal(g, r, f"run_cross over celsius {name}")
        else:
            assert np.array_equal(g, r), name
    check_left_as_run(e, res, twin5, "run_cross over celsius")
    e.close(); plan.close(); prog.close()


def test_bowen_spread_through_run_ens(inputs, params, twin5):
    mon, bud = twin5[0], twin5[1]
    prog = derive.program({"bowen": derive.bowen(), "tc": derive.celsius("Tair")})  # terms and a state record in one program
    x = derive.reference(prog, mon, bud)
    plan = ens.Plan(inputs.nx, inputs.ny, NM, [0, 0, 0], probs=[0.25, 1.0])
    e = engine.Engine(inputs, params, n_members=NM)
    res = e.run_ens(5, CO2_5, plan, records=prog)
    assert res.vars == ("bowen", "tc")
    for y in range(5):
        ref = ens.reference(x[:, y], [0, 0, 0], probs=[0.25, 1.0])
        for name in ens.PRODUCTS:
            assert_equal(getattr(res, name)[:, y], getattr(ref, name), f"run_ens over bowen year {y} of 5 {name}")
    assert not np.array_equal(x[:, 0], x[:, 2]) and not np.array_equal(x[:, 1], x[:, 3]), "the years differ"
    check_left_as_run(e, res, twin5, "run_ens over bowen")
    assert e.describe()["budget_runs"] == 1
    e.close(); plan.close(); prog.close()


# ---------------------------------------------------------------- 5. which kernels integrate
def test_a_program_without_terms_launches_no_budget_kernels(inputs, params):
    plain, with_term = derive.program({"tc": derive.celsius("Tsurf")}), derive.program({"x": derive.term("sw") - derive.state("Tsurf")})
    plan = diag.Plan(inputs.nx, inputs.ny, n_vars=1)
    p5, p13 = diag.Plan(inputs.nx, inputs.ny), diag.Plan(inputs.nx, inputs.ny, n_vars=13)
    ea, eb, ec, ed = (engine.Engine(inputs, params, n_members=NM) for _ in range(4))
    ra, rb = ea.run_diag(YEARS, CO2, plan, records=plain), eb.run_diag(YEARS, CO2, p5)
    assert ea.describe() == eb.describe() and ea.describe()["budget_runs"] == 0
    rc, rd = ec.run_diag(YEARS, CO2, plan, records=with_term), ed.run_diag(YEARS, CO2, p13, records="budget")
    assert ec.describe() == ed.describe() and ec.describe()["budget_runs"] == 1
    assert np.array_equal(ra.yearly, rb.yearly) and np.array_equal(rc.yearly, rd.yearly) and np.array_equal(ra.yearly, rc.yearly)
    # degrees Celsius are affine: the annual map is the state run's minus 273.15 to within the rounding of either side
    assert np.abs(ra.annual[:, :, 0].astype(np.float64) - (rb.annual[:, :, 0].astype(np.float64) - 273.15)).max() < 1e-4
    for x in (ea, eb, ec, ed, plan, p5, p13, plain, with_term):
        x.close()


# ---------------------------------------------------------------- 6. an any-grid case
def test_identity_run_diag_row_strips_g192x48():
    nx, ny = 192, 48
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 3, ipy=max(2, (3 * ny) // 4))
    ea, eb = engine.Engine(inp, p), engine.Engine(inp, p)
    assert ea.describe()["engine"] == "row strips"
    pa, pb = (diag.Plan(nx, ny, regions_for(nx, ny)) for _ in range(2))
    got, ref = ea.run_diag(1, 680.0, pa, records=IDENTITY), eb.run_diag(1, 680.0, pb)
    same_results(got, ref, "row strips, identity program")
    assert np.array_equal(bits(ea.state(0)), bits(eb.state(0)))
    for x in (ea, eb, pa, pb):
        x.close()


# ---------------------------------------------------------------- 7. refusals on a live engine
def test_refusals_leave_the_engine_alone(inputs, params):
    import torch
    e, twin = (engine.Engine(inputs, params, n_members=NM) for _ in range(2))
    first = [x.run(1, CO2[:, :1]) for x in (e, twin)]
    assert np.array_equal(bits(first[0][0]), bits(first[1][0]))
    one = derive.program({"tc": derive.celsius("Tsurf")})
    d5, d1 = diag.Plan(inputs.nx, inputs.ny), diag.Plan(inputs.nx, inputs.ny, n_vars=1)
    with pytest.raises(engine.GrebError) as ei:  # a plan with the wrong n_vars
        e.run_diag(1, CO2[:, :1], d5, records=one)
    assert ei.value.code == -1 and "n_vars = 5" in str(ei.value) and "1 variables" in str(ei.value), str(ei.value)
    out = np.empty((NM, 1, 12, 1, 1), np.float32)
    yearly = np.empty((NM, 1, 2), np.float32)
    co2 = np.ascontiguousarray(CO2[:, :1])
    rc = engine.lib().greb_engine_run_derived_diag(e.h, 1, abi.fptr(co2), one.handle(24, 24), d1.h, C.c_uint(abi.D_REGIONS), abi.fptr(out),
                                                   None, None, abi.fptr(yearly))  # a derive plan of another grid
    msg = engine.lib().greb_engine_last_error(e.h).decode()
    assert rc == -1 and "24 x 24" in msg and "96 x 48" in msg, (rc, msg)
    rc = engine.lib().greb_engine_run_derived_diag(e.h, 1, abi.fptr(co2), None, d1.h, C.c_uint(abi.D_REGIONS), abi.fptr(out), None, None,
                                                   abi.fptr(yearly))
    assert rc == -1 and "greb_derive is NULL" in engine.lib().greb_engine_last_error(e.h).decode()
    with_term = derive.program({"b": derive.bowen()})
    with pytest.raises(engine.GrebError) as ei:  # budget_year_dev == NULL with a TERM
        derive.apply_dev(with_term, torch.zeros((1, 12, 5, inputs.ny, inputs.nx), device="cuda"))
    assert ei.value.code == -1 and "budget_year_dev is NULL" in str(ei.value), str(ei.value)
    assert e.describe() == twin.describe() and e.describe()["budget_runs"] == 0
    (mon_a, yr_a), (mon_b, yr_b) = e.run(1, CO2[:, 1:]), twin.run(1, CO2[:, 1:])  # the engine runs on unchanged
    assert np.array_equal(bits(mon_a), bits(mon_b)) and np.array_equal(yr_a, yr_b)
    for m in range(NM):
        assert np.array_equal(bits(e.state(m)), bits(twin.state(m))), m
    for x in (e, twin, d5, d1, one, with_term):
        x.close()


# ---------------------------------------------------------------- 8. the tool
def test_tool_prints_one_json_line():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "run_derived.py"), "4", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    assert res["members"] == 4 and res["years"] == 3 and res["finite"] is True
    assert res["regions"][0] == "globe" and np.asarray(res["ice_extent"]).shape == (4, 3, 12, len(res["regions"]))
    assert 0 <= np.min(res["ice_extent"]) and np.max(res["ice_extent"]) <= 1
    assert len(res["wet_bulb_first_year"]) == 4 and res["wet_bulb_limit_C"] > 0
    assert np.asarray(res["rel_humidity_spread"]).shape == (3, 12) and np.min(res["rel_humidity_spread"]) >= 0
    assert res["ensemble_years_per_s"]["derived"] > 0 and res["ensemble_years_per_s"]["state"] > 0
    st = res["stage"]
    assert st["derive_ms"] > 0 and st["combine_ms"] > 0 and st["bytes"] > 0 and st["derive_GB_per_s"] > 0 and st["combine_GB_per_s"] > 0
