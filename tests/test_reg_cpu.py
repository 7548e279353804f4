"""CPU: the regression interface (include/greb_engine.h: greb_reg_*, greb_engine_run_reg) -- its symbols, its kernels in the
built library, its argument errors (all reported before any device query) -- and the numpy mirror regress.reference: on
hand-made series whose answers are written out here, for the bits of a season index, and against a two-pass least-squares
fit in np.longdouble.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, cross, diag, engine, regress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("greb_reg_create", "greb_reg_destroy", "greb_reg_add_year_dev", "greb_reg_finish_dev", "greb_engine_run_reg",
       "greb_engine_run_budget_reg")
NX, NY = 12, 5
I, T = regress.Index, regress.Term


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


# ---- interface -------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    f90 = open(os.path.join(ROOT, "greb_climate_model_amd", "host", "greb_c_api.f90")).read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", code), n
        assert n in engine.EXPORTS and hasattr(lib, n), n
        assert f'name="{n}"' in f90, n
    for t in ("greb_reg_index", "greb_reg_term"):
        assert f"type, bind(C) :: {t}" in f90 and f"}} {t};" in code, t
    for name in ("SLOPE", "INTERCEPT", "R2", "INDEX"):
        assert re.search(rf"#define GREB_R_{name}\s+{getattr(abi, 'R_' + name)}u", code), name
    assert re.search(rf"#define GREB_REG_MAX_INDICES\s+{abi.REG_MAX_INDICES}\b", code) and abi.REG_MAX_INDICES == 8
    assert re.search(rf"#define GREB_REG_MAX_TERMS\s+{abi.REG_MAX_TERMS}\b", code) and abi.REG_MAX_TERMS == 16
    assert C.sizeof(abi.GrebRegIndex) == C.sizeof(abi.GrebRegTerm) == 16
    text = " ".join(hdr.split())
    assert "centred on year 0" in text and "1.06 GB" in text and "never fused" in text
    state = 28 * 512 * 16 * 4608  # the tool's example run: 1.06 GB
    assert round(state / 1e9, 2) == 1.06
    total = regress.memory_bytes(regress.ALL, 512, 16, 1, 48, 96)
    assert state < total < state * 1.01  # the regional means, diag's scratch and the index words are small beside it
    assert regress.memory_bytes(abi.R_SLOPE, 512, 16, 1, 48, 96) - (total - state) == 20 * 512 * 16 * 4608
    assert regress.memory_bytes(regress.ALL, 2, 3, 4, 48, 96, run_years=10) - regress.memory_bytes(regress.ALL, 2, 3, 4, 48, 96) == \
        4 * 2 * 3 * 4608 + 4 * 2 * 10 * 4


def test_library_has_the_reg_kernels_for_gfx950(lib):
    from greb_climate_model_amd import codesha
    assert "greb_reg.hip" in build.SOURCES and "greb_reg.h" in build.HEADERS
    assert build.EXTRA_FLAGS["greb_reg.hip"] == build.EXTRA_FLAGS["greb_cross.hip"] == ["-ffp-contract=off"]
    for name, n in (("reg_update_kernel", 2), ("reg_index_kernel", 1), ("reg_finish_kernel", 1)):
        got = codesha.kernel_functions(build.LIB, name)
        assert len(got) == n and all(len(c) > 64 for c in got.values()), (name, sorted(got))


# ---- argument errors -------------------------------------------------------------------------------------------------
def _err(fn, code=-1):
    with pytest.raises(engine.GrebError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_plan_argument_errors_name_the_offender(lib):
    ix, tm = [I(0, cross.ANN)], [T(0, cross.ANN)]
    P = lambda nm, i=ix, t=tm, **k: regress.Plan(96, 48, nm, i, t, **k)
    arctic = {"Arctic": np.ones((48, 96), np.float32)}
    P(3).close()
    P(3, [I(4, cross.SEP, "Arctic", True)] * 8, [T(4, cross.SEP, 7, True)] * 16, regions=arctic, control=[1, 1, -1]).close()
    for gx, gy in ((95, 48), (8, 48), (96, 4), (96, 193)):  # the grids diag.Plan rejects
        assert f"reg_create: grid {gx} x {gy}" in _err(lambda: regress.Plan(gx, gy, 1, ix, tm))
    assert "n_members = 0" in _err(lambda: P(0))
    assert "n_members = 65536 (1 ... 65535)" in _err(lambda: P(65536)) and abi.REG_MAX_MEMBERS == 65535
    P(65535).close()
    assert "n_vars = 0" in _err(lambda: P(1, n_vars=0))
    assert "n_vars = 17" in _err(lambda: P(1, n_vars=17))
    assert "n_indices = 0" in _err(lambda: P(1, []))
    assert "n_indices = 9" in _err(lambda: P(1, ix * 9))
    assert "n_terms = 0" in _err(lambda: P(1, ix, []))
    assert "n_terms = 17" in _err(lambda: P(1, ix, tm * 17))
    assert "n_regions = 16" in _err(lambda: P(1, regions={str(k): arctic["Arctic"] for k in range(16)}))
    assert "`what` = 0" in _err(lambda: P(1, what=0))
    assert "`what` = 16" in _err(lambda: P(1, what=16))
    for bad in (5, -1):
        msg = _err(lambda: P(1, ix + [I(bad, 0)]))
        assert "index 1" in msg and f"var = {bad}" in msg, msg
        msg = _err(lambda: P(1, ix, tm + [T(bad, 0)]))
        assert "term 1" in msg and f"var = {bad}" in msg, msg
    P(1, [I(12, 0)], [T(12, 0)], n_vars=13).close()
    for bad in (17, -1):
        msg = _err(lambda: P(1, ix * 2 + [I(0, bad)]))
        assert "index 2" in msg and f"sel = {bad}" in msg, msg
        msg = _err(lambda: P(1, ix, tm * 2 + [T(0, bad)]))
        assert "term 2" in msg and f"sel = {bad}" in msg, msg
    for bad in (2, -1):
        msg = _err(lambda: P(1, [I(0, 0, bad)], regions=arctic))
        assert "index 0" in msg and f"region = {bad}" in msg, msg
    msg = _err(lambda: P(1, [I(0, 0, 1)]))  # no regions but the globe
    assert "index 0" in msg and "region = 1" in msg, msg
    for bad in (1, -1):
        msg = _err(lambda: P(1, ix, tm + [T(0, 0, bad)]))
        assert "term 1" in msg and f"index = {bad}" in msg, msg
    msg = _err(lambda: P(2, [I(0, 0, rel=2)], control=[0, 0]))
    assert "index 0" in msg and "rel = 2" in msg, msg
    msg = _err(lambda: P(2, ix, [T(0, 0, rel=2)], control=[0, 0]))
    assert "term 0" in msg and "rel = 2" in msg, msg
    msg = _err(lambda: P(2, ix, tm + [T(0, 0, rel=True)]))
    assert "term 1: rel = 1" in msg and "`control` is NULL" in msg, msg
    msg = _err(lambda: P(2, ix + [I(0, 0, rel=True)], tm + [T(0, 0, 1)]))  # through the index the term names
    assert "term 1: its index 1 has rel = 1" in msg and "`control` is NULL" in msg, msg
    msg = _err(lambda: P(2, ix + [I(0, 0, rel=True)]))  # an index no term names
    assert "index 1: rel = 1" in msg and "`control` is NULL" in msg, msg
    for bad in (np.nan, np.inf, -0.5, 1.5):
        w = np.ones((48, 96), np.float32)
        w[7, 11] = bad
        msg = _err(lambda: P(1, regions={"ok": arctic["Arctic"], "Arctic": w}))
        assert "reg_create: region 2 ('Arctic'): weight" in msg and "row 7, column 11 is not in [0, 1]" in msg, msg
    msg = _err(lambda: P(1, regions={"none": np.zeros((48, 96), np.float32)}))
    assert "reg_create: region 1 ('none') has zero weight everywhere" in msg, msg
    assert "shape (5, 12)" in _err(lambda: P(1, regions={"small": np.ones((5, 12), np.float32)}))
    north = I(0, 0, "Arctic")  # a plan resolves the name in its own copy: the caller's Index serves a plan with other regions
    a, b = P(1, [north], regions=arctic), P(1, [north], regions={"ok": arctic["Arctic"], **arctic})
    assert north.region == "Arctic" and (a.indices[0].region, b.indices[0].region) == (1, 2)
    a.close(); b.close()
    assert "names region 'Antarctic'" in _err(lambda: P(1, [I(0, 0, "Antarctic")], regions=arctic))
    msg = _err(lambda: P(3, control=[0, 3, 0]))
    assert "member 1" in msg and "control = 3" in msg, msg
    msg = _err(lambda: P(3, control=[0, 0, -2]))
    assert "member 2" in msg and "control = -2" in msg, msg
    assert "3 integers" in _err(lambda: P(3, control=[0, 0]))
    h = C.c_void_p()
    ci, ct = (abi.GrebRegIndex * 1)(), (abi.GrebRegTerm * 1)()
    assert lib.greb_reg_create(96, 48, 1, 5, None, 0, None, ci, 1, ct, 1, 1, None) == -1
    assert lib.greb_reg_create(96, 48, 1, 5, None, 0, None, None, 1, ct, 1, 1, C.byref(h)) == -1
    assert "`indices` NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_reg_create(96, 48, 1, 5, None, 0, None, ci, 1, None, 1, 1, C.byref(h)) == -1
    assert "`terms` NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_reg_create(96, 48, 1, 5, None, 1, None, ci, 1, ct, 1, 1, C.byref(h)) == -1
    assert "region_w is NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_reg_create(96, 48, 1, 5, None, 0, None, ci, 1, ct, 1, 1, C.byref(h)) == 0 and lib.greb_reg_destroy(h) == 0
    assert lib.greb_reg_destroy(None) == 0
    p = P(512, ix, tm * 16)
    assert "512 members x 16 terms" in p.describe() and f"{p.memory_bytes() / 1e6:.1f} MB" in p.describe()
    assert round(p.memory_bytes() / 1e9, 2) == 1.06
    p.close()
    # the diag plan's own messages are what they were
    assert "diag_create: grid 95 x 48" in _err(lambda: diag.Plan(95, 48))


def _aligned():
    buf = np.zeros(64, np.float32)
    return buf, C.c_void_p((buf.ctypes.data + 15) & ~15)


def test_dev_argument_errors_come_before_any_device_query(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, ok = _aligned()
    bad = C.c_void_p(ok.value + 4)
    plan = regress.Plan(96, 48, 2, [I(0, 0)], [T(0, 0)])  # all four products
    one = regress.Plan(96, 48, 2, [I(0, 0)], [T(0, 0)], what=abi.R_INTERCEPT)
    add, fin = lib.greb_reg_add_year_dev, lib.greb_reg_finish_dev
    assert add(None, 0, ok, 0, ok, None) == -1 and "reg_add_year_dev: no plan" in last()
    assert add(plan.h, 0, None, 0, ok, None) == -1 and "x_dev is NULL" in last()
    assert add(plan.h, 0, bad, 0, ok, None) == -1 and "x_dev is not 16-byte aligned" in last()
    assert add(plan.h, 0, ok, 0, None, None) == -1 and "GREB_R_INDEX selected but `index_dev` is NULL" in last()
    assert add(plan.h, 0, ok, 1, ok, None) == -1 and "k = 1, but 0 years were added" in last()
    assert add(one.h, 0, ok, 2, None, None) == -1 and "k = 2, but 0 years" in last()  # (an unselected pointer is ignored)
    assert fin(None, 0, 1, ok, ok, ok, None) == -1 and "reg_finish_dev: no plan" in last()
    for i, (name, flag) in enumerate(zip(("slope", "intercept", "r2"), ("GREB_R_SLOPE", "GREB_R_INTERCEPT", "GREB_R_R2"))):
        p = [ok] * 3
        p[i] = None
        assert fin(plan.h, 0, 1, *p, None) == -1 and f"{flag} selected but `{name}_dev` is NULL" in last(), last()
        p[i] = bad
        assert fin(plan.h, 0, 1, *p, None) == -1 and f"{name}_dev is not 16-byte aligned" in last(), last()
    assert fin(plan.h, 0, 1, ok, ok, ok, None) == -1 and "n_years = 1, but 0 years were added" in last()
    assert fin(one.h, 0, 0, None, ok, None, None) == -1 and "n_years = 0" in last()
    assert fin(one.h, 0, 1, bad, None, bad, None) == -1 and "`intercept_dev` is NULL" in last()
    plan.close(); one.close()


def test_run_reg_argument_errors_are_decided_without_an_engine(lib):
    """The plan, the variable count, the years and the outputs are looked at before the engine is: no device is needed."""
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, _ = _aligned()
    p = abi.fptr(buf)
    plan = regress.Plan(96, 48, 2, [I(0, 0)], [T(0, 0)])
    thirteen = regress.Plan(96, 48, 2, [I(12, 0)], [T(0, 0)], n_vars=13, what=abi.R_SLOPE)
    two = regress.Plan(96, 48, 2, [I(1, 0)], [T(0, 0)], n_vars=2, what=abi.R_R2 | abi.R_INDEX)
    run, brun = lib.greb_engine_run_reg, lib.greb_engine_run_budget_reg
    good = (p, p, p, p)
    assert run(None, 1, p, None, *good, None) == -1 and "run_reg: no plan" in last()
    assert run(None, 1, p, thirteen.h, *good, None) == -1 and "n_vars = 13" in last() and "5 variables" in last(), last()
    assert run(None, 0, p, plan.h, *good, None) == -1 and "years = 0" in last()
    for k, (name, flag) in enumerate(zip(regress.PRODUCTS, ("GREB_R_SLOPE", "GREB_R_INTERCEPT", "GREB_R_R2", "GREB_R_INDEX"))):
        a = list(good)
        a[k] = None
        assert run(None, 1, p, plan.h, *a, None) == -1 and f"run_reg: {flag} selected but `{name}` is NULL" in last(), last()
    assert run(None, 1, p, plan.h, *good, None) == -1 and "bad argument (engine" in last()
    # the budget route: the thirteen terms want n_vars = 13, a combination of two n_vars = 2
    assert brun(None, 1, p, None, 0, plan.h, *good, None) == -1 and "run_budget_reg" in last() and "13 variables" in last(), last()
    assert brun(None, 1, p, None, 0, thirteen.h, None, None, None, None, None) == -1 and "`slope` is NULL" in last()
    assert brun(None, 1, p, None, 0, thirteen.h, p, None, None, None, None) == -1 and "bad argument (engine" in last()
    combo = np.zeros((2, abi.NBUDGET), np.float32)
    combo[0, 0] = combo[1, 1] = 1
    assert brun(None, 1, p, abi.fptr(combo), 2, thirteen.h, *good, None) == -1 and "2 variables" in last(), last()
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, None, None, p, None, None) == -1 and "`index` is NULL" in last()
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, None, None, p, p, None) == -1 and "bad argument (engine" in last()
    combo[1] = 0
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, *good, None) == -1 and "combo row 1 is zero" in last(), last()
    for x in (plan, thirteen, two):
        x.close()


def test_dev_call_without_a_gpu_is_a_loud_error(lib):
    import torch
    buf, ok = _aligned()
    plan = regress.Plan(96, 48, 1, [I(0, 0)], [T(0, 0)], what=abi.R_SLOPE)
    if not torch.cuda.is_available():
        assert lib.greb_reg_add_year_dev(plan.h, 0, ok, 0, None, None) == -2
        assert b"no CPU path" in lib.greb_engine_last_error(None)
    plan.close()


# ---- the mirror on hand-made series ----------------------------------------------------------------------------------
G6 = np.asarray([280, 281, 282, 283, 284, 285], np.float32)


def _series(g, y, n_members=1):
    """Six years [6][n_members][12][2][NY][NX] that hold 100 everywhere but y [6] (or [6][n_members]) in January of variable 0
    and g in January of variable 1, at every point: the global mean of variable 1 is g itself."""
    x = np.full((6, n_members, 12, 2, NY, NX), 100.0, np.float32)
    for var, v in ((0, y), (1, g)):
        v = np.asarray(v, np.float32).reshape(6, -1)
        x[:, :, 0, var] = np.broadcast_to(v, (6, n_members))[:, :, None, None]
    return x


def _one(res, name, m=0, t=0):
    a = getattr(res, name)[m, t]
    assert (a == a[0, 0]).all() or np.isnan(a).all(), name
    return a[0, 0]


IX, TM = [I(1, cross.JAN)], [T(0, cross.JAN)]


def test_mirror_exact_line_constant_series_and_one_year():
    res = regress.reference(_series(G6, 3 * G6 + 7), IX, TM)
    assert np.array_equal(res.index[0, :, 0], G6)
    # centred: G = 0 ... 5, Y = 0, 3 ... 15; Sxx = 55 - 225/6 = 17.5, Sxy = 165 - 675/6 = 52.5, Syc = 495 - 2025/6 = 157.5
    assert _one(res, "slope") == 3.0 and _one(res, "r2") == 1.0
    assert _one(res, "intercept") == 7.0  # (847 + 45/6) - 3 * (280 + 15/6)
    res = regress.reference(_series(G6, 500 - 0.5 * G6), IX, TM)
    assert _one(res, "slope") == -0.5 and _one(res, "r2") == 1.0 and _one(res, "intercept") == 500.0
    # a line with one year off it: y = g but for +6 in year 5: Sxy = (0+1+4+9+16+55) - 15*21/6 = 32.5, Syc = 151 - 441/6 = 77.5
    y = G6.copy()
    y[5] += 6
    res = regress.reference(_series(G6, y), IX, TM)
    assert _one(res, "slope") == np.float32(32.5 / 17.5) and _one(res, "r2") == np.float32(32.5 * 32.5 / (17.5 * 77.5))
    # a constant y: slope +0, the intercept is y, R2 has nothing to explain
    for g in (G6, G6[::-1].copy()):
        res = regress.reference(_series(g, np.full(6, 250.0)), IX, TM)
        s = _one(res, "slope")
        assert s == 0.0 and not np.signbit(s) and _one(res, "intercept") == 250.0 and np.isnan(_one(res, "r2"))
    # a constant index: nothing to regress on
    res = regress.reference(_series(np.full(6, 288.0), 3 * G6), IX, TM)
    assert all(np.isnan(getattr(res, k)).all() for k in ("slope", "intercept", "r2")) and (res.index == 288.0).all()
    # one year
    res = regress.reference(_series(G6, 3 * G6)[:1], IX, TM)
    assert all(np.isnan(getattr(res, k)).all() for k in ("slope", "intercept", "r2")) and res.index.shape == (1, 1, 1)
    # two years: the line through two points
    res = regress.reference(_series(G6, 3 * G6 + 7)[:2], IX, TM)
    assert _one(res, "slope") == 3.0 and _one(res, "r2") == 1.0 and _one(res, "intercept") == 7.0


def test_mirror_nan_and_control():
    x = _series(G6, 3 * G6 + 7)
    x[3, 0, 0, 0, 2, 5] = np.nan  # one year of one point
    res = regress.reference(x, IX, TM)
    for k in ("slope", "intercept", "r2"):
        a = getattr(res, k)[0, 0]
        assert np.isnan(a[2, 5]) and np.isnan(a).sum() == 1, k
    assert res.slope[0, 0, 0, 0] == 3.0
    x[0, 0, 0, 0, 1, 1] = np.nan  # year 0: y0 itself
    assert np.isnan(regress.reference(x, IX, TM).slope[0, 0]).sum() == 2
    # three members: 0 has no control, 1 has member 2, 2 has itself
    g = np.stack([G6, 2 * G6 - 280, np.full(6, 280.0, np.float32)], axis=1)  # responses: -, 0 2 ... 10, 0
    y = np.stack([G6, 5 * G6, 100 + 0 * G6], axis=1)  # responses: -, 5 g - 100, 0
    x = _series(g, y, 3)
    ctl = [-1, 2, 2]
    res = regress.reference(x, [I(1, cross.JAN, rel=True), I(1, cross.JAN)], [T(0, cross.JAN, 0, True), T(0, cross.JAN, 1, True), T(0, cross.JAN, 1)], ctl)
    assert np.isnan(res.index[0, :, 0]).all() and np.array_equal(res.index[1, :, 0], 2 * G6 - 560) and not res.index[2, :, 0].any()
    for k in ("slope", "intercept", "r2"):
        a = getattr(res, k)
        assert np.isnan(a[0, :2]).all(), k   # control = -1: the rel index, and the rel term on a plain index, are NaN
        assert np.isnan(a[2, 0]).all(), k    # control = m: the index is a zero series, nothing to regress on
    assert _one(res, "slope", 0, 2) == 1.0   # member 0, plain term on the plain index: y = g
    # member 1: its response 5 g - 100 on the index response 2 g - 560, and on the plain index 2 g - 280: slope 2.5 both times
    assert _one(res, "slope", 1, 0) == 2.5 and _one(res, "slope", 1, 1) == 2.5 and _one(res, "r2", 1, 0) == 1.0
    # member 2 against itself on the plain (constant) index: NaN; its own rel term is a zero series
    assert np.isnan(res.slope[2]).all()
    # ... and with an index that varies: slope +0, R2 NaN
    g[:, 2] = G6
    res = regress.reference(_series(g, y, 3), [I(1, cross.JAN)], [T(0, cross.JAN, 0, True)], ctl)
    s = _one(res, "slope", 2)
    assert s == 0.0 and not np.signbit(s) and _one(res, "intercept", 2) == 0.0 and np.isnan(_one(res, "r2", 2))
    with pytest.raises(ValueError):
        regress.reference(x, [I(1, 0, rel=True)], TM)


def test_mirror_season_index_has_the_bits_of_the_season_formula():
    """The index of a season selector: the formula of the contract, written out here, over diag.reduce_reference rounded to
    fp32 -- and `rel` as one fp32 subtraction."""
    rng = np.random.default_rng(5)
    x = (250 + 50 * rng.random((2, 3, 12, 2, NY, NX))).astype(np.float32)
    w = rng.random((2, NY, NX)).astype(np.float32)
    ctl = [2, -1, 0]
    indices = [I(1, cross.DJF, 2), I(0, cross.ANN, 0, True), I(1, cross.JUL, 1, True), I(0, cross.SON, 1)]
    res = regress.reference(x, indices, [T(0, 0)], ctl, region_w=w)
    days = np.asarray(abi.JDAY_MON, np.float64)
    for k in range(2):
        r = diag.reduce_reference(x[k], w)[0].astype(np.float32)  # [3][12][2][3]

        def season(months, var, region):
            acc = np.zeros(3, np.float64)
            for mo in months:
                acc = acc + days[mo] * r[:, mo, var, region].astype(np.float64)
            return (acc / days[list(months)].sum()).astype(np.float32)

        djf, ann, son = season((11, 0, 1), 1, 2), season(range(12), 0, 0), season((8, 9, 10), 0, 1)
        jul = r[:, 6, 1, 1]
        want = np.stack([djf, ann - ann[[2, 0, 0]], jul - jul[[2, 0, 0]], son], axis=1)
        want[1, 1:3] = np.nan  # member 1 has no control
        got = res.index[:, k]
        assert want.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got.view(np.uint32)[~np.isnan(got)], want.view(np.uint32)[~np.isnan(want)]), (k, got, want)


def test_mirror_against_a_two_pass_fit_in_longdouble():
    """The one-pass fp64 sums centred on year 0 against the textbook two-pass fit in np.longdouble, within 1 fp32 ulp of the
    two-pass value for slope and R2.  Why 1 ulp: with C = max(Sgg/Sxx, |Sgy|/|Sxy|, Syy/Syc) <= 2^20 -- asserted below on the
    test's own inputs --, the cancellation in `S.. - S.*S./n` amplifies the relative rounding error of the fp64 sums, about
    n * 2^-53, to at most 2^20 * 10 * 2^-53 < 2^-29 in each of Sxx, Sxy and Syc, so b and R2 (a few of those) are within 2^-26 of
    the exact value, an eighth of an fp32 ulp at worst; the one rounding to fp32 adds half an ulp.  The intercept
    ybar - b * gbar is a difference of two numbers near 288 that are each that accurate, and is rounded once: it is held to one
    fp32 ulp of the largest of the two and the result."""
    rng = np.random.default_rng(11)
    L = np.longdouble
    worst = {"slope": 0.0, "r2": 0.0, "intercept": 0.0}
    for n in range(2, 10):
        nm = 4
        g = (288 + 0.03 * np.arange(n)[:, None] * (1 + rng.random(nm)) + 0.1 * rng.standard_normal((n, nm))).astype(np.float32)
        a = rng.uniform(-2, 3, (nm, NY, NX))
        y = (275 + a * (g[:, :, None, None] - 288) + 0.3 * rng.standard_normal((n, nm, NY, NX))).astype(np.float32)
        x = np.zeros((n, nm, 12, 2, NY, NX), np.float32)
        x[:, :, 0, 0] = y
        reg = np.zeros((n, nm, 12, 2, 1), np.float32)
        reg[:, :, 0, 1, 0] = g
        res = regress.reference(x, IX, TM, regions=reg)
        assert np.array_equal(res.index[:, :, 0], g.T)
        gl, yl = g.astype(L)[:, :, None, None], y.astype(L)
        gb, yb = gl.mean(axis=0), yl.mean(axis=0)
        Sxx, Sxy, Syc = ((gl - gb) ** 2).sum(axis=0), ((gl - gb) * (yl - yb)).sum(axis=0), ((yl - yb) ** 2).sum(axis=0)
        G, Y = gl - gl[0], yl - yl[0]
        cond = max(((G * G).sum(axis=0) / Sxx).max(), (np.abs((G * Y).sum(axis=0)) / np.abs(Sxy)).max(), ((Y * Y).sum(axis=0) / Syc).max())
        assert cond <= 2.0 ** 20, (n, float(cond))
        b = Sxy / Sxx
        two = {"slope": np.broadcast_to(b, y.shape[1:]), "r2": Sxy * Sxy / (Sxx * Syc), "intercept": yb - b * gb}
        scale = {"slope": np.abs(two["slope"]), "r2": np.abs(two["r2"]), "intercept": np.maximum(np.maximum(np.abs(yb), np.abs(b * gb)), np.abs(two["intercept"]))}
        for k in worst:
            got = getattr(res, k)[:, 0]
            assert np.isfinite(got).all(), (n, k)
            ulp = np.spacing(scale[k].astype(np.float32)).astype(L)
            err = float((np.abs(got.astype(L) - two[k]) / ulp).max())
            worst[k] = max(worst[k], err)
            assert err <= 1.0, (n, k, err)
    print("worst error in fp32 ulp:", worst)
