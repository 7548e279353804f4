"""CPU: the texts of the argument errors the output plans share (csrc/greb_plans.cpp), byte for byte.

Every row is one refused call through ctypes that fails before any device is touched, and the whole message it leaves in
greb_engine_last_error.  The plan kinds say the same things about a control map, a group map, a used-member map, a
selected product without a pointer and a period's years; whoever states those once for all kinds must not reword any."""
import ctypes as C

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, engine

NX, NY = 12, 5
VP = C.c_void_p
_keep = []  # the arrays the rows point into


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


def _i32(v):
    if v is None:
        return None
    a = (C.c_int32 * len(v))(*v)
    _keep.append(a)
    return a


def _f64(v):
    a = np.ascontiguousarray(v, np.float64)
    _keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_double))


_buf = np.zeros(64, np.float32)
OK = VP((_buf.ctypes.data + 15) & ~15)  # a 16-byte aligned address: never dereferenced by a refused call
BAD = VP(OK.value + 4)
F = C.cast(OK, C.POINTER(C.c_float))
I = C.cast(OK, C.POINTER(C.c_int32))
D = C.cast(OK, C.POINTER(C.c_double))
SEL = " (0 ... 11: a month; 12 ... 16: DJF, MAM, JJA, SON, ANN)"


# ---- the six creates; each returns (rc, handle)
def clim(L, nm, control, what):
    h = VP()
    return L.greb_clim_create(C.c_int(NX), C.c_int(NY), C.c_int(nm), _i32(control), C.c_uint(what), C.byref(h)), h


def ens(L, nm, group, ng, control, what=abi.S_MEAN):
    h = VP()
    return L.greb_ens_create(NX, NY, nm, _i32(group), ng, _i32(control), None, 0, what, C.byref(h)), h


def lin(L, nm, use, control, what=abi.L_COEF):
    h = VP()
    w = _f64(np.ones((1, nm)))
    return L.greb_lin_create(NX, NY, nm, w, 1, _i32(use), _i32(control), _f64(np.ones((nm, 1))), what, C.byref(h)), h


def gram(L, nm, use, control, n_records=2):
    h = VP()
    return L.greb_gram_create(NX, NY, nm, n_records, _i32([0] * n_records), 1, _i32(use), _i32(control), None, C.byref(h)), h


def cross(L, nm, events, control=None, group=None, ng=0, what=abi.T_FIRST, n_vars=2):
    h = VP()
    ev = (abi.GrebCrossEvent * len(events))(*[abi.GrebCrossEvent(*e) for e in events])
    return L.greb_cross_create(NX, NY, nm, n_vars, ev, len(events), _i32(control), _i32(group), ng, what, C.byref(h)), h


def reg(L, nm, terms, control=None, indices=((0, 16, 0, 0),), what=abi.R_SLOPE, n_vars=2):
    h = VP()
    ix = (abi.GrebRegIndex * len(indices))(*[abi.GrebRegIndex(*i) for i in indices])
    tm = (abi.GrebRegTerm * len(terms))(*[abi.GrebRegTerm(*t) for t in terms])
    return L.greb_reg_create(NX, NY, nm, n_vars, None, 0, _i32(control), ix, len(indices), tm, len(terms), what, C.byref(h)), h


EV = (0, 16, 0, 1, 1.5)  # var, sel, rel, dir, thr
TM = (0, 16, 0, 0)       # var, sel, rel, index

CREATE = [
    # a control outside -1 ... n - 1, in each of the six kinds with a member map
    ("clim_control", lambda L: clim(L, 3, [0, 3, 0], abi.C_MEAN), "clim_create: member 1: control = 3 (-1 = none, or 0 ... 2)"),
    ("ens_control", lambda L: ens(L, 3, [0, 0, 0], 1, [0, 0, -2]), "ens_create: member 2: control = -2 (-1 = none, or 0 ... 2)"),
    ("lin_control", lambda L: lin(L, 3, None, [3, 0, 0]), "lin_create: member 0: control = 3 (-1 = none, or 0 ... 2)"),
    ("gram_control", lambda L: gram(L, 2, None, [0, 2]), "gram_create: member 1: control = 2 (-1 = none, or 0 ... 1)"),
    ("cross_control", lambda L: cross(L, 3, [EV], control=[0, -2, 0]), "cross_create: member 1: control = -2 (-1 = none, or 0 ... 2)"),
    ("reg_control", lambda L: reg(L, 2, [TM], control=[0, 5]), "reg_create: member 1: control = 5 (-1 = none, or 0 ... 1)"),
    # (an unused member's control is still looked at, and before a used one's lack of a control)
    ("lin_control_unused", lambda L: lin(L, 3, [1, 1, 0], [-1, 0, 7]), "lin_create: member 0 is used but has no control (control = -1) while a control map is given"),
    ("gram_control_unused", lambda L: gram(L, 3, [0, 1, 1], [9, 0, 0]), "gram_create: member 0: control = 9 (-1 = none, or 0 ... 2)"),
    # the used members of lin and gram
    ("lin_used_no_control", lambda L: lin(L, 3, [0, 1, 1], [-1, 0, -1]), "lin_create: member 2 is used but has no control (control = -1) while a control map is given"),
    ("gram_used_no_control", lambda L: gram(L, 3, None, [0, -1, 0]), "gram_create: member 1 is used but has no control (control = -1) while a control map is given"),
    ("lin_no_used", lambda L: lin(L, 2, [0, 0], None), "lin_create: no used member (`use` is zero everywhere)"),
    ("gram_no_used", lambda L: gram(L, 3, [0, 0, 0], [-1, -1, -1]), "gram_create: no used member (`use` is zero everywhere)"),
    # the groups of ens and cross
    ("ens_group_range", lambda L: ens(L, 3, [0, 2, 1], 2, None), "ens_create: member 1: group = 2 (-1 = none, or 0 ... 1)"),
    ("ens_group_empty", lambda L: ens(L, 3, [0, -1, 0], 2, None), "ens_create: group 1 is empty"),
    ("ens_group_before_control", lambda L: ens(L, 3, [0, -2, 0], 1, [9, 0, 0]), "ens_create: member 0: control = 9 (-1 = none, or 0 ... 2)"),
    ("ens_grouped_no_control", lambda L: ens(L, 3, [0, -1, 0], 1, [0, -1, -1]), "ens_create: member 2 is in group 0 but has no control (control = -1) while a control map is given"),
    ("ens_n_groups", lambda L: ens(L, 3, [0, 0, 0], 65, None), "ens_create: n_groups = 65 (1 ... 64)"),
    ("cross_group_range", lambda L: cross(L, 3, [EV], group=[0, -2, 0], ng=1), "cross_create: member 1: group = -2 (-1 = none, or 0 ... 0)"),
    ("cross_group_empty", lambda L: cross(L, 3, [EV], group=[1, 1, -1], ng=2), "cross_create: group 0 is empty"),
    ("cross_n_groups", lambda L: cross(L, 3, [EV], group=[0, 0, 0], ng=0), "cross_create: n_groups = 0 (1 ... 64)"),
    ("cross_control_before_group", lambda L: cross(L, 2, [EV], control=[2, 0], group=[5, 0], ng=1), "cross_create: member 0: control = 2 (-1 = none, or 0 ... 1)"),
    # the items of cross and reg
    ("cross_var", lambda L: cross(L, 2, [EV, (2, 0, 0, 1, 1.0)]), "cross_create: event 1: var = 2 (0 ... 1)"),
    ("cross_sel", lambda L: cross(L, 2, [(0, 17, 0, 1, 1.0)]), "cross_create: event 0: sel = 17" + SEL),
    ("cross_rel", lambda L: cross(L, 2, [EV, (1, 12, 1, -1, 1.0)]), "cross_create: event 1: rel = 1 (member minus its control) but `control` is NULL"),
    ("reg_var", lambda L: reg(L, 2, [(-1, 0, 0, 0)]), "reg_create: term 0: var = -1 (0 ... 1)"),
    ("reg_sel", lambda L: reg(L, 2, [TM, (1, -1, 0, 0)]), "reg_create: term 1: sel = -1" + SEL),
    ("reg_rel", lambda L: reg(L, 2, [(1, 3, 1, 0)]), "reg_create: term 0: rel = 1 (member minus its control) but `control` is NULL"),
    ("reg_index", lambda L: reg(L, 2, [TM, (0, 0, 0, 1)]), "reg_create: term 1: index = 1 (0 ... 0)"),
    ("reg_index_var", lambda L: reg(L, 2, [TM], indices=[(2, 0, 0, 0)]), "reg_create: index 0: var = 2 (0 ... 1)"),
    ("reg_index_rel", lambda L: reg(L, 2, [TM], indices=[(0, 0, 1, 0)]), "reg_create: term 0: its index 0 has rel = 1 (member minus its control) but `control` is NULL"),
    # what every create says first
    ("clim_members", lambda L: clim(L, 0, None, abi.C_MEAN), "clim_create: n_members = 0"),
    ("ens_members", lambda L: ens(L, 0, [0], 1, None), "ens_create: n_members = 0"),
    ("lin_members", lambda L: lin(L, 0, None, None), "lin_create: n_members = 0"),
    ("gram_members", lambda L: gram(L, -1, None, None), "gram_create: n_members = -1"),
    ("cross_members", lambda L: cross(L, 0, [EV]), "cross_create: n_members = 0"),
    ("reg_members", lambda L: reg(L, 0, [TM]), "reg_create: n_members = 0 (1 ... 65535)"),
    ("clim_out", lambda L: (L.greb_clim_create(C.c_int(NX), C.c_int(NY), C.c_int(1), None, C.c_uint(1), None), None), "clim_create: `out` is NULL"),
    ("ens_out", lambda L: (L.greb_ens_create(NX, NY, 1, _i32([0]), 1, None, None, 0, 1, None), None), "ens_create: `out` is NULL"),
    ("lin_out", lambda L: (L.greb_lin_create(NX, NY, 1, _f64([1.0]), 1, None, None, None, 1, None), None), "lin_create: `out` is NULL"),
    ("gram_out", lambda L: (L.greb_gram_create(NX, NY, 1, 1, _i32([0]), 1, None, None, None, None), None), "gram_create: `out` is NULL"),
    ("cross_out", lambda L: (L.greb_cross_create(NX, NY, 1, 2, None, 1, None, None, 0, 1, None), None), "cross_create: `out` is NULL"),
    ("reg_out", lambda L: (L.greb_reg_create(NX, NY, 1, 2, None, 0, None, None, 1, None, 1, 1, None), None), "reg_create: `out` is NULL"),
]


@pytest.mark.parametrize("fn,want", [c[1:] for c in CREATE], ids=[c[0] for c in CREATE])
def test_create_is_refused_with_exactly_this_text(lib, fn, want):
    rc, h = fn(lib)
    assert rc == -1 and (h is None or h.value is None), rc
    assert lib.greb_engine_last_error(None).decode() == want


# ---- calls on a plan that exists: the products without a pointer, a misaligned one, the period's years
@pytest.fixture(scope="module")
def plans(lib):
    made = {
        "diag": VP(),
        "clim": clim(lib, 2, [-1, 0], abi.C_MEAN | abi.C_SEASONS | abi.C_TREND | abi.C_RESPONSE)[1],
        "clim_mean": clim(lib, 2, None, abi.C_MEAN)[1],
        "ens": ens(lib, 3, [0, 0, 1], 2, None, what=abi.S_MEAN | abi.S_VAR | abi.S_RANGE)[1],
        "lin": lin(lib, 2, None, None, what=abi.L_COEF | abi.L_RSS)[1],
        "gram": gram(lib, 2, None, None, n_records=60)[1],
        "cross": cross(lib, 2, [EV], group=[0, 0], ng=1, what=63, n_vars=5)[1],
        "cross_count": cross(lib, 2, [EV], what=abi.T_COUNT, n_vars=5)[1],
        "reg": reg(lib, 2, [TM], what=15, n_vars=5)[1],
        "reg_slope": reg(lib, 2, [TM], what=abi.R_SLOPE, n_vars=5)[1],
    }
    assert lib.greb_diag_create(C.c_int(NX), C.c_int(NY), None, C.c_int(0), C.byref(made["diag"])) == 0
    assert all(h.value for h in made.values())
    yield made
    for k, h in made.items():
        assert getattr(lib, f"greb_{k.split('_')[0]}_destroy")(h) == 0


def _with(n, i, v):
    p = [OK] * n
    p[i] = v
    return p


def _dev_cases():
    out = []
    i0, i1 = C.c_int(0), C.c_int(1)
    # clim_finish_dev(plan, device, n_years, mean, seasons, trend, mean_resp, seasons_resp, stream)
    names = ("mean", "seasons", "trend", "mean_resp", "seasons_resp")
    flags = ("GREB_C_MEAN", "GREB_C_SEASONS", "GREB_C_TREND", "GREB_C_RESPONSE with GREB_C_MEAN", "GREB_C_RESPONSE with GREB_C_SEASONS")
    for i, (n, f) in enumerate(zip(names, flags)):
        out.append((f"clim_finish_{n}_null", lambda L, P, i=i: L.greb_clim_finish_dev(P["clim"], i0, i1, *_with(5, i, None), None),
                    f"clim_finish_dev: {f} selected but `{n}_dev` is NULL"))
    out.append(("clim_finish_trend_misaligned", lambda L, P: L.greb_clim_finish_dev(P["clim"], i0, i1, *_with(5, 2, BAD), None),
                "clim_finish_dev: trend_dev is not 16-byte aligned"))
    out.append(("clim_finish_unselected_ignored", lambda L, P: L.greb_clim_finish_dev(P["clim_mean"], i0, i1, OK, None, BAD, None, None, None),
                "clim_finish_dev: n_years = 1, but 0 years were added since the last finish"))
    out.append(("clim_finish_fresh", lambda L, P: L.greb_clim_finish_dev(P["clim"], i0, i1, *[OK] * 5, None),
                "clim_finish_dev: n_years = 1, but 0 years were added since the last finish"))
    out.append(("clim_finish_zero_years", lambda L, P: L.greb_clim_finish_dev(P["clim"], i0, i0, *[OK] * 5, None),
                "clim_finish_dev: n_years = 0, but 0 years were added since the last finish"))
    out.append(("clim_add_fresh", lambda L, P: L.greb_clim_add_year_dev(P["clim"], i0, OK, i1, None),
                "clim_add_year_dev: k = 1, but 0 years were added since the last finish (years go in ascending order, k = 0 first)"))
    out.append(("clim_add_misaligned", lambda L, P: L.greb_clim_add_year_dev(P["clim"], i0, BAD, i0, None),
                "clim_add_year_dev: monthly_year_dev is not 16-byte aligned"))
    # ens_reduce_dev(plan, device, x, n, mean, var, min, max, quant, stream)
    for i, (n, f) in enumerate(zip(("mean", "var", "min", "max"), ("GREB_S_MEAN", "GREB_S_VAR", "GREB_S_RANGE", "GREB_S_RANGE"))):
        out.append((f"ens_reduce_{n}_null", lambda L, P, i=i: L.greb_ens_reduce_dev(P["ens"], 0, OK, 4, *_with(5, i, None), None),
                    f"ens_reduce_dev: {f} selected but `{n}_dev` is NULL"))
    out.append(("ens_reduce_misaligned", lambda L, P: L.greb_ens_reduce_dev(P["ens"], 0, BAD, 4, *[OK] * 5, None),
                "ens_reduce_dev: x_dev is not 16-byte aligned"))
    # lin_reduce_dev(plan, device, x, n, coef, rss, stream)
    out.append(("lin_reduce_coef_null", lambda L, P: L.greb_lin_reduce_dev(P["lin"], 0, OK, 4, None, OK, None),
                "lin_reduce_dev: GREB_L_COEF selected but `coef_dev` is NULL"))
    out.append(("lin_reduce_rss_null", lambda L, P: L.greb_lin_reduce_dev(P["lin"], 0, OK, 4, OK, None, None),
                "lin_reduce_dev: GREB_L_RSS selected but `rss_dev` is NULL"))
    out.append(("lin_reduce_misaligned", lambda L, P: L.greb_lin_reduce_dev(P["lin"], 0, BAD, 4, OK, OK, None),
                "lin_reduce_dev: x_dev is not 16-byte aligned"))
    # gram_reduce_dev(plan, device, x, len, G, stream)
    out.append(("gram_reduce_null", lambda L, P: L.greb_gram_reduce_dev(P["gram"], 0, OK, 4, None, None), "gram_reduce_dev: G_dev is NULL"))
    out.append(("gram_reduce_misaligned", lambda L, P: L.greb_gram_reduce_dev(P["gram"], 0, OK, 4, BAD, None),
                "gram_reduce_dev: G_dev is not 8-byte aligned"))
    # cross_finish_dev(plan, device, n_years, first, last, stay, count, peak, peak_year, stream)
    names = ("first", "last", "stay", "count", "peak", "peak_year")
    flags = ("GREB_T_FIRST", "GREB_T_LAST", "GREB_T_STAY", "GREB_T_COUNT", "GREB_T_PEAK", "GREB_T_PEAK")
    for i, (n, f) in enumerate(zip(names, flags)):
        out.append((f"cross_finish_{n}_null", lambda L, P, i=i: L.greb_cross_finish_dev(P["cross"], 0, 1, *_with(6, i, None), None),
                    f"cross_finish_dev: {f} selected but `{n}_dev` is NULL"))
    out.append(("cross_finish_misaligned", lambda L, P: L.greb_cross_finish_dev(P["cross"], 0, 1, *_with(6, 5, BAD), None),
                "cross_finish_dev: peak_year_dev is not 16-byte aligned"))
    out.append(("cross_finish_unselected_ignored", lambda L, P: L.greb_cross_finish_dev(P["cross_count"], 0, 1, BAD, None, None, OK, None, None, None),
                "cross_finish_dev: n_years = 1, but 0 years were added since the last finish"))
    out.append(("cross_finish_fresh", lambda L, P: L.greb_cross_finish_dev(P["cross"], 0, 1, *[OK] * 6, None),
                "cross_finish_dev: n_years = 1, but 0 years were added since the last finish"))
    out.append(("cross_add_fraction_null", lambda L, P: L.greb_cross_add_year_dev(P["cross"], 0, OK, 0, None, None),
                "cross_add_year_dev: GREB_T_FRACTION selected but `fraction_dev` is NULL"))
    out.append(("cross_add_fraction_misaligned", lambda L, P: L.greb_cross_add_year_dev(P["cross"], 0, OK, 0, BAD, None),
                "cross_add_year_dev: fraction_dev is not 16-byte aligned"))
    out.append(("cross_add_fresh", lambda L, P: L.greb_cross_add_year_dev(P["cross"], 0, OK, 1, OK, None),
                "cross_add_year_dev: k = 1, but 0 years were added since the last finish (years go in ascending order, k = 0 first)"))
    # reg_finish_dev(plan, device, n_years, slope, intercept, r2, stream)
    for i, (n, f) in enumerate(zip(("slope", "intercept", "r2"), ("GREB_R_SLOPE", "GREB_R_INTERCEPT", "GREB_R_R2"))):
        out.append((f"reg_finish_{n}_null", lambda L, P, i=i: L.greb_reg_finish_dev(P["reg"], 0, 1, *_with(3, i, None), None),
                    f"reg_finish_dev: {f} selected but `{n}_dev` is NULL"))
    out.append(("reg_finish_misaligned", lambda L, P: L.greb_reg_finish_dev(P["reg"], 0, 1, OK, BAD, OK, None),
                "reg_finish_dev: intercept_dev is not 16-byte aligned"))
    out.append(("reg_finish_unselected_ignored", lambda L, P: L.greb_reg_finish_dev(P["reg_slope"], 0, 1, OK, BAD, None, None),
                "reg_finish_dev: n_years = 1, but 0 years were added since the last finish"))
    out.append(("reg_finish_fresh", lambda L, P: L.greb_reg_finish_dev(P["reg"], 0, 1, OK, OK, OK, None),
                "reg_finish_dev: n_years = 1, but 0 years were added since the last finish"))
    out.append(("reg_add_index_null", lambda L, P: L.greb_reg_add_year_dev(P["reg"], 0, OK, 0, None, None),
                "reg_add_year_dev: GREB_R_INDEX selected but `index_dev` is NULL"))
    out.append(("reg_add_fresh", lambda L, P: L.greb_reg_add_year_dev(P["reg"], 0, OK, 1, OK, None),
                "reg_add_year_dev: k = 1, but 0 years were added since the last finish (years go in ascending order, k = 0 first)"))
    out.append(("reg_add_misaligned", lambda L, P: L.greb_reg_add_year_dev(P["reg"], 0, BAD, 0, OK, None),
                "reg_add_year_dev: x_dev is not 16-byte aligned"))
    # diag_reduce_dev(plan, device, monthly, n_members, regions, zonal, annual, stream)
    out.append(("diag_reduce_misaligned", lambda L, P: L.greb_diag_reduce_dev(P["diag"], i0, OK, i1, OK, OK, BAD, None),
                "diag_reduce_dev: annual_dev is not 16-byte aligned"))
    return out


def _run_cases():
    """The scenario runs look at the plan and the outputs before the engine: with no engine at all, the first complaint is
    the missing output, and with every output given, the engine."""
    out = []
    i1, none = C.c_int(1), None
    for i, (n, f) in enumerate(zip(("regions", "zonal", "annual"), ("GREB_D_REGIONS", "GREB_D_ZONAL", "GREB_D_ANNUAL"))):
        out.append((f"run_diag_{n}_null", lambda L, P, i=i: L.greb_engine_run_diag(none, i1, F, P["diag"], C.c_uint(7), *_with(3, i, None), None),
                    f"run_diag: {f} selected but `{n}` is NULL"))
    out.append(("run_diag_engine", lambda L, P: L.greb_engine_run_diag(none, i1, F, P["diag"], C.c_uint(7), OK, OK, OK, None),
                "run_diag: bad argument (engine, years or co2_ppm)"))
    one = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    _keep.append(one)
    names = ("mean", "seasons", "trend", "mean_resp", "seasons_resp")
    flags = ("GREB_C_MEAN", "GREB_C_SEASONS", "GREB_C_TREND", "GREB_C_RESPONSE with GREB_C_MEAN", "GREB_C_RESPONSE with GREB_C_SEASONS")
    for i, (n, f) in enumerate(zip(names, flags)):
        out.append((f"run_clim_{n}_null", lambda L, P, i=i: L.greb_engine_run_clim(none, i1, F, P["clim"], i1, *one, *_with(5, i, None), None),
                    f"run_clim: {f} selected but `{n}` is NULL"))
    out.append(("run_clim_engine", lambda L, P: L.greb_engine_run_clim(none, i1, F, P["clim"], i1, *one, *[OK] * 5, None),
                "run_clim: bad argument (engine or co2_ppm)"))
    out.append(("run_ens_max_null", lambda L, P: L.greb_engine_run_ens(None, 1, F, P["ens"], F, F, F, None, None, None),
                "run_ens: GREB_S_RANGE selected but `max` is NULL"))
    out.append(("run_budget_ens_var_null", lambda L, P: L.greb_engine_run_budget_ens(None, 1, F, None, 0, P["ens"], F, None, F, F, None, None),
                "run_budget_ens: GREB_S_VAR selected but `var` is NULL"))
    out.append(("run_ens_engine", lambda L, P: L.greb_engine_run_ens(None, 1, F, P["ens"], F, F, F, F, None, None),
                "run_ens: bad argument (engine or co2_ppm)"))
    out.append(("run_lin_coef_null", lambda L, P: L.greb_engine_run_lin(None, 1, F, P["lin"], None, F, None),
                "run_lin: GREB_L_COEF selected but `coef` is NULL"))
    out.append(("run_lin_rss_null", lambda L, P: L.greb_engine_run_lin(None, 1, F, P["lin"], F, None, None),
                "run_lin: GREB_L_RSS selected but `rss` is NULL"))
    out.append(("run_lin_engine", lambda L, P: L.greb_engine_run_lin(None, 1, F, P["lin"], F, F, None), "run_lin: bad argument (engine or co2_ppm)"))
    out.append(("run_gram_null", lambda L, P: L.greb_engine_run_gram(None, 1, F, P["gram"], None, None), "run_gram: `G` is NULL"))
    out.append(("run_gram_engine", lambda L, P: L.greb_engine_run_gram(None, 1, F, P["gram"], D, None), "run_gram: bad argument (engine or co2_ppm)"))
    maps = [I, I, I, I, F, I, F]
    names = ("first", "last", "stay", "count", "peak", "peak_year", "fraction")
    flags = ("GREB_T_FIRST", "GREB_T_LAST", "GREB_T_STAY", "GREB_T_COUNT", "GREB_T_PEAK", "GREB_T_PEAK", "GREB_T_FRACTION")
    for i, (n, f) in enumerate(zip(names, flags)):
        a = list(maps)
        a[i] = None
        out.append((f"run_cross_{n}_null", lambda L, P, a=a: L.greb_engine_run_cross(None, 1, F, P["cross"], *a, None),
                    f"run_cross: {f} selected but `{n}` is NULL"))
    out.append(("run_cross_engine", lambda L, P: L.greb_engine_run_cross(None, 1, F, P["cross"], *maps, None),
                "run_cross: bad argument (engine or co2_ppm)"))
    for i, (n, f) in enumerate(zip(("slope", "intercept", "r2", "index"), ("GREB_R_SLOPE", "GREB_R_INTERCEPT", "GREB_R_R2", "GREB_R_INDEX"))):
        a = [F] * 4
        a[i] = None
        out.append((f"run_reg_{n}_null", lambda L, P, a=a: L.greb_engine_run_reg(None, 1, F, P["reg"], *a, None),
                    f"run_reg: {f} selected but `{n}` is NULL"))
    out.append(("run_reg_engine", lambda L, P: L.greb_engine_run_reg(None, 1, F, P["reg"], F, F, F, F, None), "run_reg: bad argument (engine or co2_ppm)"))
    return out


CALLS = _dev_cases() + _run_cases()


@pytest.mark.parametrize("fn,want", [c[1:] for c in CALLS], ids=[c[0] for c in CALLS])
def test_call_is_refused_with_exactly_this_text(lib, plans, fn, want):
    assert fn(lib, plans) == -1
    assert lib.greb_engine_last_error(None).decode() == want
