"""CPU: the crossing interface (include/greb_engine.h: greb_cross_*, greb_engine_run_cross) -- its symbols, its kernels in
the built library, its argument errors (all reported before any device query) -- and the numpy mirror cross.reference on
hand-made series whose answers are written out here.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, clim, cross, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("greb_cross_create", "greb_cross_destroy", "greb_cross_add_year_dev", "greb_cross_finish_dev", "greb_engine_run_cross",
       "greb_engine_run_budget_cross")
NX, NY = 12, 5


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
    for name in ("FIRST", "LAST", "STAY", "COUNT", "PEAK", "FRACTION"):
        assert re.search(rf"#define GREB_T_{name}\s+{getattr(abi, 'T_' + name)}u", code), name
    assert re.search(rf"#define GREB_CROSS_MAX_EVENTS\s+{abi.CROSS_MAX_EVENTS}\b", code) and abi.CROSS_MAX_EVENTS == 16
    assert C.sizeof(abi.GrebCrossEvent) == 20
    assert (cross.JAN, cross.DEC, cross.DJF, cross.MAM, cross.JJA, cross.SON, cross.ANN) == (0, 11, 12, 13, 14, 15, 16)
    text = " ".join(hdr.split())
    assert "ONE fp32 subtraction (the greb_ens convention)" in text and "24 bytes" in text and "906 MB" in text
    assert cross.memory_bytes(cross.MAPS, 512, 16, 48, 96) == 24 * 512 * 16 * 4608  # 906 MB
    assert cross.memory_bytes(abi.T_FIRST | abi.T_FRACTION, 2, 3, 48, 96, n_groups=1) == (4 + 1) * 2 * 3 * 4608 + 8 * 3 * 4608


def test_library_has_the_cross_kernels_for_gfx950(lib):
    from greb_climate_model_amd import codesha
    assert "greb_cross.hip" in build.SOURCES and "greb_cross.h" in build.HEADERS
    assert build.EXTRA_FLAGS["greb_cross.hip"] == build.EXTRA_FLAGS["greb_clim.hip"] == ["-ffp-contract=off"]
    for name, n in (("cross_update_kernel", 2), ("cross_fraction_kernel", 1), ("cross_finish_kernel", 1)):
        got = codesha.kernel_functions(build.LIB, name)
        assert len(got) == n and all(len(c) > 64 for c in got.values()), (name, sorted(got))


# ---- argument errors -------------------------------------------------------------------------------------------------
def _err(fn, code=-1):
    with pytest.raises(engine.GrebError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_plan_argument_errors_name_the_offender(lib):
    E = cross.Event
    ok = [E(0, cross.ANN, 1.5)]
    P = lambda nm, ev, **k: cross.Plan(96, 48, nm, ev, **k)
    P(3, ok).close()
    P(3, [E(4, cross.SEP, 0.4, dir=-1, rel=True)] * 16, control=[1, 1, -1], group=[0, -1, 1]).close()
    for gx, gy in ((95, 48), (8, 48), (96, 4), (96, 193)):  # the grids diag.Plan rejects
        assert f"grid {gx} x {gy}" in _err(lambda: cross.Plan(gx, gy, 1, ok))
    assert "n_members = 0" in _err(lambda: P(0, ok))
    assert "n_vars = 0" in _err(lambda: P(1, ok, n_vars=0))
    assert "n_vars = 17" in _err(lambda: P(1, ok, n_vars=17))
    assert "n_events = 0" in _err(lambda: P(1, []))
    assert "n_events = 17" in _err(lambda: P(1, ok * 17))
    assert "`what` = 0" in _err(lambda: P(1, ok, what=0))
    assert "`what` = 64" in _err(lambda: P(1, ok, what=64))
    msg = _err(lambda: P(1, ok + [E(5, 0, 1.0)]))
    assert "event 1" in msg and "var = 5" in msg, msg
    msg = _err(lambda: P(1, ok + [E(-1, 0, 1.0)]))
    assert "event 1" in msg and "var = -1" in msg, msg
    P(1, [E(12, 0, 1.0)], n_vars=13).close()
    msg = _err(lambda: P(1, ok * 2 + [E(0, 17, 1.0)]))
    assert "event 2" in msg and "sel = 17" in msg, msg
    msg = _err(lambda: P(1, [E(0, -1, 1.0)]))
    assert "event 0" in msg and "sel = -1" in msg, msg
    for bad in (0, 2, -2):
        msg = _err(lambda: P(1, ok + [E(0, 0, 1.0, dir=bad)]))
        assert "event 1" in msg and f"dir = {bad}" in msg, msg
    for bad in (np.nan, np.inf, -np.inf):
        msg = _err(lambda: P(1, [E(0, 0, bad)]))
        assert "event 0" in msg and "thr" in msg and "not finite" in msg, msg
    msg = _err(lambda: P(2, ok + [E(0, 0, 1.0, rel=True)]))
    assert "event 1" in msg and "rel = 1" in msg and "`control` is NULL" in msg, msg
    msg = _err(lambda: P(2, [E(0, 0, 1.0, rel=2)], control=[0, 0]))
    assert "event 0" in msg and "rel = 2" in msg, msg
    msg = _err(lambda: P(3, ok, control=[0, 3, 0]))
    assert "member 1" in msg and "control = 3" in msg, msg
    msg = _err(lambda: P(3, ok, control=[0, 0, -2]))
    assert "member 2" in msg and "control = -2" in msg, msg
    msg = _err(lambda: P(3, ok, what=abi.T_FRACTION))
    assert "GREB_T_FRACTION" in msg and "`group` is NULL" in msg, msg
    msg = _err(lambda: P(3, ok, group=[0, 2, 0], n_groups=2))
    assert "member 1" in msg and "group = 2" in msg, msg
    assert "group 1 is empty" in _err(lambda: P(3, ok, group=[0, 2, 0]))
    assert "n_groups = 0" in _err(lambda: P(3, ok, group=[-1, -1, -1]))
    assert "n_groups = 65" in _err(lambda: P(65, ok, group=list(range(65))))
    assert "3 integers" in _err(lambda: P(3, ok, control=[0, 0]))
    assert "3 integers" in _err(lambda: P(3, ok, group=[0, 0]))
    h = C.c_void_p()
    ev = (abi.GrebCrossEvent * 1)()
    ev[0].dir = 1
    assert lib.greb_cross_create(96, 48, 1, 5, ev, 1, None, None, 0, 1, None) == -1
    assert lib.greb_cross_create(96, 48, 1, 5, None, 1, None, None, 0, 1, C.byref(h)) == -1
    assert "`events` NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_cross_destroy(None) == 0
    p = P(512, ok * 16)
    assert "906.0 MB" in p.describe()
    p.close()


def _aligned():
    buf = np.zeros(64, np.float32)
    return buf, C.c_void_p((buf.ctypes.data + 15) & ~15)


def test_dev_argument_errors_come_before_any_device_query(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, ok = _aligned()
    bad = C.c_void_p(ok.value + 4)
    plan = cross.Plan(96, 48, 2, [cross.Event(0, 0, 1.0)], group=[0, 0])  # all six products
    maps = cross.Plan(96, 48, 2, [cross.Event(0, 0, 1.0)], what=abi.T_COUNT)
    add, fin = lib.greb_cross_add_year_dev, lib.greb_cross_finish_dev
    assert add(None, 0, ok, 0, ok, None) == -1 and "cross_add_year_dev: no plan" in last()
    assert add(plan.h, 0, None, 0, ok, None) == -1 and "x_dev is NULL" in last()
    assert add(plan.h, 0, bad, 0, ok, None) == -1 and "x_dev is not 16-byte aligned" in last()
    assert add(plan.h, 0, ok, 0, None, None) == -1 and "GREB_T_FRACTION selected but `fraction_dev` is NULL" in last()
    assert add(plan.h, 0, ok, 0, bad, None) == -1 and "fraction_dev is not 16-byte aligned" in last()
    assert add(plan.h, 0, ok, 1, ok, None) == -1 and "k = 1, but 0 years were added" in last()
    assert add(maps.h, 0, ok, 2, bad, None) == -1 and "k = 2, but 0 years" in last()  # (an unselected pointer is ignored)
    assert fin(None, 0, 1, *[ok] * 6, None) == -1 and "cross_finish_dev: no plan" in last()
    names = ("first", "last", "stay", "count", "peak", "peak_year")
    flags = ("GREB_T_FIRST", "GREB_T_LAST", "GREB_T_STAY", "GREB_T_COUNT", "GREB_T_PEAK", "GREB_T_PEAK")
    for i, (name, flag) in enumerate(zip(names, flags)):
        p = [ok] * 6
        p[i] = None
        assert fin(plan.h, 0, 1, *p, None) == -1 and f"{flag} selected but `{name}_dev` is NULL" in last(), last()
        p[i] = bad
        assert fin(plan.h, 0, 1, *p, None) == -1 and f"{name}_dev is not 16-byte aligned" in last(), last()
    assert fin(plan.h, 0, 1, *[ok] * 6, None) == -1 and "n_years = 1, but 0 years were added" in last()
    assert fin(maps.h, 0, 0, None, None, None, ok, None, None, None) == -1 and "n_years = 0" in last()
    assert fin(maps.h, 0, 1, bad, None, bad, None, None, None, None) == -1 and "`count_dev` is NULL" in last()
    plan.close(); maps.close()


def test_run_cross_argument_errors_are_decided_without_an_engine(lib):
    """The plan, the variable count, the years and the outputs are looked at before the engine is: no device is needed."""
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, _ = _aligned()
    p = abi.fptr(buf)
    i = np.zeros(64, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    ev = [cross.Event(0, cross.ANN, 1.0)]
    plan = cross.Plan(96, 48, 2, ev, group=[0, 0])
    thirteen = cross.Plan(96, 48, 2, ev, n_vars=13, what=abi.T_FIRST)
    two = cross.Plan(96, 48, 2, ev, n_vars=2, what=abi.T_STAY | abi.T_FRACTION, group=[0, -1])
    run, brun = lib.greb_engine_run_cross, lib.greb_engine_run_budget_cross
    good = (i, i, i, i, p, i, p)
    assert run(None, 1, p, None, *good, None) == -1 and "run_cross: no plan" in last()
    assert run(None, 1, p, thirteen.h, *good, None) == -1 and "n_vars = 13" in last() and "5 variables" in last(), last()
    assert run(None, 0, p, plan.h, *good, None) == -1 and "years = 0" in last()
    names = ("first", "last", "stay", "count", "peak", "peak_year", "fraction")
    flags = ("GREB_T_FIRST", "GREB_T_LAST", "GREB_T_STAY", "GREB_T_COUNT", "GREB_T_PEAK", "GREB_T_PEAK", "GREB_T_FRACTION")
    for k, (name, flag) in enumerate(zip(names, flags)):
        a = list(good)
        a[k] = None
        assert run(None, 1, p, plan.h, *a, None) == -1 and f"run_cross: {flag} selected but `{name}` is NULL" in last(), last()
    assert run(None, 1, p, plan.h, *good, None) == -1 and "bad argument (engine" in last()
    # the budget route: the thirteen terms want n_vars = 13, a combination of two n_vars = 2
    assert brun(None, 1, p, None, 0, plan.h, *good, None) == -1 and "run_budget_cross" in last() and "13 variables" in last(), last()
    assert brun(None, 1, p, None, 0, thirteen.h, None, None, None, None, None, None, None, None) == -1 and "`first` is NULL" in last()
    assert brun(None, 1, p, None, 0, thirteen.h, i, None, None, None, None, None, None, None) == -1 and "bad argument (engine" in last()
    combo = np.zeros((2, abi.NBUDGET), np.float32)
    combo[0, 0] = combo[1, 1] = 1
    assert brun(None, 1, p, abi.fptr(combo), 2, thirteen.h, *good, None) == -1 and "2 variables" in last(), last()
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, None, None, i, None, None, None, None, None) == -1 and "`fraction` is NULL" in last()
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, None, None, i, None, None, None, p, None) == -1 and "bad argument (engine" in last()
    combo[1] = 0
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, *good, None) == -1 and "combo row 1 is zero" in last(), last()
    for x in (plan, thirteen, two):
        x.close()


def test_dev_call_without_a_gpu_is_a_loud_error(lib):
    import torch
    buf, ok = _aligned()
    plan = cross.Plan(96, 48, 1, [cross.Event(0, 0, 1.0)], what=abi.T_FIRST)
    if not torch.cuda.is_available():
        assert lib.greb_cross_add_year_dev(plan.h, 0, ok, 0, None, None) == -2
        assert b"no CPU path" in lib.greb_engine_last_error(None)
    plan.close()


# ---- the mirror on hand-made series ----------------------------------------------------------------------------------
def _series(values, n_members=1, var=0, month=0, n_vars=2):
    """Six years [6][n_members][12][n_vars][NY][NX] that hold 100 everywhere but `values` [6] (or [6][n_members]) in
    (var, month) at every point."""
    x = np.full((6, n_members, 12, n_vars, NY, NX), 100.0, np.float32)
    v = np.asarray(values, np.float32).reshape(6, -1)
    x[:, :, month, var] = np.broadcast_to(v, (6, n_members))[:, :, None, None]
    return x


def _one(res, name, m=0, e=0):
    a = getattr(res, name)[m, e]
    assert (a == a[0, 0]).all() or np.isnan(a).all(), name
    return a[0, 0]


def test_mirror_on_hand_made_series():
    E = cross.Event
    up = [E(0, cross.JAN, 5.0)]
    # crosses in year 2, falls back in year 4, crosses again in year 5
    r = cross.reference(_series([1, 2, 6, 7, 3, 8]), up)
    assert [_one(r, n) for n in ("first", "last", "stay", "count", "peak_year")] == [2, 5, 5, 3, 5] and _one(r, "peak") == 8
    assert all(getattr(r, n).dtype == np.int32 for n in ("first", "last", "stay", "count", "peak_year")) and r.peak.dtype == np.float32
    assert r.first.shape == (1, 1, NY, NX) and r.fraction is None
    # never crosses: -1 throughout, no hits; the peak is still the largest year
    r = cross.reference(_series([1, 2, 4, 3, 2, 1]), up)
    assert [_one(r, n) for n in ("first", "last", "stay", "count", "peak_year")] == [-1, -1, -1, 0, 2] and _one(r, "peak") == 4
    # always crosses: stay 0
    r = cross.reference(_series([6, 7, 8, 9, 8, 7]), up)
    assert [_one(r, n) for n in ("first", "last", "stay", "count", "peak_year")] == [0, 5, 0, 6, 3]
    # the last year misses: stay -1
    r = cross.reference(_series([6, 7, 8, 9, 8, 4]), up)
    assert [_one(r, n) for n in ("first", "last", "stay", "count")] == [0, 4, -1, 5]
    # q == thr hits in both directions; below, a tie of the minimum keeps the earlier year
    x = _series([4, 5, 6, 5, 4, 6])
    r = cross.reference(x, [E(0, cross.JAN, 5.0), E(0, cross.JAN, 5.0, dir=-1)])
    assert [_one(r, n, e=0) for n in ("first", "last", "stay", "count", "peak_year")] == [1, 5, 5, 4, 2]  # 6 in years 2 and 5
    assert [_one(r, n, e=1) for n in ("first", "last", "stay", "count", "peak_year")] == [0, 4, -1, 4, 0]  # 4 in years 0 and 4
    assert _one(r, "peak", e=0) == 6 and _one(r, "peak", e=1) == 4
    # a NaN year is a miss and does not become the peak; a NaN in year 0 is replaced
    r = cross.reference(_series([np.nan, 6, np.nan, 7, 7, np.nan]), up)
    assert [_one(r, n) for n in ("first", "last", "stay", "count", "peak_year")] == [1, 4, -1, 3, 3] and _one(r, "peak") == 7
    r = cross.reference(_series([np.nan] * 6), up)
    assert [_one(r, n) for n in ("first", "last", "stay", "count", "peak_year")] == [-1, -1, -1, 0, 0] and np.isnan(_one(r, "peak"))
    # the season selectors read the other months: every month 100 but January -> ANN = (31 v + 334 * 100) / 365
    r = cross.reference(_series([100, 100, 465, 100, 465, 465]), [E(0, cross.ANN, 131.0), E(0, cross.DJF, 225.0), E(0, cross.JJA, 100.5),
                                                                  E(1, cross.ANN, 100.0, dir=-1)])
    assert [_one(r, n, e=0) for n in ("first", "last", "stay", "count")] == [2, 5, 4, 3]      # 131 exactly in the crossing years
    assert [_one(r, n, e=1) for n in ("first", "last", "stay", "count")] == [2, 5, 4, 3]      # DJF = (5900 + 31 * 465) / 90 = 225.7
    assert [_one(r, n, e=2) for n in ("first", "count")] == [-1, 0]                           # June ... August never move
    assert [_one(r, n, e=3) for n in ("first", "stay", "count")] == [0, 0, 6]                 # the other variable stays at 100


def test_mirror_rel_events_and_controls():
    E = cross.Event
    # member 0 has no control, member 1 is its own control, member 2 minus member 0
    v = np.array([[1, 9, 1], [1, 9, 3], [1, 9, 4], [1, 9, 2], [1, 9, 4], [1, 9, 0]], np.float32)
    x = _series(v, n_members=3)
    r = cross.reference(x, [E(0, cross.JAN, 0.0, rel=True), E(0, cross.JAN, 2.0, rel=True)], control=[-1, 1, 0])
    for e in (0, 1):  # NaN / -1 / 0
        assert [_one(r, n, m=0, e=e) for n in ("first", "last", "stay", "count", "peak_year")] == [-1, -1, -1, 0, 0]
        assert np.isnan(_one(r, "peak", m=0, e=e))
    assert [_one(r, n, m=1, e=0) for n in ("first", "last", "stay", "count", "peak_year")] == [0, 5, 0, 6, 0]  # +0 hits >= 0
    p = _one(r, "peak", m=1, e=0)
    assert p == 0 and not np.signbit(p)
    assert [_one(r, n, m=1, e=1) for n in ("first", "count")] == [-1, 0]
    assert [_one(r, n, m=2, e=0) for n in ("first", "last", "stay", "count")] == [0, 4, -1, 5]   # 0 2 3 1 3 -1
    assert [_one(r, n, m=2, e=1) for n in ("first", "last", "stay", "count", "peak_year")] == [1, 4, -1, 3, 2] and _one(r, "peak", m=2, e=1) == 3
    with pytest.raises(ValueError):
        cross.reference(x, [E(0, 0, 0.0, rel=True)])


def test_season_quantity_has_the_bits_of_a_one_year_climatology():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((1, 3, 12, 4, NY, NX)) * 20 + 270).astype(np.float32)
    sea = clim.reference(x[:1], what=abi.C_SEASONS).seasons  # [3][5 seasons][4][NY][NX]
    for s, sel in enumerate((cross.DJF, cross.MAM, cross.JJA, cross.SON, cross.ANN)):
        for var in range(4):
            q = cross.quantity(x[0], cross.Event(var, sel, 0.0))
            assert q.dtype == np.float32 and np.array_equal(q.view(np.uint32), sea[:, s, var].view(np.uint32)), (sel, var)
    # ... and the peak of a one-year run is that quantity
    r = cross.reference(x, [cross.Event(2, cross.SON, 270.0)])
    assert np.array_equal(r.peak[:, 0].view(np.uint32), sea[:, 3, 2].view(np.uint32))


def test_fraction_of_groups_equals_the_hand_count():
    # nine members: group 0 = {0}, group 1 = {2, 5}, group 2 = {1, 3, 4, 6, 7}, member 8 in none
    group = [0, 2, 1, 2, 2, 1, 2, 2, -1]
    v = np.zeros((6, 9), np.float32)
    v[1, [0, 2, 1]] = 9          # year 1: group 0 1/1, group 1 1/2, group 2 1/5
    v[2, [5, 2, 3, 4, 6, 8]] = 9  # year 2: 0/1, 2/2, 3/5 (member 8 counts nowhere)
    v[3] = 9                     # year 3: everyone
    v[4, [1, 3, 4, 6]] = 9       # year 4: 0, 0, 4/5
    r = cross.reference(_series(v, n_members=9), [cross.Event(0, cross.JAN, 5.0), cross.Event(0, cross.JAN, 5.0, dir=-1)], group=group)
    assert r.fraction.shape == (6, 3, 2, NY, NX) and r.fraction.dtype == np.float32
    f32 = lambda a, b: np.float32(np.float64(a) / np.float64(b))
    want = np.array([[0, 0, 0], [1, f32(1, 2), f32(1, 5)], [0, 1, f32(3, 5)], [1, 1, 1], [0, 0, f32(4, 5)], [0, 0, 0]], np.float32)
    assert np.array_equal(r.fraction[:, :, 0], np.broadcast_to(want[:, :, None, None], (6, 3, NY, NX)))
    below = np.array([[1, 1, 1], [0, f32(1, 2), f32(4, 5)], [1, 0, f32(2, 5)], [0, 0, 0], [1, 1, f32(1, 5)], [1, 1, 1]], np.float32)
    assert np.array_equal(r.fraction[:, :, 1], np.broadcast_to(below[:, :, None, None], (6, 3, NY, NX)))
    with pytest.raises(ValueError):
        cross.reference(_series(v, n_members=9), [cross.Event(0, 0, 5.0)], group=[0, 2] + [0] * 7)


def test_as_year_is_exact():
    a = np.array([[-1, 0, 7], [99, -1, 2]], np.int32)
    y = cross.as_year(a, 1940)
    assert y.dtype == np.float32 and np.isnan(y[0, 0]) and np.isnan(y[1, 1])
    assert np.array_equal(y[~np.isnan(y)], np.array([1940, 1947, 2039, 1942], np.float32))
    c = cross.as_year(a, 0, never=100)
    assert c.dtype == np.float32 and np.array_equal(c, np.array([[100, 0, 7], [99, 100, 2]], np.float32))
    assert np.array_equal(cross.as_year(np.array([16777215], np.int32)), np.array([16777215], np.float32))
    with pytest.raises(ValueError):
        cross.as_year(np.array([1.0]))
