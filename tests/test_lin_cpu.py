"""CPU: the linear-model interface (include/greb_engine.h: greb_lin_*, greb_engine_run_lin) -- its symbols, its kernels in
the built library, its argument errors (all reported before any device query) -- and the numpy mirror lin.reference on
cases whose answer is known.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, engine, ens, ensemble, lin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("greb_lin_create", "greb_lin_destroy", "greb_lin_reduce_dev", "greb_engine_run_lin")


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
    for name, val in (("GREB_L_COEF", abi.L_COEF), ("GREB_L_RSS", abi.L_RSS)):
        assert re.search(rf"#define {name}\s+{val}u", code), name
    assert re.search(rf"#define GREB_LIN_MAX_TERMS\s+{abi.LIN_MAX_TERMS}\b", code)
    assert (abi.L_COEF, abi.L_RSS, abi.LIN_MAX_TERMS) == (1, 2, 64)
    assert lin.PRODUCTS == ("coef", "rss")


def test_library_has_the_linear_model_kernels_for_gfx950(lib):
    from greb_climate_model_amd import codesha
    assert "greb_lin.hip" in build.SOURCES and "greb_lin.h" in build.HEADERS
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["greb_lin.hip"]  # the operation order is the definition of the results
    co = codesha.kernel_functions(build.LIB, "lin_coef_kernel")
    assert len(co) == 4 and all(len(c) > 64 for c in co.values()), sorted(co)  # {no control, control} x {8-byte, scalar}
    rs = codesha.kernel_functions(build.LIB, "lin_rss_kernel")
    assert len(rs) == 8 and all(len(c) > 64 for c in rs.values()), sorted(rs)  # {no control, control} x {16, 32, 48, 64 terms}


# ---- argument errors -------------------------------------------------------------------------------------------------
def _err(fn, code=-1):
    with pytest.raises(engine.GrebError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_plan_argument_errors_name_the_offender(lib):
    nx, ny = 96, 48
    P = lambda *a, **k: lin.Plan(nx, ny, *a, **k)
    w3 = np.full((2, 3), 0.5)
    d3 = np.ones((3, 2))
    P(3, w3).close()
    P(3, w3, design=d3).close()
    P(3, w3, use=[1, 0, 1], control=[0, -1, 2], design=d3).close()  # a member may be its own control; an unused one needs none
    P(1, [[1.0]]).close()
    for gx, gy in ((95, 48), (8, 48), (96, 4), (96, 193)):  # the grids diag.Plan rejects
        assert f"grid {gx} x {gy}" in _err(lambda: lin.Plan(gx, gy, 1, [[1.0]]))
    assert "n_members = 0" in _err(lambda: P(0, np.zeros((1, 0))))
    assert "n_terms = 0" in _err(lambda: P(3, np.zeros((0, 3))))
    assert "n_terms = 65" in _err(lambda: P(3, np.zeros((65, 3))))
    P(3, np.zeros((64, 3))).close()
    assert "`what` = 0" in _err(lambda: P(3, w3, what=0))
    assert "`what` = 4" in _err(lambda: P(3, w3, what=4))
    assert "`what` = 5" in _err(lambda: P(3, w3, what=abi.L_COEF | 4))
    msg = _err(lambda: P(3, w3, what=abi.L_RSS))
    assert "GREB_L_RSS" in msg and "`design` is NULL" in msg, msg
    msg = _err(lambda: P(3, w3, what=abi.L_COEF | abi.L_RSS))
    assert "GREB_L_RSS" in msg and "`design` is NULL" in msg, msg
    P(3, w3, design=d3, what=abi.L_COEF).close()  # a design without GREB_L_RSS is legal
    assert "no used member" in _err(lambda: P(3, w3, use=[0, 0, 0]))
    msg = _err(lambda: P(3, w3, control=[0, 3, 0]))
    assert "member 1" in msg and "control = 3" in msg, msg
    msg = _err(lambda: P(3, w3, control=[0, 0, -2]))
    assert "member 2" in msg and "control = -2" in msg, msg
    msg = _err(lambda: P(3, w3, use=[0, 1, 0], control=[0, 0, 7]))  # ... of an unused member too
    assert "member 2" in msg and "control = 7" in msg, msg
    msg = _err(lambda: P(3, w3, use=[1, 1, 0], control=[0, -1, -1]))
    assert "member 1" in msg and "no control" in msg, msg
    for bad in (np.nan, np.inf, -np.inf):
        w = w3.copy(); w[1, 2] = bad
        msg = _err(lambda: P(3, w, design=d3))
        assert "weight" in msg and "term 1" in msg and "member 2" in msg and "not finite" in msg, msg
        P(3, w, use=[1, 1, 0], design=d3).close()  # what belongs to an unused member is not looked at
        d = d3.copy(); d[2, 1] = bad
        msg = _err(lambda: P(3, w3, design=d))
        assert "design" in msg and "term 1" in msg and "member 2" in msg and "not finite" in msg, msg
        P(3, w3, use=[1, 1, 0], design=d).close()
    assert "[n_terms][3]" in _err(lambda: P(3, np.zeros((2, 4))))
    assert "[3][2]" in _err(lambda: P(3, w3, design=np.ones((2, 3))))
    assert "3 integers" in _err(lambda: P(3, w3, use=[1, 1]))
    assert "3 integers" in _err(lambda: P(3, w3, control=[0, 0]))
    h = C.c_void_p()
    one = np.ones(1, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    assert lib.greb_lin_create(nx, ny, 1, one, 1, None, None, None, 1, None) == -1
    assert lib.greb_lin_create(nx, ny, 1, None, 1, None, None, None, 1, C.byref(h)) == -1
    assert "`weight` is NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_lin_destroy(None) == 0


def _aligned():
    buf = np.zeros(64, np.float32)
    return buf, C.c_void_p((buf.ctypes.data + 15) & ~15)


def test_dev_argument_errors_come_before_any_device_query(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, ok = _aligned()
    bad = C.c_void_p(ok.value + 4)
    plan = lin.Plan(96, 48, 2, [[0.5, 0.5]], design=[[1.0], [1.0]])
    red = lib.greb_lin_reduce_dev
    assert red(None, 0, ok, 8, ok, ok, None) == -1 and "no plan" in last()
    assert red(plan.h, 0, None, 8, ok, ok, None) == -1 and "x_dev is NULL" in last()
    assert red(plan.h, 0, bad, 8, ok, ok, None) == -1 and "x_dev is not 16-byte aligned" in last()
    assert red(plan.h, 0, ok, 0, ok, ok, None) == -1 and "n = 0" in last()
    assert red(plan.h, 0, ok, 8, None, ok, None) == -1 and "GREB_L_COEF selected but `coef_dev` is NULL" in last(), last()
    assert red(plan.h, 0, ok, 8, ok, None, None) == -1 and "GREB_L_RSS selected but `rss_dev` is NULL" in last(), last()
    plan.close()


def test_run_lin_argument_errors_are_decided_without_an_engine(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, _ = _aligned()
    p = abi.fptr(buf)
    plan = lin.Plan(96, 48, 2, [[0.5, 0.5]], design=[[1.0], [1.0]])
    run = lib.greb_engine_run_lin
    assert run(None, 1, p, None, p, p, None) == -1 and "no plan" in last()
    assert run(None, 0, p, plan.h, p, p, None) == -1 and "years = 0" in last()
    assert run(None, 1, p, plan.h, None, p, None) == -1 and "selected but `coef` is NULL" in last(), last()
    assert run(None, 1, p, plan.h, p, None, None) == -1 and "selected but `rss` is NULL" in last(), last()
    assert run(None, 1, p, plan.h, p, p, None) == -1 and "bad argument (engine" in last()
    only = lin.Plan(96, 48, 2, [[0.5, 0.5]])  # an unselected product may be NULL: the next check is reached
    assert run(None, 1, p, only.h, p, None, None) == -1 and "bad argument (engine" in last()
    plan.close(); only.close()


def test_dev_calls_without_a_gpu_are_a_loud_error(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    buf, ok = _aligned()
    plan = lin.Plan(96, 48, 1, [[1.0]])
    assert lib.greb_lin_reduce_dev(plan.h, 0, ok, 8, ok, None, None) == -2
    assert b"no CPU path" in lib.greb_engine_last_error(None)
    plan.close()


# ---- the mirror on cases with a known answer -------------------------------------------------------------------------
def records(n_members, rec, seed):
    """fp32 data in [220, 310)."""
    rng = np.random.default_rng(seed)
    x = rng.random((n_members,) + tuple(rec), dtype=np.float32) * np.float32(90.0) + np.float32(220.0)
    assert x.dtype == np.float32
    return x


def test_mirror_quarter_weights_are_the_ensemble_mean_bit_for_bit():
    """Weights 1/4 on four used members of six, with a control map: S / 4 of ens.reference is the sum of v / 4, each
    product exact (a power of two) and every partial sum the same multiple of 1/4."""
    x = records(6, (5, 7, 12), seed=1)
    use, control = [1, 0, 1, 1, 0, 1], [1, -1, 4, 3, -1, 0]
    w = np.where(np.asarray(use) != 0, 0.25, np.nan)[None]  # (an unused member's weight is never touched)
    got = lin.reference(x, w, use=use, control=control)
    ref = ens.reference(x, [0 if u else -1 for u in use], control, what=abi.S_MEAN)
    assert got.rss is None and got.coef.dtype == np.float32 and got.coef.shape == (1, 5, 7, 12)
    assert np.array_equal(got.coef[0].view(np.uint32), ref.mean[0].view(np.uint32))
    assert got.coef[0, 0, 3].any()  # member 3 is its own control; the others are not


def test_mirror_saturated_factorial_has_no_residual():
    sw = ensemble.switch_factorial(abi.X_NO_ICE | abi.X_NO_DEEP_OCEAN | abi.X_SST_PLUS1)
    names, w, d = lin.factorial(sw, abi.X_NO_ICE | abi.X_NO_DEEP_OCEAN | abi.X_SST_PLUS1, order=3)
    assert len(sw) == 8 and w.shape == (8, 8) and d.shape == (8, 8)
    x = records(8, (4, 9, 12), seed=2)
    r = lin.reference(x, w, design=d)
    assert r.rss.shape == (4, 9, 12) and not r.rss.any(), "a saturated model reproduces every member exactly"
    np.testing.assert_allclose(r.coef[0], x.astype(np.float64).mean(axis=0), rtol=1e-7)
    ice = names.index("GREB_X_NO_ICE")
    on = (sw & abi.X_NO_ICE) != 0
    half_diff = (x[on].astype(np.float64).mean(axis=0) - x[~on].astype(np.float64).mean(axis=0)) / 2
    np.testing.assert_allclose(r.coef[ice], half_diff, rtol=0, atol=310 * 2.0 ** -23)
    assert lin.reference(x, w[:4], design=d[:, :4]).rss.all()  # ... and an unsaturated one does not


def test_mirror_regression_against_independent_numpy():
    """37 members, 5 predictors and the intercept: every coefficient within 2^-23 sum_m |w| |v| of the fp64 matrix
    product -- the final fp32 rounding is at most 2^-24 of that sum, the fp64 accumulation negligible beside it."""
    rng = np.random.default_rng(3)
    pred = rng.standard_normal((37, 5))
    names, w, d = lin.regression(pred, ["a", "b", "c", "d", "e"])
    assert names == ["intercept", "a", "b", "c", "d", "e"] and w.shape == (6, 37) and d.shape == (37, 6)
    assert w.dtype == np.float64 and np.array_equal(d[:, 0], np.ones(37)) and np.array_equal(d[:, 1:], pred)
    x = records(37, (11, 13), seed=4)
    r = lin.reference(x, w, design=d)
    x64 = x.astype(np.float64)
    exact = np.einsum("km,m...->k...", w, x64)
    bound = 2.0 ** -23 * np.einsum("km,m...->k...", np.abs(w), np.abs(x64))
    err = np.abs(r.coef.astype(np.float64) - exact)
    print(f"largest error / sum |w||v|: {(err / (bound * 2.0 ** 23)).max():.3g} (2^-24 = {2.0 ** -24:.3g})")
    assert (err <= bound).all()
    fit = np.einsum("mk,k...->m...", d, exact)
    np.testing.assert_allclose(r.rss, ((x64 - fit) ** 2).sum(axis=0), rtol=1e-6)
    names, w, d = lin.regression(pred, list("abcde"), intercept=False)
    assert names == list("abcde") and w.shape == (5, 37)


def test_mirror_products_follow_the_flags():
    x = records(5, (6,), seed=5)
    names, w, d = lin.regression(np.arange(5.0)[:, None], ["t"])
    full = lin.reference(x, w, design=d)
    c, r = lin.reference(x, w, design=d, what=abi.L_COEF), lin.reference(x, w, design=d, what=abi.L_RSS)
    assert c.rss is None and r.coef is None
    assert np.array_equal(c.coef, full.coef) and np.array_equal(r.rss, full.rss)
    assert lin.reference(x, w).rss is None
    with pytest.raises(ValueError):
        lin.reference(x, w, what=abi.L_RSS)


def test_mirror_never_reads_an_unused_member():
    x = records(6, (9,), seed=6)
    use, control = [1, 1, 0, 1, 0, 1], [4, 4, -1, 0, -1, 5]  # member 4 is unused but a control; member 2 is neither
    names, w, d = lin.regression(np.arange(6.0)[:, None] ** 2, ["t2"])
    a = lin.reference(x, w, use=use, control=control, design=d)
    y = x.copy(); y[2] = np.nan
    b = lin.reference(y, w, use=use, control=control, design=d)
    assert np.isfinite(b.coef).all() and np.isfinite(b.rss).all()
    assert np.array_equal(a.coef, b.coef) and np.array_equal(a.rss, b.rss)


def test_factorial_weights_and_names():
    sw = ensemble.switch_factorial()
    names, w, d = lin.factorial(sw, 0xff, order=2)
    assert len(names) == 37 == 1 + 8 + 28 and w.shape == (37, 256) and d.shape == (256, 37)
    assert np.array_equal(np.abs(w), np.full(w.shape, 1.0 / 256)) and np.array_equal(w, d.T / 256)
    assert names[0] == "mean" and (w[0] > 0).all()
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    in_header = {n: int(b) for n, b in re.findall(r"#define (GREB_X_\w+)\s+\(1u << (\d+)\)", hdr)}
    assert len(in_header) == 8 and list(abi.X_NAMES) == sorted(in_header, key=in_header.get)
    assert names[1:9] == list(abi.X_NAMES)
    for k, name in enumerate(names[1:], start=1):
        parts = name.split(":")
        assert all(p in in_header for p in parts) and len(parts) == (1 if k < 9 else 2), name
        sign = np.ones(256)
        for p in parts:
            sign = sign * np.where(sw >> in_header[p] & 1, 1.0, -1.0)
        assert np.array_equal(d[:, k], sign), name
    assert np.array_equal(d.T @ d, 256 * np.eye(37)), "the columns are orthogonal: weight is pinv(design)"
    two = ensemble.switch_factorial(abi.X_NO_ICE | abi.X_NO_HYDRO)
    names, w, d = lin.factorial(two, abi.X_NO_ICE | abi.X_NO_HYDRO)
    assert names == ["mean", "GREB_X_NO_ICE", "GREB_X_NO_HYDRO", "GREB_X_NO_ICE:GREB_X_NO_HYDRO"]
    assert np.array_equal(w * 4, [[1, 1, 1, 1], [-1, 1, -1, 1], [-1, -1, 1, 1], [1, -1, -1, 1]])
    with pytest.raises(ValueError):
        lin.factorial(sw, 0xff, order=3)  # 93 terms
    with pytest.raises(ValueError):
        lin.factorial(sw, 0x100)


def test_tool_parses_its_command_line():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_effects.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--compare" in out.stdout and "--order" in out.stdout and "years" in out.stdout
