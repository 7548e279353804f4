"""CPU: the ensemble-output interface (include/greb_engine.h: greb_ens_*, greb_engine_run_ens) -- its symbols, its kernels
in the built library, its argument errors (all reported before any device query) -- and the numpy mirror ens.reference
against independent numpy and on cases whose answer is known exactly.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, engine, ens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("greb_ens_create", "greb_ens_destroy", "greb_ens_reduce_dev", "greb_engine_run_ens")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


def test_new_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    f90 = open(os.path.join(ROOT, "greb_climate_model_amd", "host", "greb_c_api.f90")).read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", code), n
        assert n in engine.EXPORTS and hasattr(lib, n), n
        assert f'name="{n}"' in f90, n
    for name, val in (("GREB_S_MEAN", abi.S_MEAN), ("GREB_S_VAR", abi.S_VAR), ("GREB_S_RANGE", abi.S_RANGE),
                      ("GREB_S_QUANTILES", abi.S_QUANTILES)):
        assert re.search(rf"#define {name}\s+{val}u", code), name
    for name, val in (("GREB_ENS_MAX_GROUPS", abi.ENS_MAX_GROUPS), ("GREB_ENS_MAX_PROBS", abi.ENS_MAX_PROBS),
                      ("GREB_ENS_MAX_SORTED", abi.ENS_MAX_SORTED)):
        assert re.search(rf"#define {name}\s+{val}\b", code), name
    assert (abi.S_MEAN, abi.S_VAR, abi.S_RANGE, abi.S_QUANTILES) == (1, 2, 4, 8)
    assert ens.PRODUCTS == ("mean", "var", "min", "max", "quant")


def test_library_has_the_ensemble_kernels_for_gfx950(lib):
    from greb_climate_model_amd import codesha
    assert "greb_ens.hip" in build.SOURCES and "greb_ens.h" in build.HEADERS
    assert "greb_ensemble.hip" in build.SOURCES  # the stand-alone calls stay
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["greb_ens.hip"]  # the operation order is the definition of the results
    mom = codesha.kernel_functions(build.LIB, "ens_moments_kernel")
    assert len(mom) == 4 and all(len(c) > 64 for c in mom.values()), sorted(mom)  # {no control, control} x {8-byte, scalar}
    qu = codesha.kernel_functions(build.LIB, "ens_quantile_kernel")
    assert len(qu) == 1 and len(next(iter(qu.values()))) > 64


def _err(fn, code=-1):
    with pytest.raises(engine.GrebError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_plan_argument_errors_name_the_offender(lib):
    nx, ny = 96, 48
    P = lambda *a, **k: ens.Plan(nx, ny, *a, **k)
    P(3, [0, 0, 1]).close()
    P(3, [-1, 0, 0], control=[-1, 0, 2], probs=[0.0, 0.5, 1.0]).close()  # a member may be its own control
    P(1, [0]).close()
    for gx, gy in ((95, 48), (8, 48), (96, 4), (96, 193)):  # the grids diag.Plan rejects
        assert f"grid {gx} x {gy}" in _err(lambda: ens.Plan(gx, gy, 1, [0]))
    assert "n_members = 0" in _err(lambda: P(0, []))
    assert "n_groups = 0" in _err(lambda: P(2, [-1, -1]))
    assert "n_groups = 65" in _err(lambda: P(65, list(range(65))))
    P(64, list(range(64))).close()
    msg = _err(lambda: P(3, [0, -2, 0]))
    assert "member 1" in msg and "group = -2" in msg, msg
    one = np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    h = C.c_void_p()
    two = np.array([0, 2], np.int32)
    assert lib.greb_ens_create(nx, ny, 2, two.ctypes.data_as(C.POINTER(C.c_int32)), 2, None, None, 0, 1, C.byref(h)) == -1
    msg = lib.greb_engine_last_error(None).decode()
    assert "member 1" in msg and "group = 2" in msg, msg
    msg = _err(lambda: P(3, [0, 0, 0], control=[0, 3, 0]))
    assert "member 1" in msg and "control = 3" in msg, msg
    msg = _err(lambda: P(3, [0, 0, 0], control=[0, 0, -2]))
    assert "member 2" in msg and "control = -2" in msg, msg
    assert "group 1 is empty" in _err(lambda: P(3, [0, 2, 0]))
    msg = _err(lambda: P(3, [-1, 0, 0], control=[-1, 0, -1]))
    assert "member 2" in msg and "no control" in msg, msg
    assert "`what` = 0" in _err(lambda: P(3, [0, 0, 0], what=0))
    assert "`what` = 16" in _err(lambda: P(3, [0, 0, 0], what=16))
    assert "`what` = 17" in _err(lambda: P(3, [0, 0, 0], what=abi.S_MEAN | 16))
    assert "n_probs = 0" in _err(lambda: P(3, [0, 0, 0], what=abi.S_QUANTILES))
    assert "n_probs = 17" in _err(lambda: P(3, [0, 0, 0], probs=np.linspace(0, 1, 17)))
    P(3, [0, 0, 0], probs=np.linspace(0, 1, 16)).close()
    for bad in (-0.01, 1.01, np.nan, np.inf):
        msg = _err(lambda: P(3, [0, 0, 0], probs=[0.5, bad]))
        assert "probability 1" in msg and "not in [0, 1]" in msg, msg
    P(3, [0, 0, 0], probs=[7.0], what=abi.S_MEAN).close()  # probabilities are read only under GREB_S_QUANTILES
    assert "3 integers" in _err(lambda: P(3, [0, 0]))
    assert "3 integers" in _err(lambda: P(3, [0, 0, 0], control=[0, 0]))
    assert lib.greb_ens_create(nx, ny, 1, one, 1, None, None, 0, 1, None) == -1
    assert lib.greb_ens_create(nx, ny, 1, None, 1, None, None, 0, 1, C.byref(h)) == -1
    assert "`group` is NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_ens_destroy(None) == 0


def test_quantile_group_size_limit_is_a_host_check(lib):
    n = abi.ENS_MAX_SORTED + 1
    group = [0] * n + [1]
    msg = _err(lambda: ens.Plan(96, 48, n + 1, group, probs=[0.5]), code=-4)
    assert "group 0 of 4097 members" in msg, msg
    ens.Plan(96, 48, n + 1, group).close()                         # the same plan without quantiles
    ens.Plan(96, 48, n + 1, group, probs=[0.5], what=ens.MOMENTS).close()
    ens.Plan(96, 48, n, [0] * (n - 1) + [1], probs=[0.5]).close()  # 4096 members are sorted


def _aligned():
    buf = np.zeros(64, np.float32)
    return buf, C.c_void_p((buf.ctypes.data + 15) & ~15)


def test_dev_argument_errors_come_before_any_device_query(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, ok = _aligned()
    bad = C.c_void_p(ok.value + 4)
    plan = ens.Plan(96, 48, 2, [0, 0], probs=[0.5])
    red = lib.greb_ens_reduce_dev
    assert red(None, 0, ok, 8, ok, ok, ok, ok, ok, None) == -1 and "no plan" in last()
    assert red(plan.h, 0, None, 8, ok, ok, ok, ok, ok, None) == -1 and "x_dev is NULL" in last()
    assert red(plan.h, 0, bad, 8, ok, ok, ok, ok, ok, None) == -1 and "x_dev is not 16-byte aligned" in last()
    assert red(plan.h, 0, ok, 0, ok, ok, ok, ok, ok, None) == -1 and "n = 0" in last()
    for i, name in enumerate(ens.PRODUCTS):  # the plan selects all: each needs a pointer
        assert red(plan.h, 0, ok, 8, *[None if j == i else ok for j in range(5)], None) == -1
        assert f"selected but `{name}_dev` is NULL" in last(), last()
    plan.close()


def test_run_ens_argument_errors_are_decided_without_an_engine(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, _ = _aligned()
    p = abi.fptr(buf)
    plan = ens.Plan(96, 48, 2, [0, 0], probs=[0.5])
    run = lib.greb_engine_run_ens
    assert run(None, 1, p, None, p, p, p, p, p, None) == -1 and "no plan" in last()
    assert run(None, 0, p, plan.h, p, p, p, p, p, None) == -1 and "years = 0" in last()
    for i, name in enumerate(ens.PRODUCTS):
        ptr = [None if j == i else p for j in range(5)]
        assert run(None, 1, p, plan.h, *ptr, None) == -1 and f"selected but `{name}` is NULL" in last(), last()
    assert run(None, 1, p, plan.h, p, p, p, p, p, None) == -1 and "bad argument (engine" in last()
    only_mean = ens.Plan(96, 48, 2, [0, 0], what=abi.S_MEAN)  # unselected products may be NULL: the next check is reached
    assert run(None, 1, p, only_mean.h, p, None, None, None, None, None) == -1 and "bad argument (engine" in last()
    plan.close(); only_mean.close()


def test_dev_calls_without_a_gpu_are_a_loud_error(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    buf, ok = _aligned()
    plan = ens.Plan(96, 48, 1, [0])
    assert lib.greb_ens_reduce_dev(plan.h, 0, ok, 8, ok, ok, ok, ok, None, None) == -2
    assert b"no CPU path" in lib.greb_engine_last_error(None)
    plan.close()


# ---- the mirror against independent numpy ----------------------------------------------------------------------------
GROUP = [0, 1, 0, -1, 1, 0, 1]
CONTROL = [3, 3, 0, -1, 1, 6, 2]  # controls inside (2 -> 0, 4 -> 1) and outside (0 -> 3, 1 -> 3, 5 -> 6, 6 -> 2) the member's own group
PROBS = [0.0, 0.05, 0.25, 0.5, 0.77, 0.95, 1.0]


@pytest.fixture(scope="module")
def data():
    from test_gpu_clim import synth
    return synth(1, 7, 5, 12, seed=5)[0]  # [7][12][5][5][12]


@pytest.mark.parametrize("control", [None, CONTROL])
def test_mirror_agrees_with_independent_numpy(data, control):
    """np.mean, np.var(ddof=1) and np.quantile of the fp64 samples; the bound is one fp32 rounding (2^-24 = 6e-8) with an
    order of magnitude to spare.  The group spread of the synthetic records is tens of kelvin: a well-conditioned variance."""
    r = ens.reference(data, GROUP, control, PROBS)
    assert r.mean.shape == r.var.shape == r.min.shape == r.max.shape == (2,) + data.shape[1:]
    assert r.quant.shape == (2, len(PROBS)) + data.shape[1:]
    assert all(getattr(r, n).dtype == np.float32 for n in ens.PRODUCTS)
    for g in range(2):
        members = [m for m in range(7) if GROUP[m] == g]
        v = np.stack([data[m] if control is None else data[m] - data[control[m]] for m in members])
        assert v.dtype == np.float32
        v64 = v.astype(np.float64)
        np.testing.assert_allclose(r.mean[g], v64.mean(axis=0), rtol=1e-6, atol=0)
        np.testing.assert_allclose(r.var[g], v64.var(axis=0, ddof=1), rtol=1e-6, atol=0)
        np.testing.assert_allclose(r.quant[g], np.quantile(v64, np.asarray(PROBS, np.float32).astype(np.float64), axis=0), rtol=1e-6,
                                   atol=0)
        assert np.array_equal(r.min[g], v.min(axis=0)) and np.array_equal(r.max[g], v.max(axis=0))
        np.testing.assert_allclose(r.std[g], v64.std(axis=0, ddof=1), rtol=1e-6, atol=0)


def test_mirror_products_follow_the_flags(data):
    full = ens.reference(data, GROUP, CONTROL, PROBS)
    for what, names in ((abi.S_MEAN, ("mean",)), (abi.S_VAR, ("var",)), (abi.S_RANGE, ("min", "max")), (abi.S_QUANTILES, ("quant",))):
        one = ens.reference(data, GROUP, CONTROL, PROBS, what=what)
        for n in ens.PRODUCTS:
            if n in names:
                assert np.array_equal(getattr(one, n), getattr(full, n)), (what, n)
            else:
                assert getattr(one, n) is None, (what, n)
    assert ens.reference(data, GROUP).quant is None and ens.reference(data, GROUP, what=abi.S_MEAN).std is None


# ---- the mirror on cases with a known answer -------------------------------------------------------------------------
def test_mirror_constant_field_comes_back_exactly():
    for c in (np.float32(287.65), np.float32(0.0123), np.float32(0.31)):
        x = np.full((6, 12, 5, 5, 12), c, np.float32)
        r = ens.reference(x, [0, 0, 0, 1, 1, 1], probs=[0.0, 0.3, 0.5, 1.0])
        for a in (r.mean, r.min, r.max):
            assert np.array_equal(a, np.full(a.shape, c))
        assert np.array_equal(r.quant, np.full(r.quant.shape, c))
        assert not r.var.any() and not r.std.any()


def test_mirror_group_of_one(data):
    r = ens.reference(data, [-1, 0, -1, -1, 1, 1, -1], probs=PROBS)
    assert not r.var[0].any()
    for a in (r.mean[0], r.min[0], r.max[0], *r.quant[0]):
        assert np.array_equal(a, data[1])


def test_mirror_own_control_gives_a_zero_response(data):
    r = ens.reference(data, [0, 0, 1, 1, 1, -1, -1], [0, 1, 0, 1, 2, -1, -1], probs=PROBS)
    for n in ens.PRODUCTS:
        a = getattr(r, n)[0]
        assert not a.any() and not np.signbit(a).any(), n
    assert r.var[1].all()


def test_mirror_probabilities_0_and_1_are_min_and_max(data):
    for control in (None, CONTROL):
        r = ens.reference(data, GROUP, control, probs=[0.0, 1.0])
        assert np.array_equal(r.quant[:, 0], r.min) and np.array_equal(r.quant[:, 1], r.max)


def test_tool_parses_its_command_line():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_ens.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--compare" in out.stdout and "pairs" in out.stdout and "years" in out.stdout
