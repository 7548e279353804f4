"""CPU: the covariance interface (include/greb_engine.h: greb_gram_*, greb_engine_run_gram) -- its symbols, its kernels in
the built library, its argument errors (all reported before any device query) -- and the numpy mirror gram.reference and
the helpers of gram.py on cases whose answer is known.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, engine, gram, lin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("greb_gram_create", "greb_gram_destroy", "greb_gram_reduce_dev", "greb_engine_run_gram", "greb_engine_run_budget_gram")


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
    assert re.search(rf"#define GREB_GRAM_MAX_BLOCKS\s+{abi.GRAM_MAX_BLOCKS}\b", code)
    assert re.search(rf"#define GREB_GRAM_MAX_USED\s+{abi.GRAM_MAX_USED}\b", code)
    assert (abi.GRAM_MAX_BLOCKS, abi.GRAM_MAX_USED) == (16, 1024)
    # the header is the contract: it says that fused and unfused give the same bits, and what is forbidden
    text = " ".join(hdr.split())
    assert "exact in fp64" in text and "reassociating the adds" in text


def test_library_has_the_gram_kernels_for_gfx950(lib):
    from greb_climate_model_amd import codesha
    assert "greb_gram.hip" in build.SOURCES and "greb_gram.h" in build.HEADERS
    assert build.EXTRA_FLAGS["greb_gram.hip"] == build.EXTRA_FLAGS["greb_lin.hip"]
    assert not any("fast-math" in f or f == "-Ofast" for f in build.HIPCC_FLAGS + build.EXTRA_FLAGS["greb_gram.hip"])
    tiles = codesha.kernel_functions(build.LIB, "gram_tile_kernel")
    assert len(tiles) == 6 and all(len(c) > 64 for c in tiles.values()), sorted(tiles)  # {control} x {16-byte, scalar, 16-byte scaled}
    sums = codesha.kernel_functions(build.LIB, "gram_sum_kernel")
    assert len(sums) == 1 and all(len(c) > 64 for c in sums.values()), sorted(sums)


# ---- argument errors -------------------------------------------------------------------------------------------------
def _err(fn, code=-1):
    with pytest.raises(engine.GrebError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_plan_argument_errors_name_the_offender(lib):
    nx, ny = 96, 48
    P = lambda *a, **k: gram.Plan(nx, ny, *a, **k)
    P(3, 4, [0, 1, -1, 0]).close()
    P(3, 4, [0, 0, 0, 0], use=[1, 0, 1], control=[0, -1, 2]).close()  # a member may be its own control; an unused one needs none
    P(1, 1, [0], scale=np.ones((ny, nx))).close()
    for gx, gy in ((95, 48), (8, 48), (96, 4), (96, 193)):  # the grids diag.Plan rejects
        assert f"grid {gx} x {gy}" in _err(lambda: gram.Plan(gx, gy, 1, 1, [0]))
    assert "n_members = 0" in _err(lambda: P(0, 1, [0]))
    assert "n_records = 0" in _err(lambda: P(3, 0, [], n_blocks=1))
    assert "n_blocks = 0" in _err(lambda: P(3, 2, [-1, -1]))
    assert "n_blocks = 17" in _err(lambda: P(3, 17, list(range(17))))
    P(3, 16, list(range(16))).close()
    msg = _err(lambda: P(3, 3, [0, 2, 1], n_blocks=2))
    assert "record 1" in msg and "block = 2" in msg, msg
    msg = _err(lambda: P(3, 3, [0, -2, 0]))
    assert "record 1" in msg and "block = -2" in msg, msg
    assert "block 1 is empty" in _err(lambda: P(3, 3, [0, 2, 0]))
    assert "no used member" in _err(lambda: P(3, 1, [0], use=[0, 0, 0]))
    msg = _err(lambda: P(3, 1, [0], control=[0, 3, 0]))
    assert "member 1" in msg and "control = 3" in msg, msg
    msg = _err(lambda: P(3, 1, [0], use=[0, 1, 0], control=[0, 0, 7]))  # ... of an unused member too
    assert "member 2" in msg and "control = 7" in msg, msg
    msg = _err(lambda: P(3, 1, [0], use=[1, 1, 0], control=[0, -1, -1]))
    assert "member 1" in msg and "no control" in msg, msg
    msg = _err(lambda: P(1025, 1, [0]), code=-4)  # GREB_E_UNSUPPORTED
    assert "1025 used members" in msg and "1024" in msg, msg
    P(1025, 1, [0], use=[1] * 1024 + [0]).close()
    for bad in (np.nan, np.inf, -1.0):
        s = np.ones((ny, nx), np.float32); s[5, 7] = bad
        msg = _err(lambda: P(3, 1, [0], scale=s))
        assert "scale" in msg and "row 5" in msg and "column 7" in msg, msg
    assert "4 integers" in _err(lambda: P(3, 4, [0, 0, 0]))
    assert "3 integers" in _err(lambda: P(3, 1, [0], use=[1, 1]))
    assert "3 integers" in _err(lambda: P(3, 1, [0], control=[0, 0]))
    assert "[48][96]" in _err(lambda: P(3, 1, [0], scale=np.ones((96, 48))))
    h = C.c_void_p()
    zero = np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.greb_gram_create(nx, ny, 1, 1, zero, 1, None, None, None, None) == -1
    assert lib.greb_gram_create(nx, ny, 1, 1, None, 1, None, None, None, C.byref(h)) == -1
    assert "`block` is NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_gram_destroy(None) == 0


def _aligned():
    buf = np.zeros(64, np.float32)
    return buf, C.c_void_p((buf.ctypes.data + 15) & ~15)


def test_dev_argument_errors_come_before_any_device_query(lib):
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, ok = _aligned()
    bad = C.c_void_p(ok.value + 4)
    plan = gram.Plan(96, 48, 2, 1, [0])
    red = lib.greb_gram_reduce_dev
    assert red(None, 0, ok, 8, ok, None) == -1 and "no plan" in last()
    assert red(plan.h, 0, None, 8, ok, None) == -1 and "x_dev is NULL" in last()
    assert red(plan.h, 0, bad, 8, ok, None) == -1 and "x_dev is not 16-byte aligned" in last()
    assert red(plan.h, 0, ok, 8, None, None) == -1 and "G_dev is NULL" in last()
    assert red(plan.h, 0, ok, 8, bad, None) == -1 and "G_dev is not 8-byte aligned" in last()
    assert red(plan.h, 0, ok, 0, ok, None) == -1 and "len = 0" in last()
    scaled = gram.Plan(96, 48, 2, 1, [0], scale=np.ones((48, 96)))
    assert red(scaled.h, 0, ok, 8, ok, None) == -1 and "len = 8" in last() and "4608" in last(), last()
    plan.close(); scaled.close()


def test_run_gram_argument_errors_are_decided_without_an_engine(lib):
    """The plan, the years, the record count and the output are looked at before the engine is: no device is needed."""
    last = lambda: lib.greb_engine_last_error(None).decode()
    buf, _ = _aligned()
    p = abi.fptr(buf)
    G = np.zeros(64, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    plan = gram.Plan(96, 48, 2, 60, gram.blocks_by_var(5))
    seasons = gram.Plan(96, 48, 2, 25, [0] * 25)
    run, brun = lib.greb_engine_run_gram, lib.greb_engine_run_budget_gram
    assert run(None, 1, p, None, G, None) == -1 and "run_gram: no plan" in last()
    assert run(None, 0, p, plan.h, G, None) == -1 and "years = 0" in last()
    assert run(None, 1, p, seasons.h, G, None) == -1 and "n_records = 25" in last() and "12 * 5 = 60" in last(), last()
    assert run(None, 1, p, plan.h, None, None) == -1 and "run_gram: `G` is NULL" in last(), last()
    assert run(None, 1, p, plan.h, G, None) == -1 and "bad argument (engine" in last()
    # the budget route: the thirteen terms want 12 * 13 records, a combination of two 12 * 2
    assert brun(None, 1, p, None, 0, plan.h, G, None) == -1 and "run_budget_gram" in last() and "12 * 13 = 156" in last(), last()
    combo = np.zeros((2, abi.NBUDGET), np.float32)
    combo[0, 0] = combo[1, 1] = 1
    assert brun(None, 1, p, abi.fptr(combo), 2, plan.h, G, None) == -1 and "12 * 2 = 24" in last(), last()
    two = gram.Plan(96, 48, 2, 24, gram.blocks_by_var(2))
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, None, None) == -1 and "`G` is NULL" in last(), last()
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, G, None) == -1 and "bad argument (engine" in last()
    combo[1] = 0
    assert brun(None, 1, p, abi.fptr(combo), 2, two.h, G, None) == -1 and "combo row 1 is zero" in last(), last()
    for x in (plan, seasons, two):
        x.close()


def test_dev_call_without_a_gpu_is_a_loud_error(lib):
    import torch
    buf, ok = _aligned()
    plan = gram.Plan(96, 48, 1, 1, [0])
    if not torch.cuda.is_available():
        assert lib.greb_gram_reduce_dev(plan.h, 0, ok, 8, ok, None) == -2
        assert b"no CPU path" in lib.greb_engine_last_error(None)
    plan.close()


# ---- the mirror on cases with a known answer -------------------------------------------------------------------------
def test_mirror_on_small_integers_is_the_integer_gram_matrix():
    """Integers up to 7 in magnitude, 300 elements, 5 records: every partial sum is an integer far below 2^53."""
    rng = np.random.default_rng(1)
    x = rng.integers(-7, 8, (6, 5, 300)).astype(np.float32)
    block = [1, 0, -1, 1, 0]
    xi = x.astype(np.int64)
    G = gram.reference(x, block)
    assert G.dtype == np.float64 and G.shape == (2, 6, 6)
    for b in range(2):
        want = sum(xi[:, r] @ xi[:, r].T for r in range(5) if block[r] == b)
        assert np.array_equal(G[b], want.astype(np.float64)), b
    # a used subset under a control map: differences of integers; member 3 its own control
    use, control = [1, 0, 1, 1, 0, 1], [1, -1, 4, 3, -1, 0]
    G = gram.reference(x, block, use=use, control=control)
    d = np.stack([xi[m] - xi[control[m]] for m in (0, 2, 3, 5)])
    for b in range(2):
        want = sum(d[:, r] @ d[:, r].T for r in range(5) if block[r] == b)
        assert np.array_equal(G[b], want.astype(np.float64)), b
    assert not G[:, 2].any() and not G[:, :, 2].any()  # exact zeros ...
    assert not np.signbit(G[:, 2]).any() and not np.signbit(G[:, :, 2]).any()  # ... and all of them +0.0
    # a scale of powers of two is exact as well; `members` picks rows and columns
    s = np.float32(2.0) ** rng.integers(-2, 3, 300)
    Gs = gram.reference(x, block, scale=s)
    xs = x.astype(np.float64) * s.astype(np.float64)
    assert np.array_equal(Gs[0], xs[:, 1] @ xs[:, 1].T + xs[:, 4] @ xs[:, 4].T)
    assert np.array_equal(gram.reference(x, block, scale=s, members=[1, 4]), Gs[:, [1, 4]][:, :, [1, 4]])


def test_mirror_on_random_data_stays_within_the_derived_bound():
    """Every element of G is a sum of len * n_records exact products, added one by one in fp64: its error against the
    exact sum is at most (len * n_records) * 2^-53 * sum |v_a v_c| (the standard bound (n - 1) u sum |.| of recursive
    summation, u = 2^-53).  The exact sum is taken in np.longdouble, whose own error is 2^-11 of that at least."""
    rng = np.random.default_rng(2)
    n_rec, length = 4, 999
    x = (rng.standard_normal((7, n_rec, length)) * 30 + 250).astype(np.float32)
    control = [(m + 3) % 7 for m in range(7)]
    s = rng.random(length, dtype=np.float32)
    G = gram.reference(x, [0] * n_rec, control=control, scale=s)[0]
    v = np.stack([s * (x[m] - x[control[m]]) for m in range(7)])
    assert v.dtype == np.float32
    vl = v.astype(np.longdouble).reshape(7, -1)
    exact = vl @ vl.T
    bound = length * n_rec * 2.0 ** -53 * (np.abs(vl) @ np.abs(vl).T)
    err = np.abs(G.astype(np.longdouble) - exact)
    print(f"largest error / bound: {float((err / bound).max()):.3g}")
    assert (err <= bound).all()
    assert np.array_equal(G, G.T)


def test_center_and_distance_are_exact_on_integers():
    rng = np.random.default_rng(3)
    v = rng.integers(-9, 10, (8, 40)).astype(np.int64)  # eight members: the means are multiples of 1/64
    G = (v @ v.T).astype(np.float64)
    dev = 8 * v - v.sum(axis=0, keepdims=True)  # 8 (v - mean), in integers
    assert np.array_equal(gram.center(G) * 64.0, (dev @ dev.T).astype(np.float64))
    D = ((v[:, None, :] - v[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(gram.distance(G), D.astype(np.float64))
    both = np.stack([G, 4 * G])  # over the last two axes
    assert np.array_equal(gram.center(both)[1], 4 * gram.center(G)) and np.array_equal(gram.distance(both)[1], 4 * D)
    assert np.array_equal(gram.blocks_by_var(3).reshape(12, 3), np.tile(np.arange(3), (12, 1)))
    assert np.array_equal(gram.blocks_by_var(2, months=[0, 11]).reshape(12, 2)[[0, 1, 11]], [[0, 1], [-1, -1], [0, 1]])
    s = gram.area_scale(48, 96)
    assert s.dtype == np.float32 and s.shape == (48, 96)
    lat = (np.arange(48) + 0.5) * 180.0 / 48 - 90.0
    assert np.array_equal(s[:, 0], np.sqrt(np.cos(np.deg2rad(lat))).astype(np.float32)) and np.array_equal(s[:, 0], s[:, 95])
    mask = np.zeros((48, 96)); mask[10:20] = 1
    assert np.array_equal(gram.area_scale(48, 96, mask) != 0, mask != 0)


def test_eof_reproduces_the_matrix_and_gives_orthonormal_patterns():
    """Ten members' responses to their controls, three strong modes and noise, on a 12 x 8 map with an area scale and two
    records.  (1) sum_j lam_j V_j V_j^T = C within U^2 eps ||C||_F, V_j = sqrt(lam_j) weight_j restricted to the used
    members.  (2) The weight rows fed to lin.reference return patterns that are orthonormal under the squared scale.
    The patterns come back as fp32 (2^-24 each), so two patterns' product is off by 2^-23 at most; the weights carry the
    eigen-solver's error U eps ||C|| / gap divided by lam_j: with the three leading modes well separated here (printed)
    that is far below; 1e-5 covers both with room."""
    rng = np.random.default_rng(4)
    U, ny, nx = 10, 8, 12
    modes = rng.standard_normal((3, 2, ny, nx))
    amp = rng.standard_normal((U, 3)) * np.asarray([8.0, 4.0, 2.0])
    resp = np.einsum("uk,krji->urji", amp, modes) + 0.05 * rng.standard_normal((U, 2, ny, nx))
    ctl = 250 + 20 * rng.standard_normal((U, 2, ny, nx))
    x = np.concatenate([ctl + resp, ctl]).astype(np.float32)  # member m, then its control U + m
    use, control = [1] * U + [0] * U, list(range(U, 2 * U)) * 2
    s = gram.area_scale(ny, nx)
    G = gram.reference(x, [0, 0], use=use, control=control, scale=s)[0]
    C_ = gram.center(G)

    class FakePlan:
        used, nm = np.arange(U), 2 * U
    lam, frac, w = gram.eof(G, U, FakePlan)
    assert w.shape == (U, 2 * U) and not w[:, U:].any()
    assert (np.diff(lam) <= 0).all() and abs(frac[lam > 0].sum() - 1) < 1e-12
    V = w[:, :U] * np.sqrt(np.maximum(lam, 0))[:, None]
    rebuilt = (V * lam[:, None]).T @ V
    err = np.linalg.norm(rebuilt - C_)
    print(f"eof: |V diag(lam) V^T - C|_F = {err:.3g}, bound {U * U * np.finfo(np.float64).eps * np.linalg.norm(C_):.3g}; "
          f"leading eigenvalues {lam[:4]}")
    assert err <= U * U * np.finfo(np.float64).eps * np.linalg.norm(C_)
    lam3, frac3, w3 = gram.eof(G, 3, FakePlan)
    assert np.array_equal(lam3, lam[:3]) and frac3.sum() > 0.99
    pat = lin.reference(x, w3, control=control).coef.astype(np.float64)  # [3][2][ny][nx]
    s2 = s.astype(np.float64) ** 2
    inner = np.einsum("jrab,krab,ab->jk", pat, pat, s2)
    print("eof: inner products of the patterns under the scale\n", inner)
    assert np.abs(inner - np.eye(3)).max() < 1e-5
    with pytest.raises(ValueError):
        gram.eof(G, U + 1)
