"""GPU: the linear-model output (csrc/greb_lin.hip) against lin.reference, the numpy statement of its products.

Every comparison with the mirror is for EQUAL BITS: device and mirror perform the same IEEE operations (one fp32
subtraction for the sample; fp64 multiply, then fp64 add; one conversion to fp32) in the same order on the same fp32 data
-- the kernels are built without contraction of a multiply into the add behind it -- so there is nothing for a tolerance
to cover.  The inputs are synthetic positive records as test_gpu_ens.synth makes them."""
import ctypes as C

import numpy as np
import pytest

from greb_climate_model_amd import abi, engine, ensemble, lin
from test_gpu_ens import bits, synth

pytestmark = pytest.mark.gpu

NAMES = lin.PRODUCTS
REC = (12, 5, 8, 12)  # 5 760 elements: twelve workgroups of lin_coef_kernel, twenty-three of lin_rss_kernel


def model(M, K, seed):
    """A least-squares model of K terms on M members: the intercept and K - 1 random predictors (K > M: the minimum-norm
    solution; all that matters here is a dense fp64 weight table and its design)."""
    pred = np.random.default_rng(seed).standard_normal((M, K - 1))
    _, w, d = lin.regression(pred, [f"p{j}" for j in range(K - 1)])
    assert w.shape == (K, M) and d.shape == (M, K) and np.isfinite(w).all()
    return w, d


def same_bits(got, ref, label):
    """Both products of two Results: both None, or equal shape and equal bits."""
    for name in NAMES:
        g, r = getattr(got, name), getattr(ref, name)
        assert (g is None) == (r is None), (label, name)
        if g is None:
            continue
        g, r = np.asarray(g), np.asarray(r)
        assert g.dtype == np.float32 and g.shape == r.shape, (label, name, g.dtype, g.shape, r.shape)
        bad = bits(g) != bits(r)
        print(f"{label} {name}: {int(bad.sum())} of {bad.size} values differ from the mirror")
        assert not bad.any(), (label, name, int(bad.sum()), g[bad][:4], r[bad][:4])


def to_host(res):
    import torch
    torch.cuda.synchronize()
    return lin.Result(*[None if getattr(res, n) is None else getattr(res, n).cpu().numpy() for n in NAMES])


def reduce(x, w, use=None, control=None, design=None, what=None):
    import torch
    plan = lin.Plan(96, 48, x.shape[0], w, use=use, control=control, design=design, what=what)  # (reduce_dev takes any record)
    got = to_host(lin.reduce_dev(plan, torch.from_numpy(x).cuda()))
    plan.close()
    return got


USE7 = [1, 1, 0, 1, 1, 0, 1]
CONTROL7 = [3, 3, -1, 3, 1, 0, 6]  # member 3 its own control, member 6 likewise; member 5 unused with a control, 2 without


@pytest.mark.parametrize("use", [None, USE7], ids=["all", "use"])
@pytest.mark.parametrize("control", [None, CONTROL7], ids=["raw", "response"])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_raw_lengths_against_the_mirror(n, control, use):
    """Odd n: rows that are not 8-byte aligned, and a last element whose lane owns it alone; n = 1 and 7: one workgroup."""
    if control is not None and use is None:
        control = [c if c >= 0 else 0 for c in control]  # every member is used: each needs a control
    x = synth(7, (n,), seed=n)
    w, d = model(7, 3, seed=n)
    same_bits(reduce(x, w, use, control, d), lin.reference(x, w, use, control, d), f"n={n}")


@pytest.mark.parametrize("control", [None, [(5 * m + 1) % 37 for m in range(37)]], ids=["raw", "response"])
@pytest.mark.parametrize("K", [1, 16, 17, 64])
def test_term_counts_against_the_mirror(K, control):
    """The edges of the chunks of 16 terms (one chunk, one full, one full and one term, four full) with 37 members: more
    than the rows a lane keeps in flight, and no multiple of them."""
    x = synth(37, REC, seed=K)
    w, d = model(37, K, seed=K)
    got = reduce(x, w, None, control, d)
    assert got.coef.shape == (K,) + REC and got.rss.shape == REC
    same_bits(got, lin.reference(x, w, None, control, d), f"K={K}")


def test_even_length_with_a_partial_last_workgroup():
    """n = 1 026: the 8-byte path, three workgroups of lin_coef_kernel, the last with one pair of elements."""
    x = synth(9, (1026,), seed=11)
    w, d = model(9, 4, seed=11)
    same_bits(reduce(x, w, None, None, d), lin.reference(x, w, None, None, d), "n=1026")


def test_member_list_against_the_mirror():
    """130 members, every third dropped, the last member the control of all (and of itself)."""
    M = 130
    use = [int(m % 3 != 2) for m in range(M)]
    control = [M - 1] * M
    assert use[M - 1] == 1
    x = synth(M, REC, seed=130)
    w, d = model(M, 5, seed=130)
    got = reduce(x, w, use, control, d)
    same_bits(got, lin.reference(x, w, use, control, d), "130 members")
    assert got.coef.any() and got.rss.any()


def test_each_single_flag_gives_the_numbers_of_both():
    """... and the buffer of the product it does not select, handed over filled with NaN, stays untouched."""
    import torch
    x = synth(13, (4097,), seed=9)
    xd = torch.from_numpy(x).cuda()
    w, d = model(13, 17, seed=9)
    control = [(m + 4) % 13 for m in range(13)]
    full = reduce(x, w, None, control, d)
    assert full.coef is not None and full.rss is not None
    for what, name in ((abi.L_COEF, "coef"), (abi.L_RSS, "rss")):
        plan = lin.Plan(96, 48, 13, w, control=control, design=d, what=what)
        one = to_host(lin.reduce_dev(plan, xd))
        buf = {"coef": torch.full((17, 4097), float("nan"), dtype=torch.float32, device="cuda"),
               "rss": torch.full((4097,), float("nan"), dtype=torch.float32, device="cuda")}
        engine._check(engine.lib().greb_lin_reduce_dev(plan.h, 0, C.c_void_p(xd.data_ptr()), 4097, C.c_void_p(buf["coef"].data_ptr()),
                                                       C.c_void_p(buf["rss"].data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        plan.close()
        for n in NAMES:
            if n == name:
                assert np.array_equal(bits(getattr(one, n)), bits(getattr(full, n))), (what, n)
                assert np.array_equal(bits(buf[n].cpu().numpy()), bits(getattr(full, n))), (what, n)
            else:
                assert getattr(one, n) is None, (what, n)
                assert bool(torch.isnan(buf[n]).all()), (what, n, "an unselected product's buffer was written")


def test_unused_rows_are_never_read_and_calls_repeat():
    """An unused member that is nobody's control may hold NaN: every output is finite and has the bits it had; a second
    call gives the same bits."""
    import torch
    M = 11
    use = [1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 1]
    control = [4, 4, -1, 0, -1, 5, 4, -1, 8, 0, 1]  # member 4 is unused but a control; 2 and 7 are neither
    x = synth(M, REC, seed=21)
    w, d = model(M, 6, seed=21)
    plan = lin.Plan(96, 48, M, w, use=use, control=control, design=d)
    a = to_host(lin.reduce_dev(plan, torch.from_numpy(x).cuda()))
    same_bits(a, lin.reference(x, w, use, control, d), "clean")
    y = x.copy()
    y[2] = np.nan
    y[7] = np.nan
    yd = torch.from_numpy(y).cuda()
    b, c = to_host(lin.reduce_dev(plan, yd)), to_host(lin.reduce_dev(plan, yd))
    plan.close()
    assert np.isfinite(b.coef).all() and np.isfinite(b.rss).all()
    same_bits(b, a, "NaN in unused rows")
    same_bits(c, b, "second call")


def test_independent_of_the_batch():
    """A plan's numbers do not change when unrelated members are appended to x (and left unused), nor when they sit between
    its members."""
    M = 9
    x = synth(M, REC, seed=31)
    w, d = model(M, 5, seed=31)
    control = [(m + 2) % M for m in range(M)]
    alone = reduce(x, w, None, control, d)
    more = synth(4, REC, seed=32)
    x_app = np.concatenate([x, more])
    pad = lambda a, axis: np.concatenate([a, np.full(a.shape[:axis] + (4,) + a.shape[axis + 1:], np.nan)], axis=axis)
    got = reduce(x_app, pad(w, 1), [1] * M + [0] * 4, control + [-1] * 4, pad(d, 0))
    same_bits(got, alone, "appended")
    at = [0, 1, 10, 2, 3, 11, 4, 5, 6, 12, 7, 8, 9]  # the plan's members in their order, strangers between them
    where = {m: i for i, m in enumerate(at)}
    x_mix = np.ascontiguousarray(x_app[at])
    w_mix, d_mix = np.ascontiguousarray(pad(w, 1)[:, at]), np.ascontiguousarray(pad(d, 0)[at])
    use_mix = [int(m < M) for m in at]
    control_mix = [where[control[m]] if m < M else -1 for m in at]
    same_bits(reduce(x_mix, w_mix, use_mix, control_mix, d_mix), alone, "interleaved")


# ---- run_lin on a real engine ----------------------------------------------------------------------------------------
def _same_engine_state(a, b, yr_a, yr_b):
    assert np.array_equal(yr_a, yr_b), "yearly differs"
    for m in range(a.nm):
        assert np.array_equal(a.state(m), b.state(m)), f"state of member {m} differs"


def _year(res, y):
    return lin.Result(res.coef[:, y], res.rss[y])


def _factorial_engines(inputs, params, switch_bits, n=2):
    sw = ensemble.switch_factorial(switch_bits)
    es = [engine.Engine(inputs, params, members=[{"switches": int(s)} for s in sw]) for _ in range(n)]
    for e in es:
        e.flux_correction(1)
    return sw, es


def test_run_lin_against_run(inputs, params):
    """Twin engines on the factorial of two switches, CO2 rising from year to year (a year delivered from the wrong output
    slot, or before its kernels, is not the mirror's).  Two years in one call, then one and one on a third engine."""
    which = abi.X_NO_ICE | abi.X_NO_DEEP_OCEAN
    sw, (ea, eb, ec) = _factorial_engines(inputs, params, which, n=3)
    names, w, d = lin.factorial(sw, which, order=1)  # the mean and two main effects: the interaction is the residual
    plan = lin.Plan(inputs.nx, inputs.ny, 4, w, design=d)
    co2 = np.repeat(np.asarray([[680.0, 760.0]], np.float32), 4, axis=0)
    family = eb.describe()["kernel_family"]
    mon, yr_a = ea.run(2, co2)
    res = eb.run_lin(2, co2, plan)
    assert res.coef.shape == (3, 2, 12, 5, 48, 96) and res.rss.shape == (2, 12, 5, 48, 96)
    for y in range(2):
        same_bits(_year(res, y), lin.reference(mon[:, y], w, design=d), f"run_lin year {y}")
    assert not np.array_equal(mon[:, 0], mon[:, 1]), "the years differ"
    assert res.coef[1].any() and res.rss.any(), "the ice switch has an effect, and an interaction with the deep ocean"
    assert eb.describe()["kernel_family"] == family == ea.describe()["kernel_family"]
    _same_engine_state(ea, eb, yr_a, res.yearly)
    r0, r1 = ec.run_lin(1, co2[:, :1], plan), ec.run_lin(1, co2[:, 1:], plan)  # the clock continues as after run()
    same_bits(_year(r0, 0), _year(res, 0), "1 + 1 years, first")
    same_bits(_year(r1, 0), _year(res, 1), "1 + 1 years, second")
    _same_engine_state(eb, ec, res.yearly[:, 1:], r1.yearly)
    only = lin.Plan(inputs.nx, inputs.ny, 4, w)  # another plan, one product
    mon3, yr3_a = ea.run(1, 500.0)
    res3 = eb.run_lin(1, 500.0, only)
    assert res3.rss is None
    assert np.array_equal(bits(res3.coef[:, 0]), bits(lin.reference(mon3[:, 0], w).coef))
    _same_engine_state(ea, eb, yr3_a, res3.yearly)
    for x in (ea, eb, ec, plan, only):
        x.close()


def test_run_lin_saturated_factorial_leaves_no_residual(inputs, params):
    """Eight members, three switches, all eight terms: the fit is every member itself.  Weights +-1/8 and the sums of eight
    fp32 values of one grid point are exact in fp64, so the residual is zero to the bit."""
    which = abi.X_NO_ICE | abi.X_NO_DEEP_OCEAN | abi.X_NO_HYDRO
    sw, (ea, eb) = _factorial_engines(inputs, params, which)
    names, w, d = lin.factorial(sw, which, order=3)
    assert len(sw) == 8 and len(names) == 8
    plan = lin.Plan(inputs.nx, inputs.ny, 8, w, design=d)
    mon, yr_a = ea.run(1, 680.0)
    res = eb.run_lin(1, 680.0, plan)
    same_bits(_year(res, 0), lin.reference(mon[:, 0], w, design=d), "saturated")
    print(f"saturated factorial: largest rss {float(res.rss.max()):.3g}")
    assert not res.rss.any()
    assert all(res.coef[k].any() for k in range(4)), "the mean and the three main effects are not zero"
    _same_engine_state(ea, eb, yr_a, res.yearly)
    for x in (ea, eb, plan):
        x.close()


def test_run_lin_against_run_g384(inputs384):
    p = abi.default_params(ipx=380, ipy=152)
    w, d = [[0.5, 0.5], [-0.5, 0.5]], [[1.0, -1.0], [1.0, 1.0]]
    plan = lin.Plan(384, 192, 2, w, control=[1, 1], design=d)
    ea, eb = (engine.Engine(inputs384, p, n_members=2) for _ in range(2))
    for e in (ea, eb):
        e.flux_correction(1)
    co2 = np.array([[340.0], [680.0]], np.float32)
    mon, yr_a = ea.run(1, co2)
    res = eb.run_lin(1, co2, plan)
    print(f"384x192 circulation: {eb.describe().get('circulation')}")
    same_bits(_year(res, 0), lin.reference(mon[:, 0], w, control=[1, 1], design=d), "run_lin 384x192")
    assert res.coef[0, 0, :, 0].any(), "half of member 0 at 340 ppm minus member 1 at 680 ppm is not zero"
    _same_engine_state(ea, eb, yr_a, res.yearly)
    ea.close(); eb.close(); plan.close()


def test_refused_calls_leave_the_engine_alone(inputs, params):
    co2 = np.asarray([[400.0] * 2, [800.0] * 2], np.float32)
    ea, eb = (engine.Engine(inputs, params, n_members=2) for _ in range(2))
    w, d = [[0.5, 0.5]], [[1.0], [1.0]]
    other_grid, other_members = lin.Plan(100, 37, 2, w), lin.Plan(96, 48, 3, [[0.5, 0.25, 0.25]])
    plan = lin.Plan(96, 48, 2, w, design=d)
    for bad, words in ((other_grid, ("100 x 37", "96 x 48")), (other_members, ("3 members", "has 2"))):
        with pytest.raises(engine.GrebError) as ei:
            ea.run_lin(2, co2, bad)
        assert ei.value.code == -1 and all(x in str(ei.value) for x in words), ei.value
    rss, yearly = np.empty((2, 12, 5, 48, 96), np.float32), np.zeros((2, 2, 2), np.float32)
    assert engine.lib().greb_engine_run_lin(ea.h, 2, abi.fptr(co2), plan.h, None, abi.fptr(rss), abi.fptr(yearly)) == -1
    assert "GREB_L_COEF selected but `coef` is NULL" in engine.lib().greb_engine_last_error(ea.h).decode()
    ra, rb = ea.run_lin(2, co2, plan), eb.run_lin(2, co2, plan)  # ... bit-identical to an untouched twin
    same_bits(ra, rb, "after the refusals")
    _same_engine_state(ea, eb, ra.yearly, rb.yearly)
    for x in (ea, eb, other_grid, other_members, plan):
        x.close()
