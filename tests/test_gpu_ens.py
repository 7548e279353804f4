"""GPU: the ensemble output (csrc/greb_ens.hip) against ens.reference, the numpy statement of its products.

Every comparison with the mirror is for EQUAL BITS: device and mirror perform the same IEEE operations (one fp32
subtraction for the sample; fp64 add, multiply, divide; one conversion to fp32) in the same order on the same fp32 data --
the kernels are built without contraction of a multiply into the add behind it -- so there is nothing for a tolerance
to cover.  The inputs are synthetic positive records, or differences of them, which never produce -0."""
import ctypes as C

import numpy as np
import pytest

from greb_climate_model_amd import abi, engine, ens, ensemble

pytestmark = pytest.mark.gpu

NAMES = ens.PRODUCTS
LO = np.array([220.0, 220.0, 271.0, 1e-3, 0.05], np.float32)  # Tsurf, Tair, Tocean [K], q [kg/kg], albedo
HI = np.array([310.0, 300.0, 303.0, 2e-2, 0.80], np.float32)
PROBS16 = [0.0, 0.5, 1.0, 0.05, 0.95, 0.25, 0.75, 0.1, 0.9, 0.33, 0.66, 0.01, 0.99, 0.2, 0.8, 0.5]
# 7 members: two groups of three interleaved, member 3 in none; controls inside (2 -> 0, 4 -> 1) and outside the own group
GROUP7 = [0, 1, 0, -1, 1, 0, 1]
CONTROL7 = [3, 3, 0, -1, 1, 6, 2]
# 13 members: groups of 1, 2, 3 and 5 interleaved, members 4 and 9 in none; controls inside and outside, two their own
GROUP13 = [3, 1, 3, 0, -1, 2, 3, 1, 2, -1, 3, 2, 3]
CONTROL13 = [4, 9, 0, 3, -1, 5, 9, 1, 0, -1, 12, 4, 2]
# 130 members: a group of 64 and one of 65 interleaved, the last member the control of all
GROUP130 = [m % 2 for m in range(128)] + [1, -1]
CONTROL130 = [129] * 129 + [-1]


def synth(n, rec, seed):
    """Strictly positive fp32 records of physical magnitude, [n] + rec ([..][5][ny][nx] records get the five variables'
    ranges)."""
    rng = np.random.default_rng(seed)
    x = rng.random((n,) + tuple(rec), dtype=np.float32)
    if len(rec) == 4:
        x *= (HI - LO)[:, None, None]
        x += LO[:, None, None]
    else:
        x *= np.float32(90.0)
        x += np.float32(220.0)
    assert x.dtype == np.float32 and x.min() > 0
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, label):
    """Every product of two Results: both None, or equal shape and equal bits."""
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
    return ens.Result(*[None if getattr(res, n) is None else getattr(res, n).cpu().numpy() for n in NAMES])


def reduce(x, group, control, probs, what=None):
    import torch
    rec = x.shape[1:]
    plan = ens.Plan(96, 48, x.shape[0], group, control=control, probs=probs, what=what)  # (reduce_dev takes any record)
    got = to_host(ens.reduce_dev(plan, torch.from_numpy(x).cuda()))
    plan.close()
    for n in NAMES:
        a = getattr(got, n)
        assert a is None or a.shape[-len(rec):] == rec
    return got


@pytest.mark.parametrize("control", [None, CONTROL7], ids=["raw", "response"])
@pytest.mark.parametrize("probs", [[0.5], PROBS16], ids=["1prob", "16probs"])
@pytest.mark.parametrize("nx,ny", [(96, 48), (100, 37)])
def test_grids_against_the_mirror(nx, ny, probs, control):
    """100 x 37: n = 222 000 elements per member, no multiple of a 64-point quantile tile."""
    x = synth(7, (12, 5, ny, nx), seed=nx + len(probs))
    same_bits(reduce(x, GROUP7, control, probs), ens.reference(x, GROUP7, control, probs), f"{nx}x{ny}")


def test_grid_384_against_the_mirror():
    x = synth(2, (12, 5, 192, 384), seed=384)
    same_bits(reduce(x, [0, 0], [1, 1], PROBS16), ens.reference(x, [0, 0], [1, 1], PROBS16), "384x192")


@pytest.mark.parametrize("control", [None, CONTROL7], ids=["raw", "response"])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_raw_lengths_against_the_mirror(n, control):
    """Odd n: rows that are not 8-byte aligned, and a last element whose lane owns it alone; n = 1 and 7: one tile."""
    x = synth(7, (n,), seed=n)
    same_bits(reduce(x, GROUP7, control, [0.0, 0.5, 1.0]), ens.reference(x, GROUP7, control, [0.0, 0.5, 1.0]), f"n={n}")


@pytest.mark.parametrize("probs", [[0.5], PROBS16], ids=["1prob", "16probs"])
@pytest.mark.parametrize("group,control", [(GROUP13, None), (GROUP13, CONTROL13), (GROUP130, None), (GROUP130, CONTROL130)],
                         ids=["sizes1235-raw", "sizes1235-response", "sizes64+65-raw", "sizes64+65-response"])
def test_group_layouts_against_the_mirror(group, control, probs):
    """Sizes 1, 2, 3 and 5 in one plan, interleaved, with members in no group; 64 and 65 members on a 12 x 8 record: a
    whole wavefront's worth of rows and one more, and a sort padded from 65 to 128."""
    x = synth(len(group), (12, 5, 8, 12), seed=len(group))
    got, ref = reduce(x, group, control, probs), ens.reference(x, group, control, probs)
    same_bits(got, ref, f"{len(group)} members")
    sizes = [group.count(g) for g in range(max(group) + 1)]
    assert sizes in ([1, 2, 3, 5], [64, 65])
    if sizes[0] == 1:
        assert not got.var[0].any() and np.array_equal(got.min[0], got.max[0])
    if control is not None and len(group) == 13:  # members 3 and 5 are their own controls: group 0 is member 3 alone
        assert not got.mean[0].any() and not got.quant[0].any()
    p = np.asarray(probs, np.float32)
    for q in np.flatnonzero(p == 0):
        assert np.array_equal(got.quant[:, q], got.min)
    for q in np.flatnonzero(p == 1):
        assert np.array_equal(got.quant[:, q], got.max)


def test_deterministic_and_independent_of_the_batch():
    """A second call gives the same bits; a group reduced alone -- its members in their order behind their outside controls
    in reversed order, nothing else -- gives the bits it has inside the full plan."""
    import torch
    x = synth(13, (12, 5, 8, 12), seed=77)
    xd = torch.from_numpy(x).cuda()
    plan = ens.Plan(96, 48, 13, GROUP13, control=CONTROL13, probs=PROBS16)
    a, b = to_host(ens.reduce_dev(plan, xd)), to_host(ens.reduce_dev(plan, xd))
    same_bits(a, b, "second call")
    plan.close()
    for g in range(4):
        mem = [m for m in range(13) if GROUP13[m] == g]
        others = sorted({CONTROL13[m] for m in mem} - set(mem), reverse=True)
        order = others + mem
        at = {m: i for i, m in enumerate(order)}
        small = ens.Plan(96, 48, len(order), [-1] * len(others) + [0] * len(mem),
                         control=[-1] * len(others) + [at[CONTROL13[m]] for m in mem], probs=PROBS16)
        one = to_host(ens.reduce_dev(small, xd[order].contiguous()))
        small.close()
        for name in NAMES:
            assert np.array_equal(bits(getattr(one, name)[0]), bits(getattr(a, name)[g])), (name, g)
    raw = reduce(x, GROUP13, None, PROBS16)
    for g in range(4):  # without a control map: the group's members alone
        mem = [m for m in range(13) if GROUP13[m] == g]
        one = reduce(x[mem], [0] * len(mem), None, PROBS16)
        for name in NAMES:
            assert np.array_equal(bits(getattr(one, name)[0]), bits(getattr(raw, name)[g])), (name, g)


@pytest.mark.parametrize("rec", [(12, 5, 8, 12), (4097,)], ids=["record", "odd"])
def test_each_single_flag_gives_the_numbers_of_the_full_call(rec):
    """... and the buffers of the products it does not select, handed over filled with NaN, stay untouched."""
    import torch
    x = synth(13, rec, seed=9)
    xd = torch.from_numpy(x).cuda()
    n = int(np.prod(rec))
    full = reduce(x, GROUP13, CONTROL13, PROBS16)
    assert all(getattr(full, name) is not None for name in NAMES)
    for what, names in ((abi.S_MEAN, ("mean",)), (abi.S_VAR, ("var",)), (abi.S_RANGE, ("min", "max")), (abi.S_QUANTILES, ("quant",))):
        plan = ens.Plan(96, 48, 13, GROUP13, control=CONTROL13, probs=PROBS16, what=what)
        one = to_host(ens.reduce_dev(plan, xd))
        buf = [torch.full((4, 16 if name == "quant" else 1, n), float("nan"), dtype=torch.float32, device="cuda") for name in NAMES]
        engine._check(engine.lib().greb_ens_reduce_dev(plan.h, 0, C.c_void_p(xd.data_ptr()), n,
                                                       *[C.c_void_p(t.data_ptr()) for t in buf],
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        plan.close()
        for name, t in zip(NAMES, buf):
            if name in names:
                want = bits(getattr(full, name)).reshape(-1)
                assert np.array_equal(bits(getattr(one, name)), bits(getattr(full, name))), (what, name)
                assert np.array_equal(bits(t.cpu().numpy()).reshape(-1), want), (what, name)
            else:
                assert getattr(one, name) is None, (what, name)
                assert bool(torch.isnan(t).all()), (what, name, "an unselected product's buffer was written")


def test_quantile_group_size_limit_launches_nothing():
    group = [0] * (abi.ENS_MAX_SORTED + 1)
    with pytest.raises(engine.GrebError) as ei:
        ens.Plan(96, 48, len(group), group, probs=[0.5])
    assert ei.value.code == -4 and "4097 members" in str(ei.value)
    ens.Plan(96, 48, len(group), group).close()  # the same plan without GREB_S_QUANTILES


# ---- run_ens on a real engine ----------------------------------------------------------------------------------------
def _same_engine_state(a, b, yr_a, yr_b):
    assert np.array_equal(yr_a, yr_b), "yearly differs"
    for m in range(a.nm):
        assert np.array_equal(a.state(m), b.state(m)), f"state of member {m} differs"


def _year(res, y):
    return ens.Result(*[None if getattr(res, n) is None else getattr(res, n)[:, y] for n in NAMES])


def test_run_ens_against_run(inputs, params):
    """Twin engines, a CO2 sweep that also rises from year to year (a year delivered from the wrong output slot, or before
    its kernels, is not the mirror's), one flux-correction year, three scenario years: both output slots are used and one
    is reused.  Three groups with controls inside and outside them.  Then one more year on each."""
    group, control, probs = [-1, 0, 0, 1, 1, 2, 2], [-1, 0, 0, 0, 3, 5, 1], [0.0, 0.05, 0.5, 0.95, 1.0]
    co2 = (ensemble.co2_sweep(7)[:, None] * (1.0 + 0.1 * np.arange(4))[None]).astype(np.float32)
    plan = ens.Plan(inputs.nx, inputs.ny, 7, group, control=control, probs=probs)
    ea, eb = (engine.Engine(inputs, params, n_members=7) for _ in range(2))
    for e in (ea, eb):
        e.flux_correction(1)
    family = eb.describe()["kernel_family"]
    mon, yr_a = ea.run(3, co2[:, :3])
    res = eb.run_ens(3, co2[:, :3], plan)
    assert res.mean.shape == res.var.shape == res.min.shape == res.max.shape == (3, 3, 12, 5, 48, 96)
    assert res.quant.shape == (3, 3, 5, 12, 5, 48, 96)
    for y in range(3):
        same_bits(_year(res, y), ens.reference(mon[:, y], group, control, probs), f"run_ens year {y}")
    assert not np.array_equal(mon[:, 0], mon[:, 2]), "the years differ"
    assert eb.describe()["kernel_family"] == family == ea.describe()["kernel_family"]
    _same_engine_state(ea, eb, yr_a, res.yearly)
    mon4, yr4_a = ea.run(1, co2[:, 3:])  # the clock continues as after run()
    res4 = eb.run_ens(1, co2[:, 3:], plan)
    same_bits(_year(res4, 0), ens.reference(mon4[:, 0], group, control, probs), "run_ens fourth year")
    _same_engine_state(ea, eb, yr4_a, res4.yearly)
    only = ens.Plan(inputs.nx, inputs.ny, 7, group, what=abi.S_RANGE)  # another plan, no control map, one product
    mon5, yr5_a = ea.run(1, 500.0)
    res5 = eb.run_ens(1, 500.0, only)
    assert res5.mean is None and res5.var is None and res5.quant is None
    same_bits(_year(res5, 0), ens.reference(mon5[:, 0], group, what=abi.S_RANGE), "run_ens range only")
    _same_engine_state(ea, eb, yr5_a, res5.yearly)
    ea.close(); eb.close(); plan.close(); only.close()


def test_run_ens_against_run_g384(inputs384):
    p = abi.default_params(ipx=380, ipy=152)
    probs = [0.0, 0.5, 1.0]
    plan = ens.Plan(384, 192, 2, [0, 0], control=[1, 1], probs=probs)
    ea, eb = (engine.Engine(inputs384, p, n_members=2) for _ in range(2))
    for e in (ea, eb):
        e.flux_correction(1)
    co2 = np.array([[340.0], [680.0]], np.float32)
    mon, yr_a = ea.run(1, co2)
    res = eb.run_ens(1, co2, plan)
    print(f"384x192 circulation: {eb.describe().get('circulation')}")
    same_bits(_year(res, 0), ens.reference(mon[:, 0], [0, 0], [1, 1], probs), "run_ens 384x192")
    assert res.mean[0, 0, :, 0].any(), "member 0 at 340 ppm minus member 1 at 680 ppm is not zero"
    _same_engine_state(ea, eb, yr_a, res.yearly)
    ea.close(); eb.close(); plan.close()


def test_refused_calls_leave_the_engine_alone(inputs, params):
    co2 = [[400.0] * 2, [800.0] * 2]
    ea, eb = (engine.Engine(inputs, params, n_members=2) for _ in range(2))
    other_grid, other_members, plan = ens.Plan(100, 37, 2, [0, 0]), ens.Plan(96, 48, 3, [0, 0, 0]), ens.Plan(96, 48, 2, [0, 0])
    for bad, words in ((other_grid, ("100 x 37", "96 x 48")), (other_members, ("3 members", "has 2"))):
        with pytest.raises(engine.GrebError) as ei:
            ea.run_ens(2, co2, bad)
        assert ei.value.code == -1 and all(w in str(ei.value) for w in words), ei.value
    ra, rb = ea.run_ens(2, co2, plan), eb.run_ens(2, co2, plan)  # ... bit-identical to an untouched twin
    same_bits(ra, rb, "after the refusals")
    _same_engine_state(ea, eb, ra.yearly, rb.yearly)
    for x in (ea, eb, other_grid, other_members, plan):
        x.close()
