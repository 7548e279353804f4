"""GPU: the covariance output (csrc/greb_gram.hip) against gram.reference, the numpy statement of its matrices.

Every comparison with the mirror is for EQUAL BITS of the fp64 output: device and mirror build the same fp32 samples (one
subtraction, one multiply), and then add the same exact fp64 products one by one in the same order -- a fused multiply-add
of an exact product rounds where the add alone does -- so there is nothing for a tolerance to cover.  Every member's
row is distinct, (m + 1) * pattern + noise: a tile put in the wrong place would not show on symmetric or identical data.
The kernel's tile has 64 members a side and stages 32 elements at a time: the member counts sit on both sides of one and
of two tiles, the lengths on both sides of a chunk and of the 16-byte path."""
import numpy as np
import pytest

from greb_climate_model_amd import abi, budget, engine, gram

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64, a.dtype
    return a.view(np.uint64)


def synth(M, R, rec, seed):
    """[M][R] + rec float32: member m is (m + 1) * pattern + noise, patterns of physical magnitude."""
    rng = np.random.default_rng(seed)
    pattern = rng.random((R,) + tuple(rec)) * 0.9 + 2.2
    x = (np.arange(1, M + 1).reshape((M,) + (1,) * (1 + len(rec))) * pattern + rng.standard_normal((M, R) + tuple(rec))).astype(np.float32)
    assert len({row.tobytes() for row in x.reshape(M, -1)}) == M
    return x


def same_bits(got, ref, label):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float64 and got.shape == ref.shape, (label, got.dtype, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    print(f"{label}: {int(bad.sum())} of {bad.size} values differ from the mirror")
    assert not bad.any(), (label, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], ref[bad][:4])


def symmetric(G, label):
    assert np.array_equal(bits(G), bits(np.swapaxes(G, -1, -2))), f"{label}: G differs from its transpose"


def reduce(x, block, use=None, control=None, scale=None, grid=(96, 48), n_blocks=None, repeat=False):
    import torch
    plan = gram.Plan(grid[0], grid[1], x.shape[0], x.shape[1], block, use=use, control=control, scale=scale, n_blocks=n_blocks)
    xd = torch.from_numpy(x).cuda()
    G = gram.reduce_dev(plan, xd)
    torch.cuda.synchronize()
    out = G.cpu().numpy()
    if repeat:
        again = gram.reduce_dev(plan, xd)
        torch.cuda.synchronize()
        assert np.array_equal(bits(again.cpu().numpy()), bits(out)), "a second call gives other bits"
    plan.close()
    assert out.shape == (plan.nb, plan.U, plan.U)
    return out


def own_controls(M, seed):
    """A control for every member, a few of them the member itself."""
    c = np.random.default_rng(seed).integers(0, M, M)
    c[::5] = np.arange(M)[::5]
    return [int(v) for v in c]


@pytest.mark.parametrize("control", [False, True], ids=["raw", "response"])
@pytest.mark.parametrize("M", [1, 2, 17, 63, 64, 65, 130])
def test_member_counts_against_the_mirror(M, control):
    """One member; one tile not full; a full one; one member into the second and the third tile.  Three records of 1 026
    elements (32 chunks and two elements, on the 16-byte path), the outer two in one block: records of one block that
    are not adjacent, the middle one in no block."""
    x = synth(M, 3, (1026,), seed=M)
    ctl = own_controls(M, M) if control else None
    block = [0, -1, 0]
    G = reduce(x, block, control=ctl, repeat=True)
    same_bits(G, gram.reference(x, block, control=ctl), f"M={M}")
    symmetric(G, f"M={M}")
    if control:
        own = [m for m in range(M) if ctl[m] == m]
        assert own and not G[:, own].any() and not G[:, :, own].any() and not np.signbit(G[:, own]).any(), "a member that is its own control"
    assert np.isfinite(G).all() and (control or G.all())


@pytest.mark.parametrize("control", [False, True], ids=["raw", "response"])
@pytest.mark.parametrize("n", [1, 7, 1026, 4097])
def test_lengths_against_the_mirror(n, control):
    """n = 1, 7, 4 097: rows that are not 16-byte aligned, read element by element; 7: less than a chunk; 4 097: 128 chunks
    and one element.  17 members, two blocks."""
    x = synth(17, 4, (n,), seed=n)
    ctl = own_controls(17, n) if control else None
    block = [1, 0, 0, 1]
    G = reduce(x, block, control=ctl)
    same_bits(G, gram.reference(x, block, control=ctl), f"n={n}")
    symmetric(G, f"n={n}")


@pytest.mark.parametrize("scale", [False, True], ids=["plain", "scaled"])
def test_a_whole_384_by_192_map_of_three_members(scale):
    """len = 73 728: 2 304 chunks in one accumulator's chain."""
    x = synth(3, 2, (192, 384), seed=73728)
    s = gram.area_scale(192, 384) if scale else None
    G = reduce(x, [0, 0], control=[2, 2, 0], scale=s, grid=(384, 192))
    same_bits(G, gram.reference(x, [0, 0], control=[2, 2, 0], scale=s), "len=73728")
    symmetric(G, "len=73728")


@pytest.mark.parametrize("control", [False, True], ids=["raw", "response"])
def test_sixteen_blocks_and_a_scale(control):
    """Twenty records on a 12 x 5 map (60 elements: one chunk and 28): sixteen blocks in scrambled order, two of them with
    two records that are not adjacent, two records in no block; a scale with zeros in it."""
    x = synth(17, 20, (5, 12), seed=16)
    block = [7, 3, -1, 15, 0, 7, 11, 4, 12, 1, 9, -1, 2, 14, 5, 10, 3, 6, 13, 8]
    assert sorted(set(block)) == [-1] + list(range(16))
    s = np.random.default_rng(5).random((5, 12), dtype=np.float32)
    s[2, 3:6] = 0
    ctl = own_controls(17, 16) if control else None
    G = reduce(x, block, control=ctl, scale=s, grid=(12, 5))
    assert G.shape == (16, 17, 17)
    same_bits(G, gram.reference(x, block, control=ctl, scale=s), "16 blocks")
    symmetric(G, "16 blocks")
    # a block's numbers do not depend on the other blocks: block 7 alone
    alone = [0 if b == 7 else -1 for b in block]
    same_bits(reduce(x, alone, control=ctl, scale=s, grid=(12, 5))[0], G[7], "block 7 alone")


def test_unused_rows_are_never_read():
    """130 members, every third unused and filled with NaN.  The controls are used members, or member 128: unused, but a
    control, and therefore holding data."""
    M = 130
    use = [int(m % 3 != 2) for m in range(M)]
    use[128] = 0
    control = [128 if m % 2 else (m + 3) % 129 // 3 * 3 for m in range(M)]  # 128, or a used member (a multiple of 3)
    assert all(use[c] or c == 128 for c in control)
    x = synth(M, 3, (8, 12), seed=130)
    clean = reduce(x, [0, 1, 0], use=use, control=control)
    same_bits(clean, gram.reference(x, [0, 1, 0], use=use, control=control), "130 members, every third unused")
    y = x.copy()
    for m in range(M):
        if not use[m] and m != 128:
            y[m] = np.nan
    G = reduce(y, [0, 1, 0], use=use, control=control, repeat=True)
    assert np.isfinite(G).all()
    same_bits(G, clean, "NaN in the unused rows")
    symmetric(G, "130 members")
    assert G.shape == (2, sum(use), sum(use))


@pytest.mark.parametrize("bad", [0, 64, 69])
def test_a_nan_in_one_used_member_stays_in_its_row_and_column(bad):
    """70 members (two tiles): the member at the front, at a tile's first row, in the ragged tile."""
    x = synth(70, 2, (97,), seed=bad)
    ref = reduce(x, [0, 0])
    x[bad, 1, 40] = np.nan
    G = reduce(x, [0, 0])[0]
    nan = np.isnan(G)
    want = np.zeros((70, 70), bool)
    want[bad] = want[:, bad] = True
    assert np.array_equal(nan, want), np.argwhere(nan != want)[:5]
    assert np.array_equal(bits(G[~want]), bits(ref[0][~want]))


def test_independent_of_the_batch():
    """A plan's numbers do not change when unrelated members are appended to x (and left unused), nor when they sit between
    its members."""
    M = 9
    rec = (8, 12)
    x = synth(M, 4, rec, seed=31)
    block = [0, 1, -1, 0]
    control = [(m + 2) % M for m in range(M)]
    s = gram.area_scale(8, 12)
    alone = reduce(x, block, control=control, scale=s, grid=(12, 8))
    same_bits(alone, gram.reference(x, block, control=control, scale=s), "alone")
    more = synth(4, 4, rec, seed=32) * np.float32(3)
    x_app = np.concatenate([x, more])
    got = reduce(x_app, block, use=[1] * M + [0] * 4, control=control + [-1] * 4, scale=s, grid=(12, 8))
    same_bits(got, alone, "appended")
    at = [0, 1, 10, 2, 3, 11, 4, 5, 6, 12, 7, 8, 9]  # the plan's members in their order, strangers between them
    where = {m: i for i, m in enumerate(at)}
    x_mix = np.ascontiguousarray(x_app[at])
    use_mix = [int(m < M) for m in at]
    control_mix = [where[control[m]] if m < M else -1 for m in at]
    same_bits(reduce(x_mix, block, use=use_mix, control=control_mix, scale=s, grid=(12, 8)), alone, "interleaved")


def test_seasons_of_a_climatology_are_valid_input():
    """The products of greb_clim_finish_dev lie as [member][5 seasons][n_vars][ny][nx]: n_records = 5 * n_vars."""
    import torch
    from greb_climate_model_amd import clim
    nx, ny, M = 12, 8, 5
    year = synth(M, 12 * 5, (ny, nx), seed=77).reshape(M, 12, 5, ny, nx)
    cplan = clim.Plan(nx, ny, M, what=abi.C_SEASONS)
    clim.add_year_dev(cplan, torch.from_numpy(year).cuda(), 0)
    seasons = clim.finish_dev(cplan, 1).seasons
    assert tuple(seasons.shape) == (M, 5, 5, ny, nx)
    block = np.tile(np.arange(5), 5)  # one block per variable
    plan = gram.Plan(nx, ny, M, 25, block)
    G = gram.reduce_dev(plan, seasons.reshape(M, 25, ny, nx).contiguous())
    torch.cuda.synchronize()
    same_bits(G.cpu().numpy(), gram.reference(seasons.cpu().numpy().reshape(M, 25, ny, nx), block), "seasons")
    plan.close(); cplan.close()


# ---- run_gram on a real engine ---------------------------------------------------------------------------------------
USE6, CONTROL6 = [1, 1, 1, 0, 0, 0], [3, 4, 5, 3, 4, 5]  # three members above their controls


def _same_engine_state(a, b, yr_a, yr_b):
    assert np.array_equal(yr_a, yr_b), "yearly differs"
    for m in range(a.nm):
        assert np.array_equal(a.state(m), b.state(m)), f"state of member {m} differs"


def _engines(inputs, params, n):
    es = [engine.Engine(inputs, params, n_members=6) for _ in range(n)]
    for e in es:
        e.flux_correction(1)
    return es


# CO2 rising from year to year, another level for each of the three members; their controls stay at 340 ppm
CO2_6x2 = np.asarray([[680.0, 760.0], [560.0, 600.0], [900.0, 1000.0], [340.0, 340.0], [340.0, 340.0], [340.0, 340.0]], np.float32)


def test_run_gram_against_run(inputs, params):
    """Twin engines: two years in one call against the mirror of run()'s records (a year delivered from the wrong output
    slot, or before its kernels, is not the mirror's), then one and one on a third engine."""
    ea, eb, ec = _engines(inputs, params, 3)
    s = gram.area_scale(inputs.ny, inputs.nx)
    block = gram.blocks_by_var(5)
    plan = gram.Plan(inputs.nx, inputs.ny, 6, 60, block, use=USE6, control=CONTROL6, scale=s)
    family = eb.describe()["kernel_family"]
    mon, yr_a = ea.run(2, CO2_6x2)
    res = eb.run_gram(2, CO2_6x2, plan)
    assert res.G.shape == (2, 5, 3, 3) and res.G.dtype == np.float64 and res.vars == budget.STATE_NAMES
    for y in range(2):
        ref = gram.reference(mon[:, y].reshape(6, 60, inputs.ny, inputs.nx), block, use=USE6, control=CONTROL6, scale=s)
        same_bits(res.G[y], ref, f"run_gram year {y}")
        symmetric(res.G[y], f"run_gram year {y}")
    assert not np.array_equal(res.G[0], res.G[1]) and (res.G[:, 0] > 0).all(), "the years differ; the Tsurf responses are not zero"
    assert eb.describe()["kernel_family"] == family == ea.describe()["kernel_family"]
    _same_engine_state(ea, eb, yr_a, res.yearly)
    r0, r1 = ec.run_gram(1, CO2_6x2[:, :1], plan), ec.run_gram(1, CO2_6x2[:, 1:], plan)  # the clock continues as after run()
    same_bits(r0.G[0], res.G[0], "1 + 1 years, first")
    same_bits(r1.G[0], res.G[1], "1 + 1 years, second")
    _same_engine_state(eb, ec, res.yearly[:, 1:], r1.yearly)
    raw = gram.Plan(inputs.nx, inputs.ny, 6, 60, [0] * 60)  # another plan: all six members, one block, no control, no scale
    mon3, yr3_a = ea.run(1, 500.0)
    res3 = eb.run_gram(1, 500.0, raw)
    same_bits(res3.G[0], gram.reference(mon3[:, 0].reshape(6, 60, -1), [0] * 60), "raw plan")
    _same_engine_state(ea, eb, yr3_a, res3.yearly)
    for x in (ea, eb, ec, plan, raw):
        x.close()


def test_run_gram_of_budget_combinations_against_run_budget(inputs, params):
    """records = the surface and the atmospheric net flux: against the mirror of run_budget's records, combined by
    budget.combine_reference."""
    ea, eb = _engines(inputs, params, 2)
    cb = budget.combo({"surface_net": budget.SURFACE_NET, "atmos_net": budget.ATMOS_NET})
    block = gram.blocks_by_var(2)
    plan = gram.Plan(inputs.nx, inputs.ny, 6, 24, block, use=USE6, control=CONTROL6, scale=gram.area_scale(inputs.ny, inputs.nx))
    _, bud, yr_a = ea.run_budget(2, CO2_6x2, want_monthly=False)
    res = eb.run_gram(2, CO2_6x2, plan, records=cb)
    assert res.G.shape == (2, 2, 3, 3) and res.vars == ("surface_net", "atmos_net")
    x = budget.combine_reference(cb, bud)  # [6][2][12][2][ny][nx]
    for y in range(2):
        ref = gram.reference(x[:, y].reshape(6, 24, inputs.ny, inputs.nx), block, use=USE6, control=CONTROL6, scale=plan.scale)
        same_bits(res.G[y], ref, f"run_gram of the net fluxes, year {y}")
    assert (np.diagonal(res.G, axis1=-2, axis2=-1) > 0).all()
    _same_engine_state(ea, eb, yr_a, res.yearly)
    with pytest.raises(engine.GrebError) as ei:  # the plan of the state records does not fit two variables
        eb.run_gram(1, CO2_6x2[:, :1], gram.Plan(inputs.nx, inputs.ny, 6, 60, gram.blocks_by_var(5)), records=cb)
    assert ei.value.code == -1 and "n_records = 60" in str(ei.value) and "12 * 2 = 24" in str(ei.value), ei.value
    for x in (ea, eb, plan):
        x.close()


def test_refused_calls_leave_the_engine_alone(inputs, params):
    ea, eb = _engines(inputs, params, 2)
    block = gram.blocks_by_var(5)
    plan = gram.Plan(96, 48, 6, 60, block, use=USE6, control=CONTROL6)
    other_grid, other_members = gram.Plan(100, 37, 6, 60, block), gram.Plan(96, 48, 7, 60, block)
    other_records = gram.Plan(96, 48, 6, 25, [0] * 25)
    for bad, words in ((other_grid, ("100 x 37", "96 x 48")), (other_members, ("7 members", "has 6")),
                       (other_records, ("n_records = 25", "12 * 5 = 60"))):
        with pytest.raises(engine.GrebError) as ei:
            ea.run_gram(2, CO2_6x2, bad)
        assert ei.value.code == -1 and all(x in str(ei.value) for x in words), ei.value
    yearly = np.zeros((6, 2, 2), np.float32)
    assert engine.lib().greb_engine_run_gram(ea.h, 2, abi.fptr(CO2_6x2), plan.h, None, abi.fptr(yearly)) == -1
    assert "run_gram: `G` is NULL" in engine.lib().greb_engine_last_error(ea.h).decode()
    ra, rb = ea.run_gram(2, CO2_6x2, plan), eb.run_gram(2, CO2_6x2, plan)  # ... bit-identical to an untouched twin
    same_bits(ra.G, rb.G, "after the refusals")
    _same_engine_state(ea, eb, ra.yearly, rb.yearly)
    for x in (ea, eb, other_grid, other_members, other_records, plan):
        x.close()
