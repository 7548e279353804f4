"""GPU: stochastic surface heat-flux forcing per member (greb_engine_set_noise_tables, greb_engine_set_member_noise,
greb_engine_get_noise), in the scenario phase.

1. The generator through the query: Engine.noise against noise.field, bit for bit -- cells, holds, the year boundary, a step
   whose high counter word is not zero, a season with a zero; on the fused engine, the bands and the 192x48 strips.
2. The kernels use that generator: a noisy year against tests/noise_mirror.py, FAST and STRICT.
3. amp = 0 through the noise path equals the unforced one-member engine, bit for bit, on every engine kind.
4. Reproducibility, bit for bit: a seed does not care which member carries it, how the launch is dealt or how the years are
   split into run calls; two seeds differ; sigma and 2 sigma at half the amplitude are the same weather.
5. run, run_budget and run_diag are the same run.
6. A noisy member beside a plain member: each equals its one-member engine.
7. Errors: every validation rule, a rejected call changes nothing, clearing returns to the default kernels, the
   flux-correction phase ignores all of it, and the scenario clock -- not the flux clock -- drives the counter.
Every case: corrections from a shared spun-up state (set_corrections), one scenario year (two where the split is the
subject), at most four members."""
import os

import numpy as np
import pytest

import budget_mirror
import noise_mirror
from conftest import rms, yearly_close
from greb_climate_model_amd import noise
from test_gpu_members import TOL  # RMS of a monthly-mean field: Tsurf, Tair, Tocean [K], q [kg/kg], albedo -- imported, not copied
from test_gpu_sst import ALL_KINDS, KIND_IDS, KINDS, kind_inputs, same, states, unforced  # the engines and their shared plain years

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CO2 = 680.0
MODES = [False, True]  # strict
ids = lambda s: "strict" if s else "fast"
SEED = 0x5EED0123456789AB


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


def noise_engine(eng_mod, inputs, params, kind, strict, n, start, sigma, season, cell, hold, members, **kw):
    inp, p = kind_inputs(kind, inputs, params)
    e = eng_mod.Engine(inp, p, n_members=n, strict=strict, **KINDS[kind][0], **kw)
    if start is not None:
        e.set_corrections(start["corr"], start["state"])
    e.set_noise_tables(sigma, season, cell, hold)
    e.set_member_noise(members)
    return e


def case2_members(n=1, **over):
    return [dict(dict(pattern=0, amp=1.0, seed=SEED), **over) for _ in range(n)]


# ------------------------------------------------------------------------------------------------ 1. the generator
CELLS = [(1, 1), (2, 1), (4, 3), (4, 5)]
HOLDS = [1, 6, 7]
STEPS = [0, 3, 729, 730, 2 ** 32 + 5]  # 3: where the season is zero


@pytest.mark.parametrize("kind", ["fused", "bands", "strips192"])
def test_query_equals_the_numpy_generator(eng_mod, params, inputs, kind):
    """Twelve patterns (every cell with every hold), each with its own sigma -- changing along every row and every column --
    and its own season with a zero at step 3; the member's amplitude and both seed words change from pattern to pattern."""
    inp, p = kind_inputs(kind, inputs, params)
    ny, nx = inp.ny, inp.nx
    rng = np.random.default_rng(11)
    combos = [(c, h) for c in CELLS for h in HOLDS]
    j, i = np.arange(ny, dtype=np.float32)[:, None], np.arange(nx, dtype=np.float32)[None, :]
    sigma = np.stack([(5.0 + 0.37 * j + 0.011 * i + k + rng.random((ny, nx))).astype(np.float32) for k in range(len(combos))])
    assert (np.diff(sigma, axis=1) != 0).all() and (np.diff(sigma, axis=2) != 0).all()
    season = (0.5 + rng.random((len(combos), 730))).astype(np.float32)
    season[:, 3] = 0.0
    e = noise_engine(eng_mod, inputs, params, kind, False, 2, None, sigma, season, [c for c, _ in combos], [h for _, h in combos], None)
    assert e.describe()["engine"] == KINDS[kind][1]
    seeds = noise.seeds(len(combos), 99)
    for k, (cell, hold) in enumerate(combos):
        amp = 0.75 + 0.125 * k
        e.set_member_noise([{}, {"pattern": k, "amp": amp, "seed": seeds[k]}])
        want = noise.field(sigma[k], season[k], cell, hold, seeds[k], amp, STEPS)
        for t, step in enumerate(STEPS):
            got = e.noise(1, step)
            assert got.dtype == np.float32 and np.array_equal(got, want[t]), (kind, cell, hold, step, float(np.abs(got - want[t]).max()))
        assert not want[1].any() and want[0].any() and not np.array_equal(want[2], want[0])
    assert e.describe()["noise"] == {"patterns": 12, "noisy_members": 1}
    e.close()


# ------------------------------------------------------------------------------------------------ 2. against the mirror
@pytest.fixture(scope="module")
def mirror(oracle_lib, inputs, params):
    """Computed once, shared, never changed.  From the oracle's flux-correction year, one scenario year each at 680 ppm: case
    2's noise (noise_mirror.case2) and the year without it."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    args = (inputs.tclim, inputs.z_topo, inputs.sw_solar)
    noisy = noise_mirror.run_year(o, start, CO2, noise_mirror.case2(inputs, SEED)[4], *args)
    plain = noise_mirror.run_year(o, start, CO2, None, *args)
    o.close()
    for a in noisy + plain + (start.corr, start.state5):
        a.setflags(write=False)
    return dict(start=dict(corr=start.corr, state=start.state5), noisy=noisy, plain=plain)


_case2 = {}


def case2_engine(eng_mod, inputs, params, start, strict, n=1, members=None, **kw):
    sigma, season, cell, hold, _ = noise_mirror.case2(inputs, SEED)
    return noise_engine(eng_mod, inputs, params, "fused", strict, n, start, sigma, season, cell, hold, members or case2_members(n), **kw)


def case2_run(eng_mod, inputs, params, mirror, strict):
    """Case 2 as a one-member engine from the mirror's start: (monthly, yearly, state), computed once per mode."""
    if strict not in _case2:
        e = case2_engine(eng_mod, inputs, params, mirror["start"], strict)
        mon, yr = e.run(1, CO2)
        _case2[strict] = (mon[0], yr[0], e.state(0))
        e.close()
    return _case2[strict]


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_noisy_run_against_the_mirror(eng_mod, params, inputs, mirror, strict):
    """Cell (2, 3), hold 6, sigma 30 W/m2 over ocean and 10 over land.  The measured RMS of every field is printed and written
    to profiles/noise_parity_numbers.txt."""
    mon, yr, st = case2_run(eng_mod, inputs, params, mirror, strict)
    p = eng_mod.Engine(inputs, params, strict=strict)
    p.set_corrections(mirror["start"]["corr"], mirror["start"]["state"])
    p.run(1, CO2)
    plain_state = p.state(0)
    p.close()
    assert not np.array_equal(st, plain_state)  # the noisy member's state is not the plain member's
    tag = f"noisy run vs mirror {ids(strict).upper()}"
    lines = []
    for i, tol in enumerate(TOL):
        r = rms(mon[0, :, i], mirror["noisy"][0][:, i])
        lines.append(f"{tag} field {i}: RMS {r:.3e} (bar {tol:.0e})")
        print(lines[-1])
    print(f"{tag} yearly: engine {yr.tolist()} mirror {mirror['noisy'][3].tolist()}")
    for i, tol in enumerate(TOL):
        # the noise is in there: the mirror's plain December differs by more than the bar
        assert rms(mirror["noisy"][0][11, i], mirror["plain"][0][11, i]) > tol, i
        assert rms(mon[0, :, i], mirror["noisy"][0][:, i]) < tol, (tag, i)
    yearly_close(yr[0], mirror["noisy"][3], strict)
    path = os.path.join(ROOT, "profiles", "noise_parity_numbers.txt")
    try:  # (a record for the repository, not part of the check; a read-only tree keeps the committed one)
        old = [l for l in open(path).read().splitlines() if not l.startswith(tag)] if os.path.exists(path) else \
            ["# stochastic heat flux (sigma 30 W/m2 over ocean, 10 over land, cell (2, 3), hold 6, a season of 1 ... 1.25) at 680 ppm against",
             "# tests/noise_mirror.py, 96x48 fused member kernel, one scenario year: RMS of the monthly records per field",
             "# (tests/test_gpu_noise.py::test_noisy_run_against_the_mirror)"]
        open(path, "w").write("\n".join(old + lines) + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------ 3. amp = 0
@pytest.mark.parametrize("kind,strict", ALL_KINDS, ids=KIND_IDS)
def test_amp_zero_equals_the_unforced_engine(eng_mod, params, inputs, kind, strict):
    """Two members: the noise path at amp 0 (N = +-0, TF + N = TF); none.  Both run the forcing-aware kernels and equal the
    plain engine."""
    inp, p = kind_inputs(kind, inputs, params)
    ref = unforced(eng_mod, inputs, params, kind, strict)
    sigma = np.full((inp.ny, inp.nx), 25.0, np.float32)
    e = noise_engine(eng_mod, inputs, params, kind, strict, 2, ref, sigma, None, (2, 3), 6, [{"pattern": 0, "amp": 0.0, "seed": SEED}, {}])
    d = e.describe()
    assert d["noise"] == {"patterns": 1, "noisy_members": 1} and d["kernel_family"]["scenario"] == "forcing", d
    assert np.abs(e.noise(0, 0)).max() == 0.0
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    for m in range(2):
        same((mon[m], yr[m], st[m]), ref["run"], f"{kind} {ids(strict)} amp-0 member {m}")


# ------------------------------------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_a_realisation_is_a_function_of_the_seed_alone(eng_mod, params, inputs, mirror, strict):
    """Seed s as member 0 of a one-member engine, and as members 1 (on 2 sigma at half the amplitude) and 2 of a three-member
    engine whose member 0 has another seed -- once as launched by default, once dealt by force on another chunk schedule."""
    from greb_climate_model_amd import abi
    one = case2_run(eng_mod, inputs, params, mirror, strict)
    sigma, season, cell, hold, _ = noise_mirror.case2(inputs, SEED)
    members = [{"pattern": 0, "seed": noise.seeds(1, 4)[0]}, {"pattern": 1, "amp": 0.5, "seed": SEED}, {"pattern": 0, "seed": SEED}]
    for dealt in (False, True):
        e = noise_engine(eng_mod, inputs, params, "fused", strict, 3, mirror["start"], np.stack([sigma, 2 * sigma]), np.stack([season, season]),
                         cell, hold, members)
        if dealt:
            e.set_dealing(2, abi.CHUNKS_EQUAL, force=True)
        mon, yr = e.run(1, CO2)
        st = states(e)
        if dealt:
            assert e.describe()["dealing"]["dealt_launches"] >= 1, e.describe()
        e.close()
        label = f"{ids(strict)} {'dealt' if dealt else 'default'}"
        same((mon[2], yr[2], st[2]), one, label + ": seed s as member 2 of 3")
        same((mon[1], yr[1], st[1]), one, label + ": seed s on 2 sigma at half the amplitude")
        assert not np.array_equal(mon[0], mon[2]) and rms(mon[0, 0, 11, 0], mon[2, 0, 11, 0]) > 1e-2  # two seeds differ


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_run_two_years_equals_two_runs_of_one(eng_mod, params, inputs, mirror, strict):
    a = case2_engine(eng_mod, inputs, params, mirror["start"], strict)
    mon_a, yr_a = a.run(2, CO2)
    st_a = a.state(0)
    a.close()
    b = case2_engine(eng_mod, inputs, params, mirror["start"], strict)
    m1, y1 = b.run(1, CO2)
    m2, y2 = b.run(1, CO2)
    st_b = b.state(0)
    b.close()
    same((mon_a[0, 0], yr_a[0, 0], st_a), (m1[0, 0], y1[0, 0], st_b), f"{ids(strict)} first year")
    same((mon_a[0, 1], yr_a[0, 1], st_a), (m2[0, 0], y2[0, 0], st_b), f"{ids(strict)} second year")
    same((m1[0], y1[0]), case2_run(eng_mod, inputs, params, mirror, strict)[:2], f"{ids(strict)} the shared first year")


# ------------------------------------------------------------------------------------------------ 5. same run
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_run_run_budget_and_run_diag_are_the_same_run(eng_mod, params, inputs, mirror, strict):
    from greb_climate_model_amd import abi, diag
    mon, yr, st = case2_run(eng_mod, inputs, params, mirror, strict)
    e = case2_engine(eng_mod, inputs, params, mirror["start"], strict)
    mon_b, bud, yr_b = e.run_budget(1, CO2)
    st_b = e.state(0)
    e.close()
    same((mon_b[0], yr_b[0], st_b), (mon, yr, st), f"{ids(strict)} run_budget against run")
    assert bud.shape[3] == abi.NBUDGET == 13 and np.isfinite(bud).all()
    e = case2_engine(eng_mod, inputs, params, mirror["start"], strict)
    plan = diag.Plan(inputs.nx, inputs.ny)
    res = e.run_diag(1, CO2, plan, abi.D_ANNUAL)
    st_d = e.state(0)
    e.close(); plan.close()
    assert np.array_equal(res.yearly[0], yr) and np.array_equal(st_d, st)
    ann = diag.reduce_reference(mon)[2]  # [1][5][ny][nx], fp64
    ulp = np.spacing(np.abs(ann).astype(np.float32)).astype(np.float64)
    assert (np.abs(res.annual[0].astype(np.float64) - ann) / ulp).max() <= 1.0


# ------------------------------------------------------------------------------------------------ 6. beside a plain member
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_noisy_member_beside_a_plain_member(eng_mod, params, inputs, mirror, strict):
    e = case2_engine(eng_mod, inputs, params, mirror["start"], strict, 2, [{}, case2_members()[0]])
    assert e.describe()["noise"] == {"patterns": 1, "noisy_members": 1}
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    same((mon[1], yr[1], st[1]), case2_run(eng_mod, inputs, params, mirror, strict), f"{ids(strict)} noisy member")
    p = eng_mod.Engine(inputs, params, strict=strict)
    p.set_corrections(mirror["start"]["corr"], mirror["start"]["state"])
    pm, py = p.run(1, CO2)
    ps = p.state(0)
    assert p.describe()["kernel_family"]["scenario"] == "default"
    p.close()
    same((mon[0], yr[0], st[0]), (pm[0], py[0], ps), f"{ids(strict)} plain member beside it")


# ------------------------------------------------------------------------------------------------ 7. errors and scope
def _rejected(eng_mod, e, rc, *words):
    assert rc == -1, rc
    msg = eng_mod.lib().greb_engine_last_error(e.h).decode()
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_errors_leave_the_engine_as_it_was(eng_mod, params, inputs, strict):
    import ctypes as C
    from greb_climate_model_amd import abi
    L = eng_mod.lib()
    ny, nx = inputs.ny, inputs.nx
    ref = unforced(eng_mod, inputs, params, "fused", strict)
    s2, season2, cell, hold, _ = noise_mirror.case2(inputs, SEED)
    sigma = np.ascontiguousarray(np.stack([np.ones_like(s2), s2]))
    season = np.ascontiguousarray(np.stack([season2, season2]))
    good = [{"pattern": 1, "amp": 1.0, "seed": SEED}]

    def engine():
        return noise_engine(eng_mod, inputs, params, "fused", strict, 1, ref, sigma, season, cell, hold, good)

    e = engine()
    before = e.describe()
    assert before["forcing"] == {"patterns": 0, "solar_tables": 0, "forced_members": 0} and before["sst"] == {"patterns": 0, "prescribed_members": 0}
    ptr = lambda x: None if x is None else abi.fptr(x)
    ints = lambda v: None if v is None else (C.c_int32 * len(v))(*v)
    tables = lambda n, s, t, cx=None, cy=None, h=None: L.greb_engine_set_noise_tables(e.h, n, ptr(s), ptr(t), ints(cx), ints(cy), ints(h))

    def member(**kw):
        f = (abi.GrebMemberNoise * 1)()
        f[0].pattern, f[0].amp = -1, 1.0
        for k, v in kw.items():
            setattr(f[0], k, v)
        return L.greb_engine_set_member_noise(e.h, f)

    big = np.ones((17, 5, 12), np.float32)  # (rejected before anything of it is read)
    _rejected(eng_mod, e, tables(17, big, None), "n_patterns", "17")
    _rejected(eng_mod, e, tables(-1, None, None), "n_patterns", "-1")
    _rejected(eng_mod, e, tables(2, None, season), "sigma is NULL")
    for bad, word in ((np.nan, "nan"), (np.inf, "inf"), (-0.5, "-0.5")):
        a = sigma.copy(); a[1, 7, 5] = bad
        _rejected(eng_mod, e, tables(2, a, None), "sigma", "pattern 1", "row 7", "column 5", word)
        s = season.copy(); s[0, 364] = bad
        _rejected(eng_mod, e, tables(2, sigma, s), "season", "pattern 0", "step 365", word)
    for bad in (0, 3, 8, -1):
        _rejected(eng_mod, e, tables(2, sigma, None, [1, bad]), "cell_x", "pattern 1", str(bad))
    for bad in (0, ny + 1, -2):
        _rejected(eng_mod, e, tables(2, sigma, None, None, [bad, 1]), "cell_y", "pattern 0", str(bad))
    for bad in (0, -6):
        _rejected(eng_mod, e, tables(2, sigma, None, None, None, [1, bad]), "hold", "pattern 1", str(bad))
    _rejected(eng_mod, e, tables(1, sigma[:1], None), "member 0", "pattern 1")  # fewer patterns than a member names
    _rejected(eng_mod, e, member(pattern=2), "member 0", "pattern 2")
    _rejected(eng_mod, e, member(pattern=-2), "member 0", "pattern -2")
    for bad, word in ((np.nan, "amp nan"), (np.inf, "amp inf")):
        _rejected(eng_mod, e, member(pattern=0, amp=bad), "member 0", word)
    out = np.zeros((ny, nx), np.float32)
    _rejected(eng_mod, e, L.greb_engine_get_noise(e.h, 1, 0, abi.fptr(out)), "member 1")
    _rejected(eng_mod, e, L.greb_engine_get_noise(e.h, -1, 0, abi.fptr(out)), "member -1")
    _rejected(eng_mod, e, L.greb_engine_get_noise(e.h, 0, -5, abi.fptr(out)), "step -5")
    _rejected(eng_mod, e, L.greb_engine_get_noise(e.h, 0, 0, None), "out is NULL")
    with pytest.raises(eng_mod.GrebError):
        e.set_member_noise([{"pattern": 0, "amplitude": 1.0}])
    with pytest.raises(eng_mod.GrebError):
        e.set_member_noise([{}, {}])
    with pytest.raises(eng_mod.GrebError):
        e.set_noise_tables(sigma[:, :-1])
    with pytest.raises(eng_mod.GrebError):
        e.set_noise_tables(sigma, season[:1])
    with pytest.raises(eng_mod.GrebError):
        e.set_noise_tables(sigma, None, [(1, 1)] * 3)
    assert e.describe() == before
    want0 = noise.field(s2, season2, cell, hold, SEED, 1.0, (0,))[0]
    assert np.array_equal(e.noise(0, 0), want0)  # the tables and the member's words are the ones set before
    got = e.run(1, CO2) + (e.state(0),)
    # ... equals the run of an engine that never made the rejected calls
    f = engine()
    want = f.run(1, CO2) + (f.state(0),)
    f.close()
    same(got, want, f"{ids(strict)} after the rejected calls")
    assert not np.array_equal(got[0][0], ref["run"][0])  # (and that run was noisy)
    # clearing returns to the default kernels; tables may then shrink, and the indices are validated against the new ones
    e.set_member_noise(None)
    d = e.describe()
    assert d["noise"] == {"patterns": 2, "noisy_members": 0} and d["kernel_family"]["scenario"] == "default", d
    with pytest.raises(eng_mod.GrebError):
        e.noise(0, 0)  # the member names no pattern any more
    e.set_noise_tables(sigma[:1])
    assert e.describe()["noise"] == {"patterns": 1, "noisy_members": 0}
    _rejected(eng_mod, e, member(pattern=1), "member 0", "pattern 1")
    e.set_corrections(ref["corr"], ref["state"])
    mon, yr = e.run(1, CO2)  # the second scenario year of this engine's clock: the year's records are those of a first year
    same((mon[0], yr[0], e.state(0)), ref["run"], f"{ids(strict)} cleared noise")
    e.set_noise_tables(None)
    d = e.describe()
    assert d["noise"] == {"patterns": 0, "noisy_members": 0} and d["forcing"] == before["forcing"] and d["sst"] == before["sst"]
    e.close()


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_flux_correction_ignores_the_noise_and_its_clock_does_not_drive_the_counter(eng_mod, params, inputs, strict):
    """A noisy and a plain member through one flux-correction year: corrections, state and yearly are the plain engine's, and
    the members still share one correction set.  Then the scenario year: the noisy member equals a noisy engine that never ran
    a flux-correction year but was given its result -- so the flux clock does not enter the counter.  That such an engine's
    first scenario step takes Engine.noise(m, 0) is test_noisy_run_against_the_mirror's: its mirror adds noise.field of steps
    0 ... 729, which test_query_equals_the_numpy_generator holds Engine.noise to."""
    ref = unforced(eng_mod, inputs, params, "fused", strict)
    e = case2_engine(eng_mod, inputs, params, None, strict, 2, [case2_members()[0], {}])
    d = e.describe()
    assert d["noise"]["noisy_members"] == 1 and d["correction_sets"] == 1 and d["kernel_family"]["flux_correction"] != "forcing", d
    yf = e.flux_correction(1)
    for m in range(2):
        corr, st = e.get_corrections(m)
        assert np.array_equal(corr, ref["corr"]) and np.array_equal(st, ref["state"]) and np.array_equal(yf[m], ref["flux_yearly"][0]), m
    mon, yr = e.run(1, CO2)
    st = states(e)
    e.close()
    same((mon[1], yr[1], st[1]), ref["run"], f"{ids(strict)} plain member after the flux year")
    f = case2_engine(eng_mod, inputs, params, ref, strict)  # flux clock 0, scenario clock 0
    assert not np.array_equal(f.noise(0, 0), f.noise(0, 730))
    fm, fy = f.run(1, CO2)
    fs = f.state(0)
    f.close()
    same((mon[0], yr[0], st[0]), (fm[0], fy[0], fs), f"{ids(strict)} noisy member after the flux year")
    assert not np.array_equal(mon[0], mon[1])
