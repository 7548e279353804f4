"""GPU: the edge year (tests/edge_workload.py; yardsticks checked in tests/test_edge_cpu.py) -- a model year that takes the
branches of the step the plain workload never reaches: the humidity clamp of the update (src/greb.f90:265), z_topo == 0,
a glacier on an ocean point, a warm ocean whose mixed layer stands still.  96x48, every case 1 + 1 years at most.

a. Fused member kernel and latitude bands, FAST and STRICT, created on the edge inputs: their own flux-correction year and a
   scenario year against the REFERENCE's output on those inputs (tests/golden/edge_g96.npz).
b. The same four engines from the oracle's spun-up state with the EDITED corrections: the year in which the clamp fires,
   against the mirror year (tests/budget_mirror.py); run_budget is the same run.
c. Every step-kernel variant (test_gpu_variants' two-member construction) on that year: the plain member beside a feature
   is the one-member engine of (b), bit for bit.
d. A member on a boundary set holding the edge z_topo, glacier and mldclim equals the engine created on the edge inputs.
e. point_physics at the four ice thresholds and one ulp to either side, at points of every class, against the oracle.
f. Fused STRICT against bands STRICT, bit for bit (three members with their own physics and CO2, plain and edge inputs);
   FAST with the circulation switched off likewise.
Oracle and mirror results are computed once per module, every one-member engine result once per engine kind and mode."""
import numpy as np
import pytest

import budget_mirror
import edge_workload
from conftest import load_golden, yearly_close
from test_gpu_boundary import alone, same
from test_gpu_forcing import KINDS
from test_gpu_parity import _check_run  # its TOL: Tsurf, Tair, Tocean 1e-4 K, q 2e-8, albedo 1e-6 (RMS)
from test_gpu_variants import CASES, two_members

pytestmark = pytest.mark.gpu

CO2 = 680.0
MODES = [False, True]  # strict
ENGINES = ["fused", "bands"]
ids = lambda s: "strict" if s else "fast"


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def edge(oracle_lib, inputs, params):
    """Computed once, shared, never changed: the edge inputs, the oracle's flux-correction year on them (the start), the
    edited corrections, and the mirror's year from that start with those corrections, with its census."""
    inp, pts = edge_workload.make_edge_inputs(inputs, params)
    o = oracle_lib.Oracle(inp, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    start.corr = edge_workload.edit_corrections(start.corr)
    census = edge_workload.Census(inp, params)
    monthly, budget, state = budget_mirror.run_year(o, start, CO2, observer=census)
    o.close()
    print("\n".join(census.lines()))
    assert census.counts["humidity clamp of the update"] == 4 * 86 and census.min_margin > 0.01
    for a in (monthly, budget, state, start.corr, start.state5):
        a.setflags(write=False)
    return dict(inp=inp, pts=pts, start=start, monthly=monthly, budget=budget, state=state)


_own_year, _clamp_year = {}, {}


def frozen(out):
    for a in out.values():
        a.setflags(write=False)
    return out


def own_year(eng_mod, edge, params, kind, strict):
    """A one-member engine CREATED on the edge inputs: its flux-correction year and its scenario year at 680 ppm."""
    k = (kind, strict)
    if k not in _own_year:
        e = eng_mod.Engine(edge["inp"], params, strict=strict, **KINDS[kind][0])
        assert e.describe()["engine"] == KINDS[kind][1], e.describe()
        yf = e.flux_correction(1)
        corr, st = e.get_corrections(0)
        mon, yr = e.run(1, CO2)
        _own_year[k] = frozen(dict(flux_yearly=yf[0], corr=corr, spun_up=st, monthly=mon[0], yearly=yr[0], state=e.state(0)))
        e.close()
    return _own_year[k]


def clamp_year(eng_mod, edge, params, kind, strict):
    """A one-member default engine on the edge inputs, from the oracle's spun-up state with the edited corrections: one
    scenario year through run, and the same year through run_budget."""
    k = (kind, strict)
    if k not in _clamp_year:
        e = eng_mod.Engine(edge["inp"], params, strict=strict, **KINDS[kind][0])
        assert e.describe()["engine"] == KINDS[kind][1], e.describe()
        e.set_corrections(edge["start"].corr, edge["start"].state5)
        mon, yr = e.run(1, CO2)
        st = e.state(0)
        e.set_corrections(None, edge["start"].state5)
        mon_b, bud, yr_b = e.run_budget(1, CO2)
        _clamp_year[k] = frozen(dict(monthly=mon[0], yearly=yr[0], state=st, monthly_b=mon_b[0], yearly_b=yr_b[0], state_b=e.state(0),
                                     budget=bud[0]))
        e.close()
    return _clamp_year[k]


# ------------------------------------------------------------------------------------------------ a. against the reference
@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("kind", ENGINES)
def test_edge_inputs_against_the_reference(eng_mod, edge, params, kind, strict):
    g = load_golden("edge_g96.npz")
    got = own_year(eng_mod, edge, params, kind, strict)
    _check_run(got["monthly"][0], g["monthly"], f"a. {kind} {ids(strict)}")
    yearly_close(np.concatenate([got["flux_yearly"], got["yearly"]]), g["yearly"], strict)
    assert np.isfinite(got["monthly"]).all() and np.isfinite(got["state"]).all()


# ------------------------------------------------------------------------------------------------ b. the clamp year
@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("kind", ENGINES)
def test_clamp_year_against_the_mirror(eng_mod, edge, params, kind, strict):
    got = clamp_year(eng_mod, edge, params, kind, strict)
    _check_run(got["monthly"][0], edge["monthly"], f"b. {kind} {ids(strict)}")
    same(dict(monthly=got["monthly_b"], yearly=got["yearly_b"], state=got["state_b"]),
         dict(monthly=got["monthly"], yearly=got["yearly"], state=got["state"]), f"{kind} {ids(strict)}: run_budget is the same run")
    assert got["budget"].shape == (1, 12, 13, 48, 96) and np.isfinite(got["budget"]).all()


# ------------------------------------------------------------------------------------------------ c. every variant
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("kind", ENGINES)
def test_plain_member_beside_a_feature_on_the_clamp_year(eng_mod, edge, params, kind, strict, case):
    want = clamp_year(eng_mod, edge, params, kind, strict)
    label = f"{kind} {ids(strict)} {case}"
    e = two_members(eng_mod, edge["inp"], params, kind, strict, case)
    assert e.describe()["kernel_family"] == CASES[case], (label, e.describe())
    e.set_corrections(edge["start"].corr, edge["start"].state5)
    mon, yr = e.run(1, CO2)
    same(dict(monthly=mon[0], yearly=yr[0], state=e.state(0)), {k: want[k] for k in ("monthly", "yearly", "state")}, label + ": run")
    if case != "nothing":  # the feature acts: member 1 is another run
        assert not np.array_equal(mon[1], mon[0]), label
    e.set_corrections(None, edge["start"].state5)
    mon_b, bud, yr_b = e.run_budget(1, CO2)
    same(dict(monthly=mon_b[0], yearly=yr_b[0], state=e.state(0)), {k: want[k] for k in ("monthly", "yearly", "state")}, label + ": run_budget")
    assert np.array_equal(mon_b[1], mon[1]) and np.isfinite(bud).all(), label
    e.close()


# ------------------------------------------------------------------------------------------------ d. a boundary set
@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_member_on_the_edge_set_equals_the_engine_created_on_the_edge_inputs(eng_mod, edge, inputs, params, strict):
    """The derived fields of a set (wz_air, wz_vapor, z_ocean, the initial cap_surf) at z_topo == 0 and on a mixed layer that
    stands still: made when the set is added, not when the engine is created."""
    inp = edge["inp"]
    e = eng_mod.Engine(inputs, params, n_members=2, strict=strict)
    s = e.add_boundary_set(z_topo=inp.z_topo, glacier=inp.glacier, mldclim=inp.mldclim)
    e.set_member_boundary([0, s], reinit=True)
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(2)]
    mon, yr = e.run(1, CO2)
    got = [dict(flux_yearly=yf[m], corr=spun[m][0], spun_up=spun[m][1], monthly=mon[m], yearly=yr[m], state=e.state(m)) for m in range(2)]
    e.close()
    same(got[1], own_year(eng_mod, edge, params, "fused", strict), f"{ids(strict)} member on the edge set")
    same(got[0], alone(eng_mod, inputs, params, "fused", strict, "plain"), f"{ids(strict)} member on the engine's own data")


# ------------------------------------------------------------------------------------------------ e. routine level
THRESHOLDS = ("Tl_ice1", "Tl_ice2", "To_ice1", "To_ice2")


def threshold_field(edge, params):
    """Tsurf [ny][nx]: within every class of points the twelve values (threshold, one ulp down, one ulp up) x four in turn.
    Returns the field and, per class, how often each value occurs there."""
    inp, pts = edge["inp"], edge["pts"]
    values = []
    for n in THRESHOLDS:
        t = np.float32(getattr(params, n))
        values += [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1e9))]
    values = np.asarray(values, np.float32)
    assert len(set(values.tolist())) == 12
    ice = inp.glacier > 0.5
    mld = np.zeros(ice.shape, bool)
    mld[pts["const_mld"][:, 0], pts["const_mld"][:, 1]] = True
    classes = {"land": (inp.z_topo > 0) & ~ice, "ocean": (inp.z_topo < 0) & ~ice & ~mld, "z_topo == 0": inp.z_topo == 0,
               "glacier on land": (inp.z_topo > 0) & ice, "glacier on ocean": (inp.z_topo < 0) & ice, "constant mixed layer": mld}
    Ts = np.zeros(ice.shape, np.float32)
    seen = np.zeros(ice.shape, bool)
    counts = {}
    for name, mask in classes.items():
        assert not (seen & mask).any()
        seen |= mask
        Ts[mask] = values[np.arange(mask.sum()) % 12]
        counts[name] = np.bincount(np.arange(mask.sum()) % 12, minlength=12)
    assert seen.all()
    return Ts, counts


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_point_physics_at_the_ice_thresholds(eng_mod, edge, params, oracle_lib, strict):
    """The bars of test_point_physics_vs_golden: the eight outputs without a transcendental bit-exact, the other four within
    its ulp counts.  The oracle's routines are the reference's, bit for bit (tests/test_oracle_golden.py)."""
    inp = edge["inp"]
    Ts, counts = threshold_field(edge, params)
    for name, c in counts.items():
        assert c.min() >= 2, (name, c)  # every class holds every value
    o = oracle_lib.Oracle(inp, params)
    cap0, To = o.field(4).copy(), o.field(8).copy()
    e = eng_mod.Engine(inp, params, strict=strict)
    for ityr in (1, 365, 730):
        Ta = (inp.tclim[ityr - 1] + np.float32(0.5)).astype(np.float32)
        q = inp.qclim[ityr - 1]
        out = e.point_physics(ityr, CO2, np.stack([Ts, Ta, To, q, cap0]))
        got = dict(zip(eng_mod.POINT_FIELDS, out))
        ref = {}
        ref["sw"], ref["albedo"] = o.swradiation(ityr, Ts)
        ref["LWsurf"], _, ref["LWair_down"], ref["em"] = o.lwradiation(ityr, Ts, Ta, q, CO2)
        ref["Qlat"], ref["Qlat_air"], ref["dq_eva"], ref["dq_rain"] = o.hydro(ityr, Ts, q)
        ref["dT_ocean"], ref["dTo"] = o.deep_ocean(ityr, Ts, To)
        o.field(4)[:] = cap0
        ref["cap_surf_new"] = o.seaice(ityr, Ts)
        o.field(4)[:] = cap0
        for k in ("albedo", "sw", "LWsurf", "dq_rain", "Qlat_air", "dT_ocean", "dTo", "cap_surf_new"):
            bad = np.argwhere(got[k] != ref[k])
            assert np.array_equal(got[k], ref[k]), (ids(strict), ityr, k, len(bad), bad[:8].tolist(), Ts[tuple(bad[:8].T)].tolist())
        for k, ulps in (("em", 16), ("LWair_down", 32), ("Qlat", 64), ("dq_eva", 64)):
            tol = ulps * np.spacing(np.abs(ref[k]).max())
            d = np.abs(got[k].astype(np.float64) - ref[k]).max()
            print(f"e. {ids(strict)} ityr {ityr} {k:>10s}: max |engine - oracle| {d:.3e} (bar {tol:.3e})")
            assert d <= tol, (ids(strict), ityr, k, d, tol)
        # the field does what it is for: both sides of every threshold give different answers somewhere
        assert len(np.unique(ref["albedo"][inp.z_topo < 0])) > 3 and len(np.unique(ref["cap_surf_new"][inp.z_topo < 0])) > 3
    e.close()
    o.close()


# ------------------------------------------------------------------------------------------------ f. fused against bands
PHYSICS = [{}, {"kappa": 8.8e5, "a_cloud": 0.33}, {"kappa": 6.6e5, "da_ice": 0.27, "a_no_ice": 0.09}]  # kappa within 25 % of 8e5
LEVELS = np.asarray([[340.0], [CO2], [520.0]], np.float32)


def three_members(eng_mod, inp, params, kind, strict, switches=0):
    members = [dict(d, switches=switches) for d in PHYSICS]
    e = eng_mod.Engine(inp, params, strict=strict, members=members, **KINDS[kind][0])
    assert e.describe()["engine"] == KINDS[kind][1], e.describe()
    yf = e.flux_correction(1)
    spun = [e.get_corrections(m) for m in range(3)]
    mon, yr = e.run(1, LEVELS)
    st = np.stack([e.state(m) for m in range(3)])
    for m, (_, s) in enumerate(spun):
        e.set_corrections(None, s, member=m)
    mon_b, bud, yr_b = e.run_budget(1, LEVELS)
    e.close()
    assert np.array_equal(mon_b, mon) and np.array_equal(yr_b, yr) and np.isfinite(bud).all()
    return dict(flux_yearly=yf, corr=np.stack([c for c, _ in spun]), spun_up=np.stack([s for _, s in spun]), monthly=mon, yearly=yr,
                state=st, budget=bud)


@pytest.mark.parametrize("which", ["plain", "edge"])
def test_fused_strict_equals_bands_strict(eng_mod, edge, inputs, params, which):
    """STRICT is the reference's expression trees in both engines, and the fused kernel's STRICT circulation is bit-exact
    against the reference's subroutine (test_strict_stencils_bit_exact_vs_golden): the band sub-step (launch_substep_fused,
    sweep_kernel<., kChainFused>) must give the same bits through its own data movement."""
    inp = inputs if which == "plain" else edge["inp"]
    fused, bands = (three_members(eng_mod, inp, params, kind, True) for kind in ENGINES)
    same(bands, fused, f"bands STRICT against fused STRICT, {which} inputs")
    assert not np.array_equal(fused["monthly"][0], fused["monthly"][1]) and not np.array_equal(fused["monthly"][0], fused["monthly"][2])


@pytest.mark.parametrize("which", ["plain", "edge"])
def test_fused_fast_equals_bands_fast_without_circulation(eng_mod, edge, inputs, params, which):
    """With X_NO_CIRCULATION both engines run the same point physics through different data movement.  Not compared: the
    FAST global mean yearly[..., 0], which the two engines sum in different orders (held by yearly_close)."""
    from greb_climate_model_amd import abi
    inp = inputs if which == "plain" else edge["inp"]
    fused, bands = (three_members(eng_mod, inp, params, kind, False, abi.X_NO_CIRCULATION) for kind in ENGINES)
    assert not fused["budget"][:, :, :, abi.B_DTA_CRCL].any() and not bands["budget"][:, :, :, abi.B_DQ_CRCL].any()
    for d in (fused, bands):
        del d["budget"]
        d["console"] = np.concatenate([d.pop("flux_yearly"), d.pop("yearly")], axis=1)  # [member][year][2]
        d["point_value"] = d["console"][..., 1]
    for m in range(3):
        yearly_close(bands["console"][m], fused["console"][m], False)
    del fused["console"], bands["console"]
    same(bands, fused, f"bands FAST against fused FAST without circulation, {which} inputs")
