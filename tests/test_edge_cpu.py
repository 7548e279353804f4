"""CPU: the edge year (tests/edge_workload.py) -- inputs and corrections edited so that a model year takes the branches of
the step the plain workload never reaches -- checked as a yardstick before the GPU tests (tests/test_gpu_edge.py) use it.

1. The construction is the one tests/golden/edge_g96.npz was minted on, and the oracle reproduces the reference's output on
   it bit for bit (tests/golden/make_golden_edge.py asserted that when it ran the reference).
2. The mirror year with the edited corrections equals Oracle.run with the same corrections, bit for bit.
3. The census of that year: every branch is taken, the clamp fires where and when it is meant to, nothing is near its tie.
4. The edits matter: every class of edited points moves the monthly Tsurf.
One oracle year of each kind is computed once per module and shared."""
import hashlib
import json
import os

import numpy as np
import pytest

import budget_mirror
import edge_workload
from conftest import GOLDEN, load_golden, rms

CO2 = 680.0
NEVER_TAKEN = ("humidity clamp of the update", "z_topo == 0, land albedo: cold", "z_topo == 0, land albedo: warm",
               "z_topo == 0, land albedo: ramp", "glacier on ocean, albedo overridden: cold",
               "glacier on ocean, albedo overridden: warm", "glacier on ocean, albedo overridden: ramp",
               "glacier on ocean, sea ice overridden: cold", "glacier on ocean, sea ice overridden: warm",
               "glacier on ocean, sea ice overridden: ramp", "deep ocean: warm, dmld == 0")
ALREADY_TAKEN = ("land albedo: cold", "land albedo: warm", "land albedo: ramp", "ocean albedo: cold", "ocean albedo: warm",
                 "ocean albedo: ramp", "sea ice: cold", "sea ice: warm", "sea ice: ramp", "glacier on land",
                 "deep ocean: dmld < 0", "deep ocean: dmld > 0", "deep ocean: ocean below To_ice2")


@pytest.fixture(scope="module")
def edge(oracle_lib, inputs, params):
    """Computed once, shared, never changed: the plain year of the oracle; on the edge inputs its flux-correction year and
    scenario year; from the same spun-up state and the EDITED corrections the mirror's year with its census, and Oracle.run."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    plain, _ = o.run(1, CO2)
    o.close()
    inp, pts = edge_workload.make_edge_inputs(inputs, params)
    o = oracle_lib.Oracle(inp, params)
    yf = o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    mon, yr = o.run(1, CO2)
    start.restore(o)
    for i in range(4):
        o.field(i)[:] = start.state5[i]
    corr0 = start.corr
    start.corr = edge_workload.edit_corrections(corr0)
    census = edge_workload.Census(inp, params)
    mirror = budget_mirror.run_year(o, start, CO2, observer=census)
    start.restore(o)
    for i in range(3):
        o.field(10 + i, budget_mirror.NT)[:] = start.corr[i]
    clamp_run, _ = o.run(1, CO2)
    clamp_state = o.state5()
    o.close()
    return dict(inp=inp, pts=pts, plain=plain[0], monthly=mon[0], yearly=np.concatenate([yf, yr]), start=start, corr0=corr0, census=census,
                mirror=mirror, clamp_run=clamp_run[0], clamp_state=clamp_state)


def test_construction_is_the_fixtures_and_the_oracle_is_the_reference_on_it(edge, inputs):
    g = load_golden("edge_g96.npz")
    for name in edge_workload.CLASSES:
        assert np.array_equal(g[name], edge["pts"][name]), name
    assert [len(edge["pts"][n]) for n in edge_workload.CLASSES] == [24, 24, 40, 40]
    flat = np.concatenate([edge["pts"][n] @ np.array([inputs.nx, 1]) for n in edge_workload.CLASSES])
    assert len(set(flat.tolist())) == len(flat)  # the classes are disjoint
    inp = edge["inp"]
    z0 = np.concatenate([edge["pts"]["zero_land"], edge["pts"]["zero_ocean"]])
    assert np.count_nonzero(inp.z_topo == 0) == 48 and not inp.z_topo[z0[:, 0], z0[:, 1]].any()
    assert (inputs.z_topo[edge["pts"]["zero_land"][:, 0], edge["pts"]["zero_land"][:, 1]] > 0).all()
    for n in ("zero_ocean", "glacier_ocean", "const_mld"):
        assert (inputs.z_topo[edge["pts"][n][:, 0], edge["pts"][n][:, 1]] < 0).all(), n
    assert np.count_nonzero((inp.glacier > 0.5) & (inp.z_topo < 0)) == 40
    k, l = edge["pts"]["const_mld"].T
    assert (np.ptp(inp.mldclim[:, k, l], axis=0) == 0).all() and (np.ptp(inputs.mldclim[:, k, l], axis=0) > 0).all()
    assert np.count_nonzero(np.ptp(inp.mldclim, axis=0) == 0) == np.count_nonzero(np.ptp(inputs.mldclim, axis=0) == 0) + 40
    # the reference's own output on these inputs (oracle/_ref/greb_ref, 1 + 1 yr at 680 ppm)
    assert np.array_equal(edge["monthly"], g["monthly"])
    assert np.array_equal(edge["yearly"], g["yearly"])
    assert np.isfinite(g["monthly"]).all()
    item = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))["items"]["edge_g96"]
    assert item["oracle_bit_identical"] is True and item["time_flux"] == item["time_scnr"] == 1 and item["co2_ppm"] == CO2
    assert item["sha256"] == hashlib.sha256(np.ascontiguousarray(g["monthly"]).tobytes()).hexdigest()


def test_corrections_edit_is_the_patch_at_the_four_steps(edge):
    corr = edge["start"].corr
    m = edge_workload.clamp_patch()
    assert m.sum() == 86 and m[20:24, 40:52].all() and m[0, ::5].all() and m[47, 3::7].all() and m[5, 92:].all()
    assert m[20:24].sum() == 48 and m[0].sum() == 20 and m[47].sum() == 14 and m[5].sum() == 4
    hit = corr[1] == -1
    assert sorted(set(np.nonzero(hit)[0].tolist())) == list(edge_workload.CLAMP_STEPS) == [9, 10, 364, 729]
    for s in edge_workload.CLAMP_STEPS:
        assert np.array_equal(hit[s], m)
    # everything else is the flux-correction year's
    assert np.array_equal(corr[1][~hit], edge["corr0"][1][~hit]) and np.array_equal(corr[[0, 2]], edge["corr0"][[0, 2]])
    assert not (edge["corr0"][1] == -1).any()


def test_mirror_clamp_year_equals_oracle_run(edge):
    """test_budget_cpu's property on the year in which the clamp fires."""
    monthly, budget, state = edge["mirror"]
    assert np.array_equal(monthly, edge["clamp_run"]), float(np.abs(monthly.astype(np.float64) - edge["clamp_run"]).max())
    assert np.array_equal(state, edge["clamp_state"])
    assert np.isfinite(monthly).all() and np.isfinite(budget).all() and np.isfinite(state).all()
    assert not np.array_equal(monthly, edge["monthly"])  # the clamp year is another year
    print(f"clamp year against the edge year without the edit: monthly Tsurf moves by up to {np.abs(monthly[:, 0] - edge['monthly'][:, 0]).max():.3f} K")


def test_observer_changes_nothing(edge, oracle_lib, params):
    """run_year with an observer returns what run_year without one returns."""
    o = oracle_lib.Oracle(edge["inp"], params)
    got = budget_mirror.run_year(o, edge["start"], CO2)
    o.close()
    for a, b in zip(got, edge["mirror"]):
        assert np.array_equal(a, b)


def test_census_every_branch_is_taken(edge):
    c, pts = edge["census"], edge["pts"]
    print("\n".join(c.lines()))
    for name in NEVER_TAKEN + ALREADY_TAKEN:
        assert c.counts[name] > 0, name
    # the clamp: at each of the four steps at every patched point, and at no other step or point
    m = edge_workload.clamp_patch()
    assert np.flatnonzero(c.fired).tolist() == list(edge_workload.CLAMP_STEPS)
    for s in edge_workload.CLAMP_STEPS:
        assert np.array_equal(c.fired_at[s], m), s
    assert c.counts["humidity clamp of the update"] == 4 * 86
    # no arithmetic mode can decide otherwise: no point-step within 1 % of the tie, no denormal humidity
    assert c.min_margin > 0.01, c.min_margin
    assert c.q_min > 1e-6, c.q_min
    # every edited point is counted in its branch
    for cls, names in (("zero", ("zero_land", "zero_ocean")), ("glacier_ocean", ("glacier_ocean",)), ("const_mld", ("const_mld",))):
        for n in names:
            assert (c.per_point[cls][pts[n][:, 0], pts[n][:, 1]] > 0).all(), (cls, n)
        mask = np.zeros_like(c.per_point[cls], bool)
        for n in names:
            mask[pts[n][:, 0], pts[n][:, 1]] = True
        assert not c.per_point[cls][~mask].any(), cls  # ... and these branches are the edited points' alone


def test_the_edits_matter(edge):
    """Against the oracle on the plain workload every class of edited points moves the monthly Tsurf: a point counts when
    some month moves by at least 0.01 K -- a branch missed at that point alone is then an RMS over the grid of
    0.01 / sqrt(4608) = 1.5e-4 K, above the 1e-4 K tolerance of the whole-run comparison -- and at most a quarter of a
    class may fall below."""
    d = np.abs(edge["monthly"][:, 0].astype(np.float64) - edge["plain"][:, 0]).max(axis=0)
    for n in edge_workload.CLASSES:
        x = d[edge["pts"][n][:, 0], edge["pts"][n][:, 1]]
        print(f"edit {n:>14s}: monthly Tsurf moves by median {np.median(x):.3f} K, least {x.min():.3f} K, {np.count_nonzero(x < 0.01)} of {len(x)} points below 0.01 K")
        assert np.count_nonzero(x < 0.01) <= len(x) // 4, (n, np.sort(x)[:12])
    assert rms(edge["monthly"][:, 0], edge["plain"][:, 0]) > 1e-2
