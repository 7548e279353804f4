"""The edge year: the synthetic workload edited so that a model year takes the branches of the point physics that the plain
workload never reaches.  TEST INFRASTRUCTURE, NOT PRODUCT.

A plain year (flux-correction year, then a scenario year at 680 ppm) never fires the specific-humidity clamp of the update
(src/greb.f90:265), has no point with z_topo == 0, no glacier on an ocean point and no warm ocean point whose mixed layer
stands still.  make_edge_inputs() edits the boundary fields, edit_corrections() the humidity flux correction; Census counts
the branches from a mirror year (budget_mirror.run_year(..., observer=Census(...))).

The construction is deterministic: the point lists come from the input fields and one seeded generator, and are stored in
tests/golden/edge_g96.npz, where tests/test_edge_cpu.py compares them with what this module makes."""
import dataclasses

import numpy as np

from greb_climate_model_amd import abi, workload

f32 = np.float32
NT = abi.NSTEP_YR
SEED = 20251
N_ZERO, N_GLACIER, N_MLD = 24, 40, 40
CLAMP_STEPS = (9, 10, 364, 729)  # 0-based: two consecutive steps, a step in mid-year, the last step of December and the year
CLASSES = ("zero_land", "zero_ocean", "glacier_ocean", "const_mld")


def edge_points(inp=None, params=None):
    """The four point lists, each int32 [n][2] of (row, longitude), sorted.  The three ocean classes are disjoint.
    const_mld: the 40 ocean points with the largest annual range of mldclim among those whose climatological Tsurf is at or
    above To_ice2 for at least a quarter of the year (deep_ocean's entrainment acts on a warm ocean only; random points move
    the climate too little).  glacier_ocean: ocean points whose climatological Tsurf is cold (<= To_ice1) at some time, in
    the ramp at some time, warm (>= To_ice2) all year -- a third each.  zero_*: random."""
    inp = workload.make_inputs() if inp is None else inp
    p = abi.default_params() if params is None else params
    rng = np.random.default_rng(SEED)
    land, ocean, ice = inp.z_topo > 0, inp.z_topo < 0, inp.glacier > 0.5
    assert not (inp.z_topo == 0).any() and not (ocean & ice).any()  # what the plain workload lacks
    t = inp.tclim
    warm_steps = (t >= f32(p.To_ice2)).sum(axis=0)

    def pick(mask, n):
        idx = np.flatnonzero(mask.ravel())
        return np.sort(rng.choice(idx, n, replace=False))

    free = ocean.copy()
    cand = np.flatnonzero((free & (warm_steps >= NT // 4)).ravel())
    span = np.ptp(inp.mldclim, axis=0).ravel()[cand]
    const_mld = np.sort(cand[np.argsort(-span, kind="stable")[:N_MLD]])
    free.ravel()[const_mld] = False
    tmin = t.min(axis=0)
    cold = free & (tmin <= f32(p.To_ice1))
    ramp = free & ~cold & (tmin < f32(p.To_ice2))
    warm = free & (tmin >= f32(p.To_ice2))
    n3 = N_GLACIER // 3
    glacier_ocean = np.sort(np.concatenate([pick(cold, n3), pick(ramp, n3), pick(warm, N_GLACIER - 2 * n3)]))
    free.ravel()[glacier_ocean] = False
    zero_ocean = pick(free, N_ZERO)
    zero_land = pick(land & ~ice, N_ZERO)
    rc = lambda flat: np.stack(np.unravel_index(flat, inp.z_topo.shape), axis=1).astype(np.int32)
    return dict(zero_land=rc(zero_land), zero_ocean=rc(zero_ocean), glacier_ocean=rc(glacier_ocean), const_mld=rc(const_mld))


def make_edge_inputs(inp=None, params=None):
    """workload.make_inputs() with z_topo = 0 at 24 land and 24 ocean points, glacier = 1 at 40 ocean points, and the
    mixed-layer depth of step 0 held all year at 40 ocean points.  Returns (inputs, point lists)."""
    inp = workload.make_inputs() if inp is None else inp
    pts = edge_points(inp, params)
    z, g, mld = inp.z_topo.copy(), inp.glacier.copy(), inp.mldclim.copy()
    for name in ("zero_land", "zero_ocean"):
        z[pts[name][:, 0], pts[name][:, 1]] = f32(0)
    g[pts["glacier_ocean"][:, 0], pts["glacier_ocean"][:, 1]] = f32(1)
    k, l = pts["const_mld"][:, 0], pts["const_mld"][:, 1]
    mld[:, k, l] = mld[0, k, l]
    return dataclasses.replace(inp, z_topo=z, glacier=g, mldclim=mld), pts


def clamp_patch(ny=48, nx=96):
    """Where edit_corrections sets qF = -1: three whole quads in each of four mid-latitude rows, the two polar chain rows
    at strides that are no multiple of a quad, and the last quad of a sub-cycled row (the zonal wrap)."""
    m = np.zeros((ny, nx), bool)
    m[20:24, 40:52] = True
    m[0, ::5] = True
    m[47, 3::7] = True
    m[5, 92:96] = True
    return m


def edit_corrections(corr):
    """A copy of corr [3][730][ny][nx] (TF, qF, ToF) with qF = -1 kg/kg on clamp_patch() at CLAMP_STEPS: dq <= -q there
    whatever the other terms are, so the update takes dq = -0.9 q (src/greb.f90:265)."""
    corr = np.array(corr, np.float32, copy=True)
    m = clamp_patch(*corr.shape[2:])
    for s in CLAMP_STEPS:
        corr[1, s][m] = f32(-1)
    return corr


class Census:
    """Observer of budget_mirror.run_year: counts the point-steps that take each branch of the step.
    counts: dict name -> int; per_point: dict class -> int [ny][nx] point-steps in that class's own branch;
    fired: int [730] points the humidity clamp fired at per step, fired_at: bool [730][ny][nx];
    min_margin: the smallest |dq + q| / q seen (the distance of any point-step from the clamp's tie)."""

    def __init__(self, inp, params):
        self.inp, self.p = inp, params
        ny, nx = inp.z_topo.shape
        self.counts = {}
        self.per_point = {c: np.zeros((ny, nx), np.int64) for c in ("zero", "glacier_ocean", "const_mld")}
        self.fired = np.zeros(NT, np.int64)
        self.fired_at = np.zeros((NT, ny, nx), bool)
        self.min_margin = np.inf
        self.q_min = np.inf

    def _add(self, name, mask):
        self.counts[name] = self.counts.get(name, 0) + int(np.count_nonzero(mask))

    def _three(self, name, where, T, t1, t2):
        self._add(name + ": cold", where & (T <= t1))
        self._add(name + ": warm", where & (T >= t2))
        self._add(name + ": ramp", where & (T > t1) & (T < t2))

    def __call__(self, ityr, Ts, To, q, dq, Ts0):
        inp, p = self.inp, self.p
        z, ice = inp.z_topo, inp.glacier > 0.5
        tl1, tl2, to1, to2 = (f32(getattr(p, n)) for n in ("Tl_ice1", "Tl_ice2", "To_ice1", "To_ice2"))
        sw_land, ocean, zero = z >= 0, z < 0, z == 0
        self._three("land albedo", sw_land & ~ice, Ts, tl1, tl2)
        self._three("ocean albedo", ocean & ~ice, Ts, to1, to2)
        self._three("sea ice", ocean & ~ice, Ts0, to1, to2)
        self._add("glacier on land", (z > 0) & ice)
        self._three("z_topo == 0, land albedo", zero, Ts, tl1, tl2)
        self._three("glacier on ocean, albedo overridden", ocean & ice, Ts, to1, to2)
        self._three("glacier on ocean, sea ice overridden", ocean & ice, Ts0, to1, to2)
        mld = inp.mldclim[ityr - 1]
        dmld = mld - inp.mldclim[ityr - 2 if ityr > 1 else NT - 1]
        warm = ocean & (Ts >= to2)
        self._add("deep ocean: dmld < 0", warm & (dmld < 0))
        self._add("deep ocean: dmld > 0", warm & (dmld > 0))
        self._add("deep ocean: warm, dmld == 0", warm & (dmld == 0))
        self._add("deep ocean: ocean below To_ice2", ocean & (Ts < to2))
        self._add("Tsurf equal to an ice threshold", (Ts == tl1) | (Ts == tl2) | (Ts == to1) | (Ts == to2))
        self.per_point["zero"] += zero
        self.per_point["glacier_ocean"] += ocean & ice
        self.per_point["const_mld"] += warm & (dmld == 0)
        fire = dq <= -q
        self._add("humidity clamp of the update", fire)
        self.fired[ityr - 1] = np.count_nonzero(fire)
        self.fired_at[ityr - 1] = fire
        self.min_margin = min(self.min_margin, float((np.abs(dq.astype(np.float64) + q) / q).min()))
        self.q_min = min(self.q_min, float(q.min()))

    def lines(self):
        out = [f"census {name:<44s} {n:>9d} point-steps" for name, n in self.counts.items()]
        out.append(f"census clamp fired at steps {np.flatnonzero(self.fired).tolist()} (0-based), points per step {sorted(set(self.fired[self.fired > 0].tolist()))}")
        out.append(f"census smallest |dq + q| / q {self.min_margin:.4f}; smallest q {self.q_min:.3e}")
        return out
