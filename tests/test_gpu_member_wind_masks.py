"""GPU: the wind signs the fused 96x48 member kernel keeps as lane masks instead of splitting every staged wind into
max(u,0) and min(u,0) in every sub-step (greb_pair.h: wind_term; greb_member_bulk.h: make_signs).

  * every sign pattern -- positive, negative, +0.0, -0.0 in each of the four positions of a quad, in the first and the
    last quad of a row, in a row of each task family and in rows 1 and 46; all winds zero; all winds of one sign -- through
    the engine module's batched mirror (greb_circulation_batched -> launch_circulation_g96, the member kernel's own
    sub-step loop) against the oracle, with the bars of tests/test_gpu_member_substep_folds.py: STRICT bit-exact, FAST
    within 1e-5 of the largest increment + one ulp of the state per sub-step;
  * the masks follow the winds from model step to model step (they are derived anew in every circulation call): a year
    of the engine against the reference's monthly means -- the winds change sign at many points over a year; a mask of an
    earlier step advects with the wrong neighbours and shows as kelvins -- and the switch-aware instantiation leaves a
    member without switches bit for bit what the default instantiation makes of it."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_member_substep_folds import _params, fast_bound
from test_gpu_members import bit_for_bit
from test_gpu_parity import _check_run

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = (1, 5, 9, 20, 30, 46)  # row 1, a sub-cycled row of a row pair and the single one, a full row of a pair and a single one, row 46
QUADS = (0, 23)
N_PATTERN = 4                 # fields 0-3 carry the patterns; 4: no wind; 5 / 6: every wind positive / negative


def kind_of(a):
    """0 positive, 1 negative, 2 +0.0, 3 -0.0"""
    return np.where(a > 0, 0, np.where(a < 0, 1, np.where(np.signbit(a), 3, 2)))


def _value(kind, mag):
    return (f32(mag), f32(-mag), f32(0.0), -f32(0.0))[kind]


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def fields(inputs, oracle_lib, params):
    o = oracle_lib.Oracle(inputs, params)
    wa, wv = o.field(5).copy(), o.field(6).copy()
    o.close()
    rng = np.random.default_rng(22)
    Ta = (inputs.tclim[99] + (1.5 * rng.standard_normal((48, 96))).astype(f32)).astype(f32)
    q = (inputs.qclim[99] * (f32(0.9) + f32(0.2) * rng.random((48, 96)).astype(f32))).astype(f32)
    u = (inputs.uclim[99] + (2.0 * rng.standard_normal((48, 96))).astype(f32)).astype(f32)
    v = (inputs.vclim[99] + (1.0 * rng.standard_normal((48, 96))).astype(f32)).astype(f32)
    X = np.stack([Ta, q, (Ta - f32(200.0)).astype(f32), q, Ta, q, Ta])
    W = np.stack([wa, wv, wa, wv, wa, wv, wa])
    U = np.stack([u, (-u).astype(f32), u, (-u).astype(f32), np.zeros_like(u), np.abs(u) + f32(0.25), -np.abs(u) - f32(0.25)])
    V = np.stack([v, v, (-v).astype(f32), (-v).astype(f32), np.zeros_like(v), np.abs(v) + f32(0.25), -np.abs(v) - f32(0.25)])
    # the patterns: over the four fields every position of quad 0 and of quad 23 of every covered row sees all four kinds,
    # u and v one kind apart
    for f in range(N_PATTERN):
        for r, k in enumerate(ROWS):
            for g, qd in enumerate(QUADS):
                for p in range(4):
                    kind = (f + g + p + r) % 4
                    U[f, k, 4 * qd + p] = _value(kind, 2.0 + 0.5 * p)
                    V[f, k, 4 * qd + p] = _value((kind + 1) % 4, 1.0 + 0.25 * p)
    return X, W, U, V


def test_patterns_are_present(fields):
    X, W, U, V = fields
    for A in (U, V):
        for k in ROWS:
            for qd in QUADS:
                for p in range(4):  # every kind at every position of each of the two quads
                    seen = {int(kind_of(A[f, k, 4 * qd + p])) for f in range(N_PATTERN)}
                    assert seen == {0, 1, 2, 3}, (k, qd, p, seen)
                for f in range(N_PATTERN):  # and every kind within the quad of one field
                    assert {int(x) for x in kind_of(A[f, k, 4 * qd:4 * qd + 4])} == {0, 1, 2, 3}, (f, k, qd)
        assert (A[4] == 0).all() and not np.signbit(A[4]).any()
        assert (A[5] > 0).all() and (A[6] < 0).all()
    assert 1 <= min(ROWS) and max(ROWS) <= 46 and any(10 <= k <= 37 for k in ROWS) and any(2 <= k <= 9 for k in ROWS)


@pytest.mark.parametrize("nsub", [1, 2, 24])
def test_sign_patterns(eng_mod, oracle_lib, inputs, fields, nsub):
    X, W, U, V = fields
    p = _params(nsub)
    o = oracle_lib.Oracle(inputs, p)
    ref = np.stack([o.circulation(X[i], W[i], u=U[i], v=V[i]) for i in range(len(X))])
    o.close()
    assert np.isfinite(ref).all()
    got = eng_mod.circulation(X, W, U, V, p, strict=True)
    assert np.array_equal(got, ref), float(np.abs(got.astype(np.float64) - ref).max())
    fast = eng_mod.circulation(X, W, U, V, p)
    for i in range(len(X)):
        err, tol = np.abs(fast[i].astype(np.float64) - ref[i]), fast_bound(ref[i], X[i], nsub)
        print(f"nsub {nsub} field {i}: FAST max error {err.max():.3e} (covered rows: {err[ROWS, :].max():.3e}) bound {tol:.3e}")
        assert err.max() <= tol, (nsub, i, float(err.max()), tol)


@pytest.fixture(scope="module")
def default_run(eng_mod, params, inputs):
    """Two FAST members of the default engine, 1 flux-correction year + 1 scenario year, into a NaN-filled buffer; shared
    by the two engine tests below."""
    e = eng_mod.Engine(inputs, params, n_members=2)
    yf = e.flux_correction(1)
    out = np.full((2, 1, 12, 5, 48, 96), np.nan, np.float32)
    mon, yr = e.run(1, 680.0, out=out)
    st = [e.state(m) for m in range(2)]
    e.close()
    return mon, yr, yf, st


def test_masks_follow_the_winds_through_a_year(default_run):
    """The run and the bars of test_gpu_member_substep_folds.test_full_family_tiling_reaches_every_row_quad, repeated here
    as the guard on the masks: they are derived at the top of every circulation call, so a mask of an earlier step cannot
    be used today; if a later change keeps them across calls, this is where it shows."""
    mon, yr, yf, st = default_run
    g = load_golden("run_short_g96.npz")
    assert np.isfinite(mon).all() and all(np.isfinite(s).all() for s in st)
    for m in range(2):
        _check_run(mon[m].reshape(12, 5, 48, 96), g["monthly"][:12], f"member{m}")
    assert np.array_equal(mon[0], mon[1])  # the two members are the same run


def test_switch_aware_launch_rederives_the_masks(eng_mod, params, inputs, default_run):
    mon, yr, yf, st = default_run
    e = eng_mod.Engine(inputs, params, members=[{"switches": 0}, {"switches": 1}])
    d = e.describe()
    assert d["engine"] == "fused member kernel" and d["member_switches"] == "per member", d
    yf2 = e.flux_correction(1)
    mon2, yr2 = e.run(1, 680.0)
    got = (mon2[0], yr2[0], yf2[0], e.state(0))
    e.close()
    want = (mon[0].reshape(mon2[0].shape), yr[0], yf[0], st[0])
    bit_for_bit(got, want, "member without switches beside one with a switch")
