"""GPU: which lane computes which row-quad in the fused 96x48 member kernel (greb_member_deal.h: task_rowquad deals the tasks
to the LDS's lane groups) must not show in the results.  The kernel's own sub-step loop through its batched mirror
(greb_circulation_batched -> launch_circulation_g96) against the oracle's `circulation`, batch 2, for 1, 3 (an odd count:
the result ends in the other buffer) and 24 sub-steps (the full call): STRICT bit-exact, FAST within the bound of
tests/test_gpu_member_substep_folds.py.

The winds are unique per (row, quad) and change sign inside every quad, and the tracer differs between quads 0 and 23 of
every row: a task that reads another row's or quad's winds, takes the wrong neighbour across the seam between quads 23 and
0, or uses another task's sign masks computes something else."""
import numpy as np
import pytest

from test_gpu_member_substep_folds import _params, fast_bound

pytestmark = pytest.mark.gpu

f32 = np.float32
NSUB = (1, 3, 24)


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
    rng = np.random.default_rng(8)
    k, x = np.meshgrid(np.arange(48), np.arange(96), indexing="ij")
    quad, pos = x // 4, x % 4
    Ta = (inputs.tclim[40] + (1.5 * rng.standard_normal((48, 96))).astype(f32) + (0.125 * quad).astype(f32)).astype(f32)
    q = (inputs.qclim[40] * (f32(0.8) + f32(0.4) * rng.random((48, 96)).astype(f32)) * (f32(1.0) + f32(0.01) * quad.astype(f32))).astype(f32)
    # |u|, |v|: one level per (row, quad), a small step per position; the sign alternates inside the quad and the
    # alternation starts differently from quad to quad and from row to row (u) or the other way round (v)
    level = (1.0 + (k * 24 + quad) / 256.0)
    sign_u = np.where((pos + quad + k) % 2 == 0, 1.0, -1.0)
    sign_v = np.where((pos // 2 + quad + 2 * k) % 2 == 0, 1.0, -1.0)
    u = (sign_u * (level + 0.001 * pos)).astype(f32)
    v = (sign_v * (0.5 * level + 0.002 * pos)).astype(f32)
    X = np.stack([Ta, q])
    W = np.stack([wa, wv])
    U = np.stack([u, (-u[:, ::-1]).astype(f32)])
    V = np.stack([v, (-v[::-1]).astype(f32)])
    return X, W, U, V


@pytest.fixture(scope="module")
def reference(oracle_lib, inputs, fields):
    """the oracle's circulation of the two fields for each sub-step count, computed once"""
    X, W, U, V = fields
    out = {}
    for nsub in NSUB:
        o = oracle_lib.Oracle(inputs, _params(nsub))
        out[nsub] = np.stack([o.circulation(X[i], W[i], u=U[i], v=V[i]) for i in range(len(X))])
        o.close()
        assert np.isfinite(out[nsub]).all()
    return out


def test_fields_tell_rows_and_quads_apart(fields):
    X, W, U, V = fields
    for A in (U, V):
        for i in range(2):
            quads = np.abs(A[i]).reshape(48, 24, 4)
            key = np.round(quads[:, :, 0].astype(np.float64) * (1 if A is U else 2) * 256).astype(int)
            assert len(np.unique(key)) == 48 * 24                                  # one level per (row, quad)
            s = np.sign(A[i]).reshape(48, 24, 4)
            assert ((s.min(axis=2) < 0) & (s.max(axis=2) > 0)).all()               # both signs inside every quad
    for i in range(2):
        assert (X[i][:, 0:4] != X[i][:, 92:96]).all()                              # quads 0 and 23 of every row differ


@pytest.mark.parametrize("nsub", NSUB)
def test_strict_is_the_oracle_bit_for_bit(eng_mod, fields, reference, nsub):
    X, W, U, V = fields
    got = eng_mod.circulation(X, W, U, V, _params(nsub), strict=True)
    ref = reference[nsub]
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (len(bad), bad[:6].tolist(), float(np.abs(got.astype(np.float64) - ref).max()))


@pytest.mark.parametrize("nsub", NSUB)
def test_fast_is_within_the_routine_bound(eng_mod, fields, reference, nsub):
    X, W, U, V = fields
    fast = eng_mod.circulation(X, W, U, V, _params(nsub))
    for i in range(len(X)):
        err, tol = np.abs(fast[i].astype(np.float64) - reference[nsub][i]), fast_bound(reference[nsub][i], X[i], nsub)
        print(f"nsub {nsub} field {i}: FAST max error {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}, bound {tol:.3e}")
        assert err.max() <= tol, (nsub, i, float(err.max()), tol)
