"""GPU: the year walk that the crossing and the regression update kernels share (csrc/greb_yearwalk.h), at the smallest
shapes where it can go wrong.

The grid is 12 x 5: 15 point quads, so the one block of 256 lanes is partly filled and most lanes return before the loads.
Two members, member 0 without a control and member 1 with member 0 as its control; two variables; two years, so that both
the storing first year and an updating year run.  Variable 0 has several selectors -- a month, DJF (which wraps December
to February of the same year) and ANN --, all of them `rel`: member 1 reads its control's months, member 0 gets the quiet
NaN.  Variable 1 has a single item.  The items are given in an order that is not the table's (variable, then selector), so
the products must come back in the caller's order.  The device must equal cross.reference / regress.reference in int32
values, fp32 bits and NaN positions."""
import numpy as np
import pytest
import torch  # before the library is loaded, as the other GPU tests import it

from greb_climate_model_amd import abi, cross, diag, regress

pytestmark = pytest.mark.gpu

NX, NY, N, NV, YEARS = 12, 5, 2, 2, 2
CONTROL = [-1, 0]


@pytest.fixture(scope="module")
def years():
    rng = np.random.default_rng(125)
    x = (rng.random((YEARS, N, 12, NV, NY, NX), dtype=np.float32) * np.float32(10) + np.float32(270)).astype(np.float32)
    x.setflags(write=False)
    return x


def _same_bits(got, ref, label):
    g, r = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert g.dtype == r.dtype and g.shape == r.shape, (label, g.dtype, r.dtype, g.shape, r.shape)
    if g.dtype == np.float32:
        gn, rn = np.isnan(g), np.isnan(r)
        bad = (gn != rn) | (~gn & ~rn & (g.view(np.uint32) != r.view(np.uint32)))
    else:
        bad = g != r
    print(f"{label}: {int(bad.sum())} of {bad.size} values differ")
    assert not bad.any(), (label, int(bad.sum()), g[bad][:4], r[bad][:4])


def test_cross_walk_on_a_partly_filled_block(years):
    E = cross.Event
    events = [E(1, cross.JUL, 275.0), E(0, cross.ANN, 0.0, rel=True), E(0, cross.MAR, 0.5, dir=-1, rel=True),
              E(0, cross.DJF, -0.25, rel=True), E(0, cross.ANN, 275.0)]
    ref = cross.reference(years, events, CONTROL, [0, 0])
    # member 0 has no control: its `rel` events never hit and their peak is NaN; member 1's hit somewhere and miss somewhere
    assert all(np.isnan(ref.peak[0, e]).all() and (ref.count[0, e] == 0).all() for e in (1, 2, 3))
    assert all(np.isfinite(ref.peak[1, e]).all() and 0 < ref.count[1, e].mean() < YEARS for e in (1, 2, 3))
    assert np.isfinite(ref.peak[:, [0, 4]]).all()
    plan = cross.Plan(NX, NY, N, events, n_vars=NV, control=CONTROL, group=[0, 0])
    assert plan.what == cross.ALL
    frac = [cross.add_year_dev(plan, torch.tensor(xk).cuda(), k) for k, xk in enumerate(years)]
    res = cross.finish_dev(plan, YEARS)
    torch.cuda.synchronize()
    for name in ("first", "last", "stay", "count", "peak", "peak_year"):
        _same_bits(getattr(res, name).cpu().numpy(), getattr(ref, name), "cross " + name)
    _same_bits(np.stack([f.cpu().numpy() for f in frac]), ref.fraction, "cross fraction")
    plan.close()


def test_reg_walk_on_a_partly_filled_block(years):
    I, T = regress.Index, regress.Term
    indices = [I(0, cross.ANN), I(1, cross.JUL, rel=True)]
    terms = [T(1, cross.JUN, 0), T(0, cross.ANN, 1, rel=True), T(0, cross.FEB, 0, rel=True), T(0, cross.DJF, 0, rel=True), T(0, cross.ANN, 0)]
    dplan = diag.Plan(NX, NY, None, n_vars=NV)
    means = [diag.reduce_dev(dplan, torch.tensor(xk).cuda(), abi.D_REGIONS).regions for xk in years]
    torch.cuda.synchronize()
    means = np.stack([m.cpu().numpy() for m in means])  # the regional means as the device makes them
    dplan.close()
    ref = regress.reference(years, indices, terms, CONTROL, regions=means)
    # member 0: NaN in every `rel` term and in the `rel` index; member 1 and the plain terms: numbers
    assert np.isnan(ref.slope[0, 1:4]).all() and np.isnan(ref.index[0, :, 1]).all()
    assert np.isfinite(ref.slope[1, [0, 2, 3, 4]]).all() and np.isfinite(ref.slope[0, [0, 4]]).all() and np.isfinite(ref.index[1]).all()
    plan = regress.Plan(NX, NY, N, indices, terms, n_vars=NV, control=CONTROL)
    index = [regress.add_year_dev(plan, torch.tensor(xk).cuda(), k) for k, xk in enumerate(years)]
    res = regress.finish_dev(plan, YEARS)
    torch.cuda.synchronize()
    for name in ("slope", "intercept", "r2"):
        _same_bits(getattr(res, name).cpu().numpy(), getattr(ref, name), "reg " + name)
    _same_bits(np.stack([i.cpu().numpy() for i in index], axis=1), ref.index, "reg index")
    plan.close()
