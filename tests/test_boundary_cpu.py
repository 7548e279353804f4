"""CPU: the host side of boundary sets (greb_engine_add_boundary_set, greb_engine_set_member_boundary) -- the exported
symbols, what an upstream experiment changes in the boundary data (original.experiment_overrides against
original.experiment_inputs and greb.original.model.f90:162-166), and the Python-side argument checks."""
import numpy as np
import pytest

from greb_climate_model_amd import abi, build, engine, original

FIELDS = ("z_topo", "glacier", "sw_solar", "tclim", "qclim", "uclim", "vclim", "mldclim", "cldclim", "swetclim")  # greb_fields


def test_new_symbols_are_exported():
    import ctypes as C
    L = C.CDLL(build.build_lib())
    for name in ("greb_engine_add_boundary_set", "greb_engine_set_member_boundary"):
        assert name in engine.EXPORTS and hasattr(L, name), name
    assert abi.MAX_BOUNDARY_SETS == 16 and abi.BS_REINIT == 1
    assert set(abi.BOUNDARY_FIELDS) == set(FIELDS) - {"sw_solar"}


def expected_fields(le):
    """greb.original.model.f90:162-166"""
    want = set()
    if le == 1:
        want.add("z_topo")
    if le <= 2:
        want.add("cldclim")
    if le <= 3:
        want.add("qclim")
    if le <= 9 or le == 11:
        want.add("mldclim")
    return want


@pytest.mark.parametrize("le", range(1, 17))
def test_overrides_applied_to_the_inputs_are_experiment_inputs(inputs, le):
    ov = original.experiment_overrides(inputs, le)
    assert set(ov) == expected_fields(le), (le, sorted(ov))
    mod = original.experiment_inputs(inputs, le)
    for name in FIELDS:
        want = ov.get(name, getattr(inputs, name))
        got = getattr(mod, name)
        assert got.dtype == np.float32 and np.array_equal(got, want), (le, name)
        if name not in ov:
            assert got is getattr(inputs, name), (le, name)  # untouched fields are shared, not copied
        else:
            assert got.shape == getattr(inputs, name).shape and not np.array_equal(got, getattr(inputs, name)), (le, name)


def test_override_values_and_d_ocean(inputs):
    ov = original.experiment_overrides(inputs, 1, d_ocean=30.0)
    assert (ov["mldclim"] == np.float32(30.0)).all() and (ov["cldclim"] == np.float32(0.7)).all()
    assert (ov["qclim"] == np.float32(0.0052)).all()
    z = inputs.z_topo
    assert np.array_equal(ov["z_topo"][z <= 1.0], z[z <= 1.0]) and (ov["z_topo"][z > 1.0] == 1.0).all()
    assert original.experiment_overrides(inputs, 10) == {} and original.experiment_overrides(inputs, 16) == {}


def test_python_side_checks_of_a_boundary_set(inputs):
    nx, ny = inputs.nx, inputs.ny
    ok = engine.boundary_fields(nx, ny, dict(cldclim=inputs.cldclim.astype(np.float64), glacier=inputs.glacier, tclim=None))
    assert sorted(ok) == ["cldclim", "glacier"]
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in ok.values())
    assert np.array_equal(ok["cldclim"], inputs.cldclim)
    bad = [
        (dict(), "no field"),
        (dict(tclim=None), "no field"),
        (dict(sw_solar=inputs.sw_solar), "set_forcing_tables"),
        (dict(clouds=inputs.cldclim), "unknown field 'clouds'"),
        (dict(cldclim=inputs.cldclim[0]), "cldclim has shape"),
        (dict(z_topo=inputs.tclim), "z_topo has shape"),
        (dict(glacier=inputs.glacier.T), "glacier has shape"),
        (dict(qclim=inputs.qclim[:, :, :-4]), "qclim has shape"),
        (dict(glacier=inputs.glacier.astype(np.complex64)), "glacier has dtype complex64"),
        (dict(glacier=inputs.glacier > 0), "glacier has dtype bool"),
        (dict(z_topo=np.full((ny, nx), "0")), "z_topo has dtype"),
    ]
    for fields, text in bad:
        with pytest.raises(engine.GrebError) as ei:
            engine.boundary_fields(nx, ny, fields)
        assert ei.value.code == -1 and text in str(ei.value), (text, str(ei.value))
