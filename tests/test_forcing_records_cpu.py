"""CPU: the layout of the packed forcing record the FAST fused 96x48 member kernel reads its boundary data from
(greb_kernels.h: forcing_record_offset, through the exported layout queries): a static part
[row][field][96] and, behind it, 730 step slices [row][field][96].  No GPU call is made."""
import numpy as np
import pytest

from greb_climate_model_amd import abi, build, engine

NX, NY = 96, 48
STATIC = ("z_topo", "glacier", "z_ocean", "wz_air")
STEP = ("tclim", "cldclim", "mldclim", "mldclim_prev", "swetclim", "wind_speed")


@pytest.fixture(scope="module")
def layout():
    build.build_lib()
    return engine.forcing_record_layout(NX, NY)


def parts(layout):
    """(name of the part, indices of its fields, its size in floats)"""
    st = [f for f, s in enumerate(layout.static) if s]
    return (("static", st, layout.static_floats),
            ("step", [f for f in range(len(layout.names)) if f not in st], layout.step_floats))


def test_fields(layout):
    """Everything the default scenario and flux-correction quads read from boundary data; uclim and vclim only as the
    finished wind-speed term.  The static fields come first."""
    assert layout.names == STATIC + STEP
    assert layout.static == (True,) * len(STATIC) + (False,) * len(STEP)
    L = engine.lib()
    for f in (-1, len(layout.names)):
        assert L.greb_forcing_record_field_name(f) is None and L.greb_forcing_record_field_static(f) == -1


def test_offsets_are_distinct_and_cover_each_part_exactly(layout):
    assert layout.offsets.shape == (NY, len(layout.names), NX)
    for name, fields, floats in parts(layout):
        flat = np.sort(layout.offsets[:, fields, :].reshape(-1))
        assert np.array_equal(flat, np.arange(floats)), f"{name}: every float is exactly one (row, field, longitude)"
        assert floats == NY * len(fields) * NX


def test_quads_are_16_byte_aligned_and_contiguous(layout):
    """A quad (4 consecutive longitudes) of a field is one 16-byte load; the 24 quads of a row are 384 contiguous bytes.
    Both parts start 16-byte aligned inside the record."""
    off = layout.offsets
    assert (off[:, :, 0::4] * 4 % 16 == 0).all()
    assert (np.diff(off, axis=2) == 1).all()
    assert layout.static_floats * 4 % 16 == 0 and layout.step_floats * 4 % 16 == 0


def test_field_offsets_fit_the_instruction_immediate(layout):
    """A quad's fields sit at base + lane offset + field offset; the field offset is an instruction immediate."""
    off = layout.offsets
    for name, fields, _ in parts(layout):
        for j, f in enumerate(fields):
            b = layout.field_bytes[f]
            assert 0 <= b <= 4095 and b == j * NX * 4, (layout.names[f], b)
            assert ((off[:, f, :] - off[:, fields[0], :]) * 4 == b).all(), layout.names[f]
    assert engine.lib().greb_forcing_record_field_bytes(len(layout.names)) == -1


def test_record_size_is_the_static_part_and_730_steps(layout):
    assert layout.record_bytes == (layout.static_floats + layout.step_floats * abi.NSTEP_YR) * 4
    assert layout.record_bytes < 2 ** 31  # the kernel's offsets into a record are 32-bit


def test_outside_the_record_is_minus_one(layout):
    f = engine.lib().greb_forcing_record_offset
    for row, field, lon in ((-1, 0, 0), (NY, 0, 0), (0, -1, 0), (0, len(layout.names), 0), (0, 0, -1), (0, 0, NX)):
        assert f(row, field, lon) == -1, (row, field, lon)
