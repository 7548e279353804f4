"""CPU: stochastic surface heat-flux forcing (include/greb_engine.h: greb_engine_set_noise_tables, greb_engine_set_member_noise,
greb_engine_get_noise).

greb_climate_model_amd/noise.py -- the numpy statement of the device generator -- against the published Philox4x32-10 known
answers, the first deviates, the statistics of 1.8 million deviates at four standard errors, and the cell and hold rules;
tests/noise_mirror.py, the yardstick of the GPU tests, held to the unhooked mirror year at amp = 0.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import budget_mirror
import noise_mirror
import sst_mirror
from greb_climate_model_amd import abi, build, noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CO2 = 680.0
KEY = (12345, 678)


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_lib())


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = noise.philox4x32(counter, key)
    assert all(w.dtype == np.uint32 for w in got)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_philox_broadcasts_over_arrays():
    c = np.arange(7, dtype=np.uint32)
    got = noise.philox4x32((c, 5, 0, 0), KEY)
    for i in range(7):
        one = noise.philox4x32((i, 5, 0, 0), KEY)
        assert [int(w[i]) for w in got] == [int(w) for w in one]


def test_first_deviates():
    """Key (12345, 678), step 0, cells 0 ... 3 at cell (1, 1), hold 1: the fp32 bits of z."""
    z = noise.deviates(KEY, 4, 1, (1, 1), 1, (0,))
    assert z.dtype == f32 and z.shape == (1, 1, 4)
    assert z.view(np.uint32).ravel().tolist() == [1069776130, 1055522110, 3220200440, 3190176006]
    # a 64-bit integer seed is the same key
    assert np.array_equal(noise.deviates(678 << 32 | 12345, 4, 1), z)
    # one call serves a cell pair: cells 0, 1 are the two halves of counter 0
    w = noise.philox4x32((0, 0, 0, 0), KEY)
    s = [(int(a) & 0xFFFF) + (int(a) >> 16) + (int(b) & 0xFFFF) + (int(b) >> 16) for a, b in ((w[0], w[1]), (w[2], w[3]))]
    want = [(f32(x) - f32(131070.0)) * noise.Z_SCALE for x in s]
    assert z[0, 0, :2].tolist() == want
    assert noise.Z_SCALE == f32(np.sqrt(3.0 / (65536.0 ** 2 - 1.0))) and noise.Z_SCALE.view(np.uint32) == 0x37DDB3D7


def test_statistics_at_four_standard_errors():
    """96 x 48, steps 0 ... 399: 1 843 200 deviates.  Measured: mean -1.7e-4, variance 1.00012, max |z| 3.338, excess kurtosis
    -0.298, lag-1 correlation -4e-4, neighbour correlation -1.1e-3.  The variance of a sample variance of N deviates with
    excess kurtosis g is (2 + g) / N: four standard errors are 4 sqrt(1.7 / N) = 3.8e-3."""
    z = noise.deviates(KEY, 96, 48, (1, 1), 1, range(400)).astype(np.float64)
    n = z.size
    assert n == 1843200
    se = 4.0 / np.sqrt(n)
    mean, var = z.mean(), z.var()
    kurt = (z ** 4).mean() / var ** 2 - 3.0
    lag1 = (z[1:] * z[:-1]).mean()
    nb = (z[:, :, 1:] * z[:, :, :-1]).mean()
    print(f"mean {mean:.2e} var {var:.5f} max |z| {np.abs(z).max():.3f} excess kurtosis {kurt:.3f} lag-1 {lag1:.1e} neighbour {nb:.1e}")
    assert abs(mean) < se and se < 2.95e-3
    assert abs(var - 1.0) < 3.8e-3
    assert abs(lag1) < se and abs(nb) < se
    assert np.abs(z).max() <= noise.Z_MAX
    assert abs(kurt + 0.3) < 0.02  # a sum of four uniforms: -1.2 / 4


def test_cells_and_hold():
    nx, ny = 96, 48
    z = noise.deviates(KEY, nx, ny, (4, 5), 7, range(0, 22))
    # constant inside a cell, and the last cell row is short: 48 = 9 * 5 + 3
    for j0 in range(0, ny, 5):
        rows = z[:, j0:min(j0 + 5, ny)]
        assert (rows == rows[:, :1]).all()
    assert ny % 5 == 3 and np.array_equal(z[:, 45], z[:, 47]) and not np.array_equal(z[:, 44], z[:, 45])
    assert (z.reshape(22, ny, nx // 4, 4) == z.reshape(22, ny, nx // 4, 4)[..., :1]).all()
    # it changes at cell boundaries (every boundary of a row and a column of cells: no two neighbours agree)
    assert (z[0, 0, 3:-1:4] != z[0, 0, 4::4]).all() and (z[0, 4:-1:5, 0] != z[0, 5::5, 0]).all()
    # constant over `hold` steps, changing at block boundaries
    for t in range(21):
        assert np.array_equal(z[t], z[t + 1]) == ((t + 1) % 7 != 0), t
    # hold 7 carries across the year boundary: 729 and 730 are both block 104
    a = noise.deviates(KEY, nx, ny, (1, 1), 7, (727, 728, 729, 730, 734, 735))
    assert 729 // 7 == 730 // 7 == 104
    assert np.array_equal(a[1], a[2]) and np.array_equal(a[2], a[3]) and np.array_equal(a[3], a[4])
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[4], a[5])
    # the high counter word: step 2^32 + 5 at hold 1 is not step 5
    b = noise.deviates(KEY, nx, ny, (2, 1), 1, (5, 2 ** 32 + 5))
    assert not np.array_equal(b[0], b[1]) and np.abs(b).max() <= noise.Z_MAX
    # cell (2, 1): pairs of longitudes
    assert np.array_equal(b[0][:, 0::2], b[0][:, 1::2]) and (b[0][:, 1:-1:2] != b[0][:, 2::2]).mean() > 0.99
    for bad in ((3, 1), (1, 0), (1, 49)):
        with pytest.raises(ValueError):
            noise.deviates(KEY, nx, ny, bad)
    with pytest.raises(ValueError):
        noise.deviates(KEY, nx, ny, (1, 1), 0)


def test_field_is_one_rounding_per_operation():
    rng = np.random.default_rng(2)
    sigma = (30.0 * rng.random((48, 96))).astype(f32)
    season = rng.random(730).astype(f32)
    steps = (0, 729, 730, 2 ** 32 + 5)
    n = noise.field(sigma, season, (2, 3), 6, KEY, 1.7, steps)
    z = noise.deviates(KEY, 96, 48, (2, 3), 6, steps)
    assert n.dtype == f32
    for t, s in enumerate(steps):
        want = np.empty((48, 96), f32)
        for j in range(0, 48, 7):  # (a few rows, scalar by scalar)
            for i in range(96):
                want[j, i] = f32(f32(f32(sigma[j, i] * season[s % 730]) * f32(1.7)) * z[t, j, i])
            assert np.array_equal(n[t, j], want[j])
    # common random numbers: the pattern is not part of the counter -- 2 sigma at half the amplitude is the same field
    assert np.array_equal(noise.field(2 * sigma, season, (2, 3), 6, KEY, 0.85, steps), noise.field(sigma, season, (2, 3), 6, KEY, 1.7, steps))
    assert np.array_equal(noise.field(sigma, None, (1, 1), 1, KEY, 1.0, (3,)), (sigma * noise.deviates(KEY, 96, 48, steps=(3,))[0])[None])


def test_seeds_are_distinct():
    s = noise.seeds(4096, 7)
    assert len(set(s)) == 4096 and all(0 <= x < 2 ** 64 for x in s)
    assert noise.seeds(3, 7) == s[:3] and noise.seeds(3, 8)[:2] == s[1:3]
    assert len({x >> 32 for x in s}) > 4000 and len({x & 0xFFFFFFFF for x in s}) > 4000  # both key words vary


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.fixture(scope="module")
def years(oracle_lib, inputs, params):
    """One flux-correction year; from its end the mirror year without a hook, with case 2's noise at amp 0, and at amp 1."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    args = (inputs.tclim, inputs.z_topo, inputs.sw_solar)
    sigma, season, cell, hold, n = noise_mirror.case2(inputs)
    plain = sst_mirror.run_year(o, start, CO2, None, *args)
    off = noise_mirror.run_year(o, start, CO2, noise_mirror.Noise(sigma, season, cell, hold, n.seed, 0.0), *args)
    on = noise_mirror.run_year(o, start, CO2, n, *args)
    o.close()
    return dict(plain=plain, off=off, on=on)


def test_amp_zero_mirror_year_equals_the_unhooked_year(years):
    for got, want, name in zip(years["off"], years["plain"], ("monthly", "budget", "state", "yearly")):
        assert np.array_equal(got, want), name


def test_noisy_mirror_year_differs_from_the_unhooked_year(years):
    d = np.asarray(years["on"][0][11, 0], np.float64) - years["plain"][0][11, 0]
    r = float(np.sqrt((d * d).mean()))
    print(f"December Tsurf, noisy mirror year against the plain one: RMS {r:.3e} K")
    assert r > 1e-2
    assert not np.array_equal(years["on"][2], years["plain"][2])


def test_case2_tables_are_what_the_gpu_case_asks_for(inputs):
    sigma, season, cell, hold, n = noise_mirror.case2(inputs)
    ocean = np.asarray(inputs.z_topo) < 0
    assert (sigma[ocean] == 30.0).all() and (sigma[~ocean] == 10.0).all() and ocean.any() and (~ocean).any()
    assert cell == (2, 3) and hold == 6 and season.min() >= 1.0 and season.max() > 1.2


# ------------------------------------------------------------------------------------------------ header and exports
def test_header_and_exports_carry_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    from greb_climate_model_amd import engine
    for name in ("greb_engine_set_noise_tables", "greb_engine_set_member_noise", "greb_engine_get_noise"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in engine.EXPORTS and hasattr(lib, name), name
    m = re.search(r"typedef struct greb_member_noise \{(.*?)\} greb_member_noise;", hdr, re.S)
    fields = []
    for t, names in re.findall(r"(int32_t|uint32_t|float)\s+([\w, ]+);", m.group(1)):
        fields += [(n.strip(), {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}[t]) for n in names.split(",")]
    assert fields == list(abi.GrebMemberNoise._fields_)
    assert C.sizeof(abi.GrebMemberNoise) == 16
    assert int(re.search(r"#define\s+GREB_MAX_NOISE_PATTERNS\s+(\d+)", hdr).group(1)) == abi.MAX_NOISE_PATTERNS == 16
    assert int(re.search(r"#define\s+GREB_NBUDGET\s+(\d+)", hdr).group(1)) == 13  # the noise is not a budget term
    for name in ("set_noise_tables", "set_member_noise", "noise"):
        assert hasattr(engine.Engine, name)


def test_calls_reject_a_null_engine(lib):
    """Argument errors come before anything touches a device."""
    abi.noise_prototypes(lib)
    a = np.ones((1, 48, 96), f32)
    s = (abi.GrebMemberNoise * 1)()
    for rc in (lib.greb_engine_set_noise_tables(None, 1, abi.fptr(a), None, None, None, None),
               lib.greb_engine_set_noise_tables(None, 0, None, None, None, None, None),
               lib.greb_engine_set_member_noise(None, s), lib.greb_engine_set_member_noise(None, None),
               lib.greb_engine_get_noise(None, 0, 0, abi.fptr(a))):
        assert rc in (-1, -3), rc
    lib.greb_engine_last_error.restype = C.c_char_p
    assert b"no engine" in lib.greb_engine_last_error(None)
