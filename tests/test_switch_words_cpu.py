"""CPU: the oracle takes any of the 256 switch words (oracle_set_switches; every physics branch of oracle/greb_oracle.c
tests one GREB_X_* bit), and the fixture of 24 such words (tests/switch_words.py, tests/golden/switch_words_g96.npz) is
what the oracle gives.  That the oracle keyed on bits is still the upstream variant for the ten pinned experiments is
tests/test_logexp_cpu.py, unchanged; here: the map log_exp -> word, that a word alone drives the same run, the fixture,
the precedence of the three transport bits, and the one combination under which the model itself blows up."""
import hashlib
import json
import os

import numpy as np
import pytest

import switch_words as SW
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    return SW.load_fixture(GOLDEN)


def test_manifest_lists_the_word_sets():
    it = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))["items"]["switch_words_g96"]
    assert it["recipe"] == "tests/golden/make_golden_switch_words.py"
    assert [int(w, 16) for w in it["set_a_own_spin_up"]] == list(SW.SET_A)
    assert [int(w, 16) for w in it["set_b_shared_spin_up"]] == list(SW.SET_B)


def test_set_a_is_a_resolution_iv_fraction():
    """Every pair of bits meets in all four states; every state of the three transport bits occurs twice."""
    a = np.asarray(SW.SET_A)
    for i in range(8):
        for j in range(i + 1, 8):
            assert sorted(set(zip((a >> i) & 1, (a >> j) & 1))) == [(0, 0), (0, 1), (1, 0), (1, 1)], (i, j)
    assert sorted(np.bincount((a >> 4) & 7, minlength=8)) == [2] * 8
    assert not any(w & 0x10 for w in SW.SET_B) and len(set(SW.SET_A) | set(SW.SET_B)) == 24


def test_log_exp_map_of_the_oracle(inputs, oracle_lib):
    """The table of tests/test_gpu_logexp.py::test_switch_map_matches_the_original_conditions; 4, 7, 16 and below 4 completed
    from the conditions of greb_log_exp_switches (csrc/greb_members.cpp)."""
    from greb_climate_model_amd import abi
    nothing_runs = abi.X_NO_ICE | abi.X_NO_HYDRO | abi.X_NO_DEEP_OCEAN | abi.X_NO_CIRCULATION
    want = {1: nothing_runs, 2: nothing_runs, 3: nothing_runs, 4: nothing_runs,
            5: abi.X_NO_ICE | abi.X_NO_HYDRO | abi.X_NO_DEEP_OCEAN,
            6: abi.X_NO_HYDRO | abi.X_NO_DEEP_OCEAN,
            7: abi.X_NO_VAPOR_TRANSPORT | abi.X_NO_DEEP_OCEAN,
            8: abi.X_VAPOR_DIFFUSION_ONLY | abi.X_NO_DEEP_OCEAN,
            9: abi.X_NO_DEEP_OCEAN, 10: 0,
            11: abi.X_LW_LINEAR_VAPOR | abi.X_NO_DEEP_OCEAN, 12: 0,
            13: abi.X_NO_HYDRO,
            14: abi.X_NO_DEEP_OCEAN | abi.X_SST_PLUS1,
            15: abi.X_NO_HYDRO | abi.X_NO_DEEP_OCEAN | abi.X_SST_PLUS1,
            16: abi.X_NO_VAPOR_TRANSPORT | abi.X_NO_DEEP_OCEAN | abi.X_SST_PLUS1}
    assert (abi.X_NO_ICE, abi.X_NO_HYDRO, abi.X_NO_DEEP_OCEAN, abi.X_LW_LINEAR_VAPOR, abi.X_NO_CIRCULATION,
            abi.X_NO_VAPOR_TRANSPORT, abi.X_VAPOR_DIFFUSION_ONLY, abi.X_SST_PLUS1) == tuple(1 << b for b in range(8))
    o = oracle_lib.Oracle(inputs)
    got = {le: o.log_exp_switches(le) for le in range(1, 17)}
    with pytest.raises(ValueError):
        o.set_switches(0x100)
    o.close()
    assert got == want


@pytest.mark.parametrize("log_exp", (5, 8, 11, 15, 16))
def test_a_word_alone_drives_the_experiment(inputs, oracle_lib, log_exp):
    """Oracle.run_original (boundary data changed by oracle_set_log_exp, branches by the word it derives) against an oracle
    that never hears of log_exp: made on original.experiment_inputs, given the word, the same CO2 and the same phases."""
    from greb_climate_model_amd import abi, original

    def original_params():  # greb.original.model.f90:69, as tests/test_logexp_cpu.py
        return abi.default_params(cp_land=float(np.float32(4186.0) / np.float32(4.5)))
    o = oracle_lib.Oracle(inputs, original_params())
    _, want = o.run_original(log_exp, 1, 0, 1)
    word = o.log_exp_switches(log_exp)
    o.close()
    co2_ctrl = 340.0
    o = oracle_lib.Oracle(original.experiment_inputs(inputs, log_exp), original_params())
    o.lib.oracle_set_co2_flux(o.h, oracle_lib.C.c_float(co2_ctrl))
    o.set_switches(word)
    o.flux_correction(1)
    o.begin_run(np.stack([o.field(i).copy() for i in range(4)]), 1940.0, scenario=True)
    got, _ = o.run(1, co2_ctrl if log_exp >= 14 else original.co2_level(log_exp, 1940.0))
    o.close()
    assert np.isfinite(want).all() and np.array_equal(got, want)


SHA_CASES = tuple(("a", w) for w in SW.SET_A if w & 0x10) + (("a", 0x00), ("a", 0xc5), ("a", 0x2d), ("b", 0x4c), ("b", 0xa2))


@pytest.mark.parametrize("which,word", SHA_CASES, ids=[SW.key(*c) for c in SHA_CASES])
def test_oracle_reproduces_the_fixture(inputs, params, oracle_lib, fixture, which, word):
    mon, yr = SW.oracle_case(oracle_lib, inputs, params, which, word)
    c = fixture[SW.key(which, word)]
    assert hashlib.sha256(np.ascontiguousarray(mon[0]).tobytes()).digest() == c["sha256"]
    assert np.array_equal(mon[0, -1], c["last"]) and np.array_equal(yr, c["yearly"])
    assert np.array_equal(mon[0].astype(np.float64).mean(axis=(2, 3)), c["means"])


def test_fixture_is_finite_and_its_bars_are_the_tolerance_or_three_times_the_noise(fixture):
    tol = np.asarray(SW.TOL)
    for k, c in fixture.items():
        assert np.isfinite(c["last"]).all() and np.isfinite(c["means"]).all() and np.isfinite(c["yearly"]).all(), k
        assert (c["noise"] >= 0).all() and (c["noise"] < tol).all(), (k, c["noise"] / tol)  # the yardstick itself is within TOL
        assert (SW.bar(c) >= tol).all() and (SW.bar(c) < 3 * tol).all(), k


def test_transport_precedence_masks_the_lower_bits(inputs, params, oracle_lib):
    """NO_CIRCULATION > NO_VAPOR_TRANSPORT > VAPOR_DIFFUSION_ONLY: a bit below a set one changes nothing, bit for bit."""
    def run(word):
        return SW.oracle_case(oracle_lib, inputs, params, "a", word)
    for group in ((0x10, 0x30, 0x50, 0x70), (0x20, 0x60)):
        want = run(group[0])
        assert np.isfinite(want[0]).all()
        for w in group[1:]:
            got = run(w)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), hex(w)


def test_linear_vapour_without_circulation_blows_up_in_the_model_itself(inputs, params, oracle_lib):
    """LW_LINEAR_VAPOR and NO_CIRCULATION with hydrology (0x18): the oracle, like the engine (profiles/lin_numbers.txt
    section 3), is finite in scenario year 1 and not from year 2 on -- the model's behaviour, not the port's.  With NO_HYDRO
    added (0x1a) it stays finite.  Which values go first is not pinned."""
    mon, yr = SW.oracle_case(oracle_lib, inputs, params, "a", 0x18, years=3)
    assert np.isfinite(mon[0]).all() and np.isfinite(yr[:2]).all()
    assert not np.isfinite(mon[1]).all() and not np.isfinite(mon[2]).all()
    mon, yr = SW.oracle_case(oracle_lib, inputs, params, "a", 0x1a, years=3)
    assert np.isfinite(mon).all() and np.isfinite(yr).all()
