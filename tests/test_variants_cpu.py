"""CPU: which variant of the step kernels a launch takes (greb_kernels.h: kVariants, select_variant), and that the built
library holds exactly those kernels.  greb_step_variant goes through the selection the launchers go through and
greb_step_variants hands out the list they pick from, so a rule that drifts from the list, or a list entry nothing can
reach, shows here and not as a missing kernel on the GPU.  The expected masks below were read off the launchers' if-chains
as they stood before the selection became one function; they are written out, not computed."""
import ctypes as C
import itertools
import re

import pytest

from greb_climate_model_amd import build, engine
from test_isa_cpu import _kernel_notes, code_objects  # noqa: F401  (code_objects: the module fixture, reused here)

FLUX, EXP, BUDGET, FORCE, BOUND = 1, 2, 4, 8, 16

ELEVEN = [0, FLUX, EXP, FLUX | EXP, BUDGET, EXP | BUDGET, EXP | FORCE, EXP | BUDGET | FORCE, FLUX | EXP | BOUND,
          EXP | FORCE | BOUND, EXP | BUDGET | FORCE | BOUND]

# (flux_phase, switches, budget, forced, on_sets) -> mask
EXPECTED = {
    "plain, flux phase": ((1, 0, 0, 0, 0), FLUX),
    "plain, scenario": ((0, 0, 0, 0, 0), 0),
    "switches, flux phase": ((1, 1, 0, 0, 0), FLUX | EXP),
    "switches, scenario": ((0, 1, 0, 0, 0), EXP),
    "budget": ((0, 0, 1, 0, 0), BUDGET),
    "budget + switches": ((0, 1, 1, 0, 0), EXP | BUDGET),
    "forced": ((0, 0, 0, 1, 0), EXP | FORCE),
    "forced + switches": ((0, 1, 0, 1, 0), EXP | FORCE),
    "forced + budget": ((0, 0, 1, 1, 0), EXP | BUDGET | FORCE),
    "on sets, flux phase": ((1, 0, 0, 0, 1), FLUX | EXP | BOUND),
    "on sets + forced, flux phase": ((1, 0, 0, 1, 1), FLUX | EXP | BOUND),
    "on sets, scenario": ((0, 0, 0, 0, 1), EXP | FORCE | BOUND),
    "on sets + forced, scenario": ((0, 0, 0, 1, 1), EXP | FORCE | BOUND),
    "on sets + budget": ((0, 0, 1, 0, 1), EXP | BUDGET | FORCE | BOUND),
}
# the flux-correction phase delivers no budget; a forced launch without a boundary set exists in the scenario phase only
REJECTED = [(1, sw, 1, fo, bs) for sw in (0, 1) for fo in (0, 1) for bs in (0, 1)] + [(1, sw, 0, 1, 0) for sw in (0, 1)]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


def test_both_calls_are_exported(lib):
    for name in ("greb_step_variant", "greb_step_variants"):
        assert name in engine.EXPORTS and hasattr(lib, name)


def test_the_list_is_the_eleven_variants(lib):
    assert engine.step_variants() == ELEVEN
    assert lib.greb_step_variants(None, 0) == 11
    two = (C.c_uint * 3)(7, 7, 7)
    assert lib.greb_step_variants(two, 2) == 11 and list(two) == [0, FLUX, 7]  # capacity is honoured
    assert lib.greb_step_variants(None, 2) == -1 and lib.greb_step_variants(two, -1) == -1


def test_every_flag_combination_reaches_a_listed_variant_and_every_listed_one_is_reached():
    reached = {}
    for flags in itertools.product((0, 1), repeat=5):
        v = engine.step_variant(*flags)
        if v is not None:
            reached.setdefault(v, []).append(flags)
    assert sorted(reached) == sorted(engine.step_variants()), reached
    assert len(reached) == 11 and sum(len(f) for f in reached.values()) == 32 - len(REJECTED)


@pytest.mark.parametrize("label", EXPECTED)
def test_selection_is_what_the_launchers_chains_gave(label):
    flags, mask = EXPECTED[label]
    assert engine.step_variant(*flags) == mask, (label, flags)


def test_switches_change_nothing_above_them():
    """Forcing- and boundary-aware kernels are switch-aware already: the switches of a member do not select another."""
    for flux, budget, forced, on_sets in itertools.product((0, 1), repeat=4):
        if forced or on_sets:
            assert engine.step_variant(flux, 0, budget, forced, on_sets) == engine.step_variant(flux, 1, budget, forced, on_sets)


@pytest.mark.parametrize("flags", REJECTED, ids=lambda f: "".join(map(str, f)))
def test_contradicting_arguments_are_an_error_and_write_nothing(lib, flags):
    v = C.c_uint(0xDEADBEEF)
    assert lib.greb_step_variant(*flags, C.byref(v)) == -1 and v.value == 0xDEADBEEF
    assert b"step_variant" in lib.greb_engine_last_error(None)
    assert engine.step_variant(*flags) is None


def test_null_destination_is_an_error(lib):
    assert lib.greb_step_variant(0, 0, 0, 0, 0, None) == -1


def test_the_library_holds_exactly_the_listed_kernels(code_objects):  # noqa: F811
    """Per arithmetic mode, one member_kernel and one physics_step_kernel for every entry of the list, no more and no fewer:
    <bool STRICT, unsigned V> mangles as ILb<0|1>ELj<V>EE."""
    names = set()
    for path in code_objects:
        names.update(_kernel_notes(path))
    for kernel in ("member_kernel", "physics_step_kernel"):
        got = sorted(n for n in names if re.match(rf"^_ZN4greb\d+{kernel}I", n))
        want = sorted(f"_ZN4greb{len(kernel)}{kernel}ILb{s}ELj{v}EEEv" for s in (0, 1) for v in engine.step_variants())
        assert len(got) == 22 and [re.match(r"^(.*?EEEv)", n).group(1) for n in got] == want, (kernel, got)
