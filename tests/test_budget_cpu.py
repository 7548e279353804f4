"""CPU: the budget output's ABI (include/greb_engine.h: GREB_NBUDGET, GREB_B_*, greb_budget_name,
greb_engine_run_budget) and the yardstick of its GPU tests -- tests/budget_mirror.py, a scenario year stepped from Python
over the oracle's per-routine entry points -- held to Oracle.run bit for bit before anything is measured against it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import budget_mirror
from greb_climate_model_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_lib())


def test_budget_symbols_resolve(lib):
    for name in ("greb_engine_run_budget", "greb_budget_name"):
        assert hasattr(lib, name), name
    from greb_climate_model_amd import engine
    assert {"greb_engine_run_budget", "greb_budget_name"} <= set(engine.EXPORTS)


def test_budget_names_match_the_python_list(lib):
    f = lib.greb_budget_name
    f.restype = C.c_char_p
    f.argtypes = [C.c_int]
    assert [f(i).decode() for i in range(abi.NBUDGET)] == list(abi.BUDGET_NAMES)
    assert f(abi.NBUDGET) is None and f(-1) is None


def test_header_constants_match_abi_py():
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    assert int(re.search(r"#define\s+GREB_NBUDGET\s+(\d+)", hdr).group(1)) == abi.NBUDGET == 13
    idx = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+GREB_B_(\w+)\s+(\d+)", hdr)}
    assert len(idx) == abi.NBUDGET and sorted(idx.values()) == list(range(abi.NBUDGET)), idx
    for name, i in idx.items():
        assert getattr(abi, "B_" + name) == i, name
        assert abi.BUDGET_NAMES[i].lower() == name.lower(), (name, abi.BUDGET_NAMES[i])


def test_run_budget_null_arguments_fail_without_a_device(lib):
    """Argument errors come before anything touches a device: no engine -> GREB_E_INVALID."""
    assert lib.greb_engine_run_budget(None, 1, None, None, None, None, 0) == -1


def test_mirror_year_equals_oracle_run(oracle_lib, inputs, params):
    """The yardstick is checked before it is used: after one flux-correction year, one scenario year of the mirror and one
    of Oracle.run from the same state give the same 12 x 5 records and the same final state, bit for bit."""
    o = oracle_lib.Oracle(inputs, params)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    monthly, budget, state = budget_mirror.run_year(o, start, 680.0)
    start.restore(o)
    ref, _ = o.run(1, 680.0)
    assert np.array_equal(monthly, ref[0]), float(np.abs(monthly.astype(np.float64) - ref[0]).max())
    assert np.array_equal(state, o.state5())
    o.close()
    # the thirteen sums are real fields: finite, the signs the update expects, something everywhere it should be
    assert budget.shape == (12, abi.NBUDGET, inputs.ny, inputs.nx) and np.isfinite(budget).all()
    assert (budget[:, abi.B_SW] >= 0).all() and (budget[:, abi.B_LW_SURF] < 0).all()
    assert (budget[:, abi.B_DQ_RAIN] <= 0).all() and np.abs(budget[:, abi.B_DQ_EVA]).max() > 0
    assert np.abs(budget[:, abi.B_DTA_CRCL]).max() > 1e-3
