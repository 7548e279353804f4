"""The launch orders of the row-strip kernels, task for task as pinned in tests/golden/strip_orders.npz
(make_golden_strip_orders.py): the circulation sub-step, the one-launch circulation call (including the budgets where it
declines) and the batched diffusion sweep.  Host-only entry points, no GPU needed."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_strip_orders", os.path.join(HERE, "golden", "make_golden_strip_orders.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

GOLD = np.load(os.path.join(HERE, "golden", "strip_orders.npz"))
CASES = list(M.cases())


def test_the_pin_covers_every_case():
    assert sorted(f"{key}_{n}" for key, _, names in CASES for n in names) == sorted(GOLD.files)


@pytest.mark.parametrize("key,fn,names", CASES, ids=[c[0] for c in CASES])
def test_order_is_the_pinned_one(key, fn, names):
    for name, got in zip(names, fn()):
        want = GOLD[f"{key}_{name}"]
        np.testing.assert_array_equal(np.asarray(got, np.int32), want, err_msg=f"{key}: {name}")
