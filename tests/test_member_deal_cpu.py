"""CPU: the fused member kernel's static work deal (greb_member_deal.h: deal_fast / deal_strict, task_rowquad) computes every
4-longitude quad of rows 1 .. 46 exactly once per sub-step and leaves the polar rows to their own waves.  The library
proves this when it is compiled (static_assert on deal_is_complete); greb_member_deal_cover hands out the same constexpr
table -- counted by row-quads from the very enumeration the kernel's lanes use, not by pass indices -- so a deal that
drops or doubles a task is visible here too."""
import ctypes as C

import numpy as np
import pytest

from greb_climate_model_amd import build, engine


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


@pytest.mark.parametrize("strict", [False, True])
def test_every_row_quad_is_dealt_exactly_once(lib, strict):
    cover = engine.member_deal_cover(strict)
    assert cover.shape == (48, 24) and cover.dtype == np.int32
    want = np.ones((48, 24), np.int32)
    want[0] = want[47] = 0  # the polar rows: the chain wave(s)
    bad = np.argwhere(cover != want)
    assert bad.size == 0, [(int(k), int(q), int(cover[k, q])) for k, q in bad[:8]]
    assert int(cover[10:38].sum()) == 28 * 24  # the full family: 672 row-quads


def test_bad_argument_is_an_error(lib):
    assert lib.greb_member_deal_cover(0, None) == -1
    out = (C.c_int * (48 * 24))(*([7] * (48 * 24)))
    assert lib.greb_member_deal_cover(1, out) == 0 and set(out) == {0, 1}

