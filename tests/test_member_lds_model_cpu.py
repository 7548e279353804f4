"""CPU: the LDS traffic of the fused member kernel's sub-step loop, modelled from the table the library exports
(greb_member_lds_table: every lane's offsets of every LDS instruction of every dealt bulk pass, made from the kernel's own
deal, task enumeration and LDS map) with the lane groups and the bank rule of the LDS (tools/lds_conflicts.py).

  * the loop's ds_read_b128 take at most 1.05 x the cycles of a conflict-free layout in FAST, and the stores no more than
    under the row-major enumeration this one replaced: 276 cycles (tools/lds_conflicts.py on a -DGREB_TASKS_ROW_MAJOR
    build, profiles/r08_member_lds_groups_model.txt; there the reads took 2 080 cycles against 1 716);
  * every offset lies inside the array its access belongs to;
  * every row-quad of rows 1 .. 46 is stored exactly once, both halves."""
import importlib.util
import os

import numpy as np
import pytest

from greb_climate_model_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE_CYCLES_ROW_MAJOR = 276
NX, NY, NQ = 96, 48, 24


@pytest.fixture(scope="module")
def tool():
    build.build_lib()
    spec = importlib.util.spec_from_file_location("lds_conflicts", os.path.join(ROOT, "tools", "lds_conflicts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module", params=[False, True], ids=["fast", "strict"])
def table(request, tool):
    t = engine.member_lds_table(request.param)
    assert t.ndim == 2 and t.shape[1] == 7 and t.dtype == np.int32 and len(t) % 64 == 0
    return request.param, t


def test_the_model_counts_what_the_guide_says(tool):
    lanes = np.arange(64)
    assert tool.instruction_cycles(4 * lanes, False, 16) == (4, 4)        # consecutive quads: one cycle per group
    assert tool.instruction_cycles(64 * lanes, False, 16) == (64, 4)      # one bank for all: 16-way in each group
    assert tool.instruction_cycles(0 * lanes, False, 16) == (4, 4)        # one address: a broadcast
    assert tool.instruction_cycles(4 * lanes, True, 16) == (8, 8)         # stores: 8 lanes x 4 dwords = the 32 banks
    assert tool.instruction_cycles(32 * lanes, True, 16) == (64, 8)
    a = 4 * lanes
    a[4] = a[0] + 64                                                      # lanes 0 and 4 are in different read groups
    assert tool.instruction_cycles(a, False, 16) == (4, 4)
    a[12] = a[0] + 64                                                     # lanes 0 and 12 share one
    assert tool.instruction_cycles(a, False, 16) == (5, 4)
    a[:] = -1
    a[:32] = 4 * lanes[:32]
    assert tool.instruction_cycles(a, False, 16) == (2, 2)                # an idle half wave costs nothing


def test_reads_are_nearly_conflict_free_and_stores_no_worse(tool, table):
    strict, t = table
    m = tool.model(t, engine.LDS_KINDS)
    cyc, free = tool.reads_b128(m)
    print(f"{'STRICT' if strict else 'FAST'}: ds_read_b128 {cyc} cycles, conflict-free {free}; stores {m['store'][0]} / {m['store'][1]}")
    if not strict:
        assert free == 1716 and m["store"][2] == 6 * 4 + 6 * 2  # 444 reads x 4 groups less the idle half of the short F1 pass
        assert cyc <= 1.05 * free, (cyc, free)
        assert m["store"][0] <= STORE_CYCLES_ROW_MAJOR, m["store"]
    else:  # the same enumeration under the STRICT deal
        assert cyc <= 1.05 * free, (cyc, free)
        assert m["store"][0] == m["store"][1], m["store"]


def test_every_offset_lies_inside_its_array(table):
    strict, t = table
    lm = engine.member_lds_map()
    RS, XB = lm["RS"], lm["X1"] - lm["X0"]
    assert lm["END"] * 4 <= 160 * 1024 and XB == (NY + 2) * RS
    t = t[t[:, 6] >= 0]
    kind, nbytes, off = t[:, 4], t[:, 5], t[:, 6].astype(np.int64)
    assert (nbytes[kind != 4] == 16).all() and (off[nbytes == 16] % 4 == 0).all()
    name = np.array(engine.LDS_KINDS)[kind]

    def rows_of(sel, base):  # (row with the guard row as -1, float within the row)
        r = off[sel] - base
        assert ((r >= 0) & (r < XB)).all()
        return r // RS - 1, r % RS

    for k in ("column", "side"):  # reads of buffer 0 of X, or of W
        sel = name == k
        in_w = off[sel] >= lm["W"]
        for base, part in ((lm["X0"], ~in_w), (lm["W"], in_w)):
            idx = np.flatnonzero(sel)[part]
            assert len(idx)
            row, x = rows_of(idx, base)
            assert (x + 4 <= 2 * NX).all(), k                                    # not in the row's padding
            lo, hi = (-1, NY) if k == "column" else (1, NY - 2)                   # the column reaches the guard rows
            assert row.min() == lo and row.max() == hi, (k, row.min(), row.max())
    sel = name == "store"                                                         # buffer 1 of X, rows 1 .. 46
    row, x = rows_of(sel, lm["X1"])
    assert (x + 4 <= 2 * NX).all() and row.min() == 1 and row.max() == NY - 2
    sel = name == "wind"
    w = off[sel] - lm["WX"]
    assert ((w >= 0) & (w + 4 <= 2 * NX * NY)).all() and (w % (NX * NY) + 4 <= NX * NY).all()
    assert ((w % (NX * NY)) // NX).min() == 1 and ((w % (NX * NY)) // NX).max() == NY - 2
    sel = name == "const"
    c = off[sel]
    assert ((c >= lm["ROWK"]) & (c + nbytes[sel] // 4 <= lm["END"])).all()


def test_every_row_quad_is_stored_exactly_once(table):
    strict, t = table
    lm = engine.member_lds_map()
    RS = lm["RS"]
    st = t[(t[:, 4] == 3) & (t[:, 6] >= 0)][:, 6].astype(np.int64) - lm["X1"]
    row, x = st // RS - 1, st % RS
    count = np.zeros((NY, 2, NQ), np.int32)  # [row][half][quad]: the [half][quad][4] row layout
    np.add.at(count, (row, x // NX, (x % NX) // 4), 1)
    want = np.ones_like(count)
    want[0] = want[NY - 1] = 0
    bad = np.argwhere(count != want)
    assert bad.size == 0, bad[:8].tolist()
    # lanes without a task exist only in the upper half of the two short passes
    lanes_idle = t[t[:, 6] < 0]
    assert set(np.unique(lanes_idle[:, 3]).tolist()) <= set(range(32, 64))
