#!/usr/bin/env python3
"""CPU model of the LDS traffic of the fused member kernel's sub-step loop (no GPU).

The library hands out the float offset of every LDS access of every lane of every dealt bulk pass of one sub-step
(greb_member_lds_table: made from the kernel's deal, task enumeration and LDS map).  This applies the lane groups and the
bank rule of the LDS to it and prints, per kind of access, the LDS-array cycles against the cycles of a conflict-free
layout (one per lane group with an active lane):
  ds_read_b128    4 groups of 16 lanes {0-3,12-15,20-27} {4-11,16-19,28-31} and the same + 32;  bank = dword address mod 64
  ds_write_b128   8 groups of 8 consecutive lanes;                                              bank = dword address mod 32
  ds_read_b32     2 groups of 32 consecutive lanes;                                             bank = dword address mod 32
Only the lanes of a group conflict, lanes with the same address share one access, and every further distinct address on a
bank costs the group one more cycle.  The polar rows' chain wave and the point physics are not modelled.

  python tools/lds_conflicts.py [fast|strict] [library]
`library`: a variant build to model instead of the release library, e.g. the row-major enumeration
(python -m greb_climate_model_amd.build variant rowmajor tuning greb_member.hip -DGREB_TASKS_ROW_MAJOR)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_G16 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_B128 = (_G16 + [[l + 32 for l in g] for g in _G16], 64)
WRITE_B128 = ([list(range(8 * i, 8 * i + 8)) for i in range(8)], 32)
READ_B32 = ([list(range(32)), list(range(32, 64))], 32)


def instruction_cycles(offsets, store, nbytes):
    """(cycles, conflict-free cycles) of one wave instruction; offsets: 64 float offsets, -1 = lane inactive."""
    groups, banks = WRITE_B128 if store else (READ_B128 if nbytes == 16 else READ_B32)
    cyc = free = 0
    for g in groups:
        on_bank = {}
        for lane in g:
            a = int(offsets[lane])
            if a < 0:
                continue
            for d in range(nbytes // 4):
                on_bank.setdefault((a + d) % banks, set()).add(a)
        if on_bank:
            free += 1
            cyc += max(len(s) for s in on_bank.values())
    return cyc, free


def model(table, kinds):
    """{kind name: [cycles, conflict-free cycles, instructions]} of a table of engine.member_lds_table."""
    out = {k: [0, 0, 0] for k in kinds}
    t = table[np.lexsort((table[:, 3], table[:, 2], table[:, 1], table[:, 0]))]
    assert len(t) % 64 == 0
    for ins in t.reshape(-1, 64, 7):
        assert (ins[:, :3] == ins[0, :3]).all() and (ins[:, 3] == np.arange(64)).all() and (ins[:, 4:6] == ins[0, 4:6]).all()
        kind, nbytes = kinds[ins[0, 4]], int(ins[0, 5])
        c, f = instruction_cycles(ins[:, 6], kind == "store", nbytes)
        o = out[kind]
        o[0] += c; o[1] += f; o[2] += 1
    return out


def reads_b128(m):
    """cycles and conflict-free cycles of the loop's ds_read_b128: columns, left / right quads and winds"""
    return [sum(m[k][i] for k in ("column", "side", "wind")) for i in (0, 1)]


def main():
    from greb_climate_model_amd import build, engine
    strict = sys.argv[1:2] == ["strict"]
    if len(sys.argv) > 2:
        engine._lib_path = os.path.abspath(sys.argv[2])
    else:
        build.build_lib()
    m = model(engine.member_lds_table(strict), engine.LDS_KINDS)
    print(f"{'STRICT' if strict else 'FAST'} bulk waves, one sub-step ({os.path.basename(engine._lib_path)}): LDS-array cycles")
    print(f"{'access':28s} {'instr':>6s} {'cycles':>7s} {'conflict-free':>14s}")
    names = {"side": "X and W left/right quads", "wind": "winds (WX, WY)", "column": "X and W columns", "store": "stores (ds_write_b128)",
             "const": "row constants"}
    for k in ("side", "wind", "column"):
        print(f"{names[k]:28s} {m[k][2]:6d} {m[k][0]:7d} {m[k][1]:14d}")
    r = reads_b128(m)
    print(f"{'total ds_read_b128':28s} {sum(m[k][2] for k in ('side', 'wind', 'column')):6d} {r[0]:7d} {r[1]:14d}   x {r[0] / r[1]:.3f}")
    for k in ("store", "const"):
        print(f"{names[k]:28s} {m[k][2]:6d} {m[k][0]:7d} {m[k][1]:14d}")
    print(f"per member-year (24 sub-steps x 730 steps): {r[0] * 24 * 730 / 1e6:.2f} M read cycles, {(r[0] - r[1]) * 24 * 730 / 1e6:.2f} M of them conflicts")


if __name__ == "__main__":
    main()
