// greb_member_grid.h -- the fused member kernel's grid constants and its padded row stride: plain constants, no includes
// (greb_member_lds.h lays the LDS out with them, greb_member_deal.h deals the tasks with them)
#pragma once

namespace greb {

constexpr int NX = 96, NY = 48, NQ = 24, NP = 4608;
constexpr int kThreads = 512;
// floats per interleaved row: 2*NX = 192 data + 16 of padding, i.e. a row stride of 52 sixteen-byte slots = 4 mod 16.
// A ds_read_b128 is served in four groups of 16 lanes, which are NOT consecutive lanes: {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same two + 32; a ds_write_b128 in eight groups of 8 consecutive lanes.  The bank of a
// dword is its address mod 64 (stores: mod 32), so the 16 lanes of a read group take one LDS cycle when their slots fall
// into 16 different slot classes (slot mod 16), the 8 of a store group when theirs differ mod 8; every further slot of a
// class costs the group a cycle.  With the unpadded stride (48 slots = 0 mod 16) every row started in the same class
// (42 % of the LDS cycles of the round-1 kernel were bank conflicts); with 4 mod 16, rows 2 mod 4 apart are offset by 8
// classes, and 8 consecutive quads of one row and of the other fill the 16 classes.  What the layout guarantees today
// (task_rowquad deals the lanes of a pass to these groups; tools/lds_conflicts.py counts it from the kernel's own
// tables, tests/test_member_lds_model_cpu.py holds it): every ds_read_b128 of X and W in the sub-step loop -- column,
// left and right quads, the seam between quads 23 and 0 included -- and every store is conflict-free; of the wind reads
// (WX, WY: row stride 24 slots = 8 mod 16, no padding) those of a third of the read groups are 2-way: 1 760 modelled
// cycles per sub-step against 1 716 conflict-free, where the row-major enumeration took 2 080.  (The 9.6 KB the padding
// costs are those of the polar chains' former Jacobi row buffers plus the slack: the chains exchange their halos by
// ds_bpermute now.)
constexpr int RS = 2 * NX + 16;

} // namespace greb
