// greb_member_deal.h -- the fused member kernel's schedule: which wave runs which pass of bulk tasks, which (row, quad) a
// lane of a pass holds, and the proof that every row-quad is computed once.  All of it is __host__ __device__ constexpr:
// no LDS access, no builtins -- the kernel (greb_member_bulk.h: make_tasks), the host-visible tables of greb_member.hip
// and a host-only translation unit read the same functions.  It needs the grid constants and, for the two attributes,
// the HIP runtime header: a host compiler that can read that header can read this one.
//
// The schedule (both arithmetic modes).  Task kinds: one row (S1 sub-cycled family, F1 full family) or two stacked rows (ST, FT).
//   ST  rows (1,2) (3,4) (5,6) (7,8) (39,40) .. (45,46) : 8 pairs x 24 quads = 3 full passes
//   FT  rows (10,11) .. (24,25)                          : 8 pairs x 24 quads = 3 full passes
//   S1  rows 9, 38                                       : 48 tasks, one pass
//   F1  rows 26 .. 37                                    : 288 tasks, 4.5 passes
// VALU instructions per pass in FAST before the factor 3 of rows 1 / 46 moved to stage_winds and dif_cc/20 to Circ::init:
// ST 426, FT 306, S1 223, F1 156.  After it the sub-step loop bodies of the bulk waves hold 288 / 346 / 435 / 493 / 493
// vector instructions where they held 290 / 364 / 438 / 512 / 512 (read off the release library's ISA).
// Waves w and w+4 share a SIMD; the polar rows (a dependent chain of 8 + 1 Jacobi sweeps per sub-step) have their own
// wave(s): wave 6 in FAST, waves 2 and 3 in STRICT.  The SIMD's issue arbiter favours the OLDER wave; the younger one runs in the
// slots that leaves, and once the older wave is done the younger runs alone at a single wave's issue rate (one
// instruction per ~5 cycles at best, ~6-7 with its LDS waits) -- so the older wave of a pair carries the larger
// share and the two should finish together.  In-kernel stamps (tools/stamp_member.py) give each wave's busy time
// per sub-step.  The loop is VALU-pipe bound: a packed fp32 instruction occupies the SIMD for ~4.9 cycles (measured,
// tools/ubench/valu_rate.hip; a scalar one ~2.3-2.7).
#pragma once

#include <hip/hip_runtime.h>

#include "greb_member_grid.h"

namespace greb {

enum { kNone = 0, kS1 = 1, kF1 = 2, kST = 3, kFT = 4 };
struct Pass { int kind, index; };
// FAST: ONE wave runs all four polar chains (quad_chain_substep: 36-instruction sweeps, ~2 600 busy cycles per
// sub-step when it has the SIMD to itself, where two waves took ~4 400 each) and there are seven bulk waves.  The chain
// wave issues one instruction every ~5 cycles for as long as it runs; as the OLDER wave of its SIMD it leaves its
// partner little of the pipe until it is done, as the YOUNGER one (wave 6) it fills the slots its partner leaves and
// both finish together.  Measured sub-step times (tools/deal_search.py: in-kernel stamps, 512 members, one GPU session
// per group; slots w0 w1 w2 w3 | w4 w5 w6 w7, C = the chains, S = ST, T = FT, H = S1, F = F1):
//   chains on wave 6 (younger wave of SIMD 2)
//     S0+F0 S2+F1 T1+F3 T2+H+F2 | S1    T0    C     F4      4 773   <- the table until the wind signs became masks
//     S0+F0 S1+H  T1+F3 T2+F1+F2| S2    T0    C     F4      4 814
//     S0+F0 S2+H  T1+F3 T2+F1+F2| S1    T0    C     F4      4 817
//     S0+F0 S2+H  T1+F3 T2+F1   | S1    T0    C     F2+F4   4 886
//     S0+F0 S2+H  T1+F3+F4 T2+F1+F2 | S1 T0   C     -       5 315   (the chains starve behind three passes)
//     S0+F0 S2+H  T1+F3 T2+F1+F2| S1    T0+F4 C     -       5 665
//   chains on wave 2 (older wave of SIMD 2), same call: 4 900
//     S0+F0 S2+H  C     T2+F1+F2| S1    T0    T1+F3 F4      4 900 ... 4 932
//     S0+F0 S2+H  C     T2+F1   | S1    T0    T1+F3 F2+F4   4 975
//     S0+F0 S2+F1 C     T2+H+F2 | S1    T0    T1+F3 F4      4 974
//     S0+F0 S2+H  C     T2+F1+F2| S1    T0    T1    F3+F4   5 070   (wave 7 waits behind wave 3's three passes)
//     S0+F0 S2+T0 C     H+F1+F2 | S1    T2    T1    F3+F4   5 094
//     S0    S2+F0 C     H+F1+F2 | S1    T0    T1+T2 F3+F4   5 988   (two FT passes behind the chain wave)
//   chains on wave 7 (younger wave of SIMD 3): 5 432
// With the table below the busiest wave of each SIMD is busy 4 318 / 4 296 / 4 225 / 4 393 cycles.
// Also measured (same tooling, one call, chains on wave 6, this table 4 684): the full family's 672 row-quads dealt as
// X = 4 passes of (row pair, quad) tasks + 2.5 passes of single rows instead of 3 + 4.5 -- a lane's pair task need not
// belong to a whole row pair -- took 4 654 at best (S0+F0 S2+F1 T1+F2 T2+H | S1 T0 C T3), 4 658 and 4 850 in two other
// deals; X = 5 (+ half a single pass) 5 060 .. 5 641 in four deals: a fifth pair pass finds no SIMD it balances on.  30
// cycles did not pay for a second task enumeration; the split stays 3 + 4.5.
// With the wind signs kept as lane masks (greb_pair.h: wind_term; profiles/r06_member_wind_masks_stamps.txt) every bulk wave
// but wave 3 got shorter under the table above -- its T2+H+F2 stayed at 4 387 busy cycles, sub-step 4 664 where the split
// form took 4 685 -- and the F1 pass F2 moved from wave 3 to wave 7:
//     S0+F0 S2+F1 T1+F3 T2+H    | S1    T0    C     F2+F4   4 579   <- the table below (busy 3 535 3 641 3 127 3 364 | 4 243 4 184 4 154 4 057)
//     S0+F0 S2+F1 T1+F3 T2+F2   | S1    T0    C     H+F4    4 582
//     S0+F0 S2+F1 T1+F3 T2+H+F2 | S1    T0    C     F4      4 664
//     S0    S2+F1 T1+F3 T2+H+F2 | S1    T0    C     F0+F4   4 889
//     S0+F0 S2+F1 T1+F3+F2 T2+H | S1    T0    C     F4      5 089
// With the tasks dealt to the LDS's lane groups (task_rowquad; profiles/r08_member_lds_groups_stamps.txt) every pass got
// shorter and the busiest waves of the four SIMDs moved from 4 221 4 315 4 109 3 931 to 4 128 4 040 4 044 3 900; the table stays:
//     S0+F0 S2+F1 T1+F3 T2+H    | S1    T0    C     F2+F4   4 428   <- the table below (busy 3 417 3 492 2 941 3 191 | 4 128 4 040 4 044 3 900)
//     S0+F0 S2+F1 T1+F3 T2+F2   | S1    T0    C     H+F4    4 449
//     S0+F0 S2+F1 T1+F3 T2+H+F2 | S1    T0    C     F4      4 515
//     S0    S2+F1 T1+F3 T2+H+F2 | S1    T0    C     F0+F4   4 710
__host__ __device__ constexpr Pass deal_fast(int wave, int i) {
  constexpr Pass none{kNone, 0};
#if defined(GREB_TUNING) && defined(GREB_DEAL_FAST) // tools/deal_search.py: a deal given on the compiler command line
  constexpr Pass t[8][3] = {GREB_DEAL_FAST};
#else
  constexpr Pass t[8][3] = {
      /* w0 */ {{kST, 0}, {kF1, 0}, none},     /* w1 */ {{kST, 2}, {kF1, 1}, none},
      /* w2 */ {{kFT, 1}, {kF1, 3}, none},     /* w3 */ {{kFT, 2}, {kS1, 0}, none},
      /* w4 */ {{kST, 1}, none, none},         /* w5 */ {{kFT, 0}, none, none},
      /* w6 */ {none, none, none},             /* w7 */ {{kF1, 2}, {kF1, 4}, none}};
#endif
  return t[wave][i];
}
// STRICT: waves 2 and 3 are the polar waves (chain_substep, one pole each)
__host__ __device__ constexpr Pass deal_strict(int wave, int i) {
  constexpr Pass none{kNone, 0};
  // Measured sub-step times of the deals tried (in-kernel stamps, 512 members, cycles at 2.36 GHz; the first line is
  // round 1's deal):   w0 ST0 FT0 | w4 ST1 ; w1 ST2 F1_0 | w5 S1 F1_1 F1_2 ; w6 FT1 F1_3 ; w7 FT2 F1_4   6 299
  //                    one F1 pass moved from the younger to the older wave of SIMD 1                          5 838
  //                    ... and the other F1 pass of wave 5 moved to wave 6 (pole SIMD)                         6 115
  //                    w0 ST0 F1 F1 | w4 ST1 ; w1 ST2 FT0 | w5 S1 F1 ; w6 FT1 F1 ; w7 FT2 F1                   6 059
  //                    an ST pass on a pole SIMD (w6 ST2), FT1 F1 on w4                                        6 210
  // With the clamp fast path and the polar halos by ds_bpermute (polar waves 4 700 -> 4 100 busy cycles) the second
  // line takes 5 501; the table below -- its S1 pass moved to wave 6, wave 5 left with two F1 passes -- 5 416.
  // Static s_setprio 1 on the younger waves, on waves 6/7 or on the polar waves: 6 847 / 6 661 / 5 855 -- the
  // prioritised wave runs its instructions at ~6 cycles each and its partner then runs alone; age order is best.
  constexpr Pass t[8][3] = {
      /* w0 */ {{kST, 0}, {kFT, 0}, none},     /* w1 */ {{kST, 2}, {kF1, 0}, {kF1, 1}},
      /* w2 */ {none, none, none},             /* w3 */ {none, none, none},
      /* w4 */ {{kST, 1}, none, none},         /* w5 */ {{kF1, 2}, {kF1, 3}, none},
      /* w6 */ {{kFT, 1}, {kS1, 0}, none},     /* w7 */ {{kFT, 2}, {kF1, 4}, none}};
  return t[wave][i];
}
template <bool STRICT>
__host__ __device__ constexpr Pass deal(int wave, int i) { return STRICT ? deal_strict(wave, i) : deal_fast(wave, i); }
#if defined(GREB_TUNING) && defined(GREB_POLAR_WAVE_FAST) // tools/deal_search.py: which wave runs the FAST polar chains
constexpr int kPolarWaveFast = GREB_POLAR_WAVE_FAST;
#else
constexpr int kPolarWaveFast = 6;
#endif
template <bool STRICT>
__host__ __device__ constexpr bool is_polar_wave(int wave) { return STRICT ? (wave == 2 || wave == 3) : wave == kPolarWaveFast; }

// the first row and the quad of task t (= 64 * pass index + lane) of a kind; valid = 0: no such task
struct RowQuad { int k, q, valid; };
__host__ __device__ constexpr int task_rows(int kind) { return kind == kST || kind == kFT ? 2 : (kind == kS1 || kind == kF1 ? 1 : 0); }
__host__ __device__ constexpr int kind_tasks(int kind) {
  return kind == kST || kind == kFT ? 8 * NQ : (kind == kS1 ? 2 * NQ : (kind == kF1 ? 12 * NQ : 0));
}
// The enumeration follows the lane groups of the LDS (see RS).  A SEGMENT is 8 cyclically consecutive quads of a row, from
// quad q0 on: 8 slot classes in a row, shifted as a whole by the reads of the left / right quads unless the shift crosses
// the seam between quads 23 and 0 (24 = 8 mod 16 moves the quads beyond the seam by 8 classes).  A row is cut at
// q0 = rot, rot + 8, rot + 16 with rot = 1 (even rows) or 5 (odd rows): only the third segment holds the seam, and every
// segment starts in slot class 1 mod 8 (a pair task's second row: 5 mod 8).  A read group of 16 lanes holds two segments
// whose classes are 8 apart:
//   the first two segments of ONE row -- conflict-free in the column, left, right and wind reads;
//   the third segments of two rows that are 2 mod 4 apart (same q0, so the seam shifts both alike) -- conflict-free in the
//   X and W reads; in WX / WY (row stride 24 slots = 8 mod 16) these two rows start in the same class, a 2-way conflict
//   on 2 of a row task's reads in a third of the groups, which is what tools/lds_conflicts.py still counts.
// The 32 lanes of a half wave are the chunks c = 0 .. 7 of 4 lanes; read group 0 is {c0, c3, c5, c6}, read group 1
// {c1, c2, c4, c7} (the parity of c's bits), a store group two neighbouring chunks.  Chunk c holds the quads 4 (c & 1) ..
// + 3 of segment (c >> 1) & 1 of its read group, so a store group is the first half of one segment and the second half of
// another: 8 different classes mod 8.
// The rows of a kind in pairs 2 mod 4 apart: groups 3p, 3p + 1 are the two rows' own, 3p + 2 their third segments.
// S1 (rows 9 and 38, 1 mod 4 apart): the two third segments have a read group each, in lanes 32 .. 47.
struct Segment { int k, q0; };
__host__ __device__ constexpr int seg_rot(int k) { return 1 + 4 * (k & 1); }
__host__ __device__ constexpr Segment task_segment(int kind, int group, int member) {
  if (kind == kS1) {
    const int k = group == 0 || group == 3 ? 38 : 9;
    return Segment{k, seg_rot(k) + (group >= 2 ? 16 : 8 * member)};
  }
  const int p = group / 3, g = group % 3;
  int a = 1;
  if (kind == kST) a = p < 2 ? 1 + 4 * p : 31 + 4 * p;             // (1,3) (5,7) (39,41) (43,45)
  else if (kind == kFT) a = 10 + 4 * p;                            // (10,12) .. (22,24)
  else if (kind == kF1) a = 26 + 4 * (p >> 1) + (p & 1);           // (26,28) (27,29) (30,32) .. (35,37)
  const int k = g == 0 ? a : (g == 1 ? a + 2 : a + 2 * member);
  return Segment{k, seg_rot(k) + (g == 2 ? 16 : 8 * member)};
}
// number of passes of a kind, and of tasks of one of its passes: 64 = every lane has one
__host__ __device__ constexpr int kind_passes(int kind) { return kind == kST || kind == kFT ? 3 : (kind == kS1 ? 1 : (kind == kF1 ? 5 : 0)); }
__host__ __device__ constexpr int pass_tasks(int kind, int index) {
  const int left = kind_tasks(kind) - 64 * index;
  return left >= 64 ? 64 : (left > 0 ? left : 0);
}
// The eight segments of a pass, a byte each for the row and for q0: segment s = 4 (half wave) + 2 (read group) + member.
// make_tasks gets them as two 64-bit literals and a lane finds its own with a shift: the enumeration costs the once-per-step
// setup no more instructions than the division by 24 of the row-major one did.
struct PassSegments { unsigned long long k, q0; };
__host__ __device__ constexpr PassSegments pass_segments(int kind, int index) {
  PassSegments p{0, 0};
  for (int s = 0; s < 8; ++s) {
    const int group = 4 * index + (s >> 1);
    const Segment g = 32 * (group >> 1) < kind_tasks(kind) ? task_segment(kind, group, s & 1) : Segment{1, 0};
    p.k |= (unsigned long long)g.k << (8 * s);
    p.q0 |= (unsigned long long)g.q0 << (8 * s);
  }
  return p;
}
// (the task of lane 0 .. 63, whether or not a short pass has one for it)
__host__ __device__ constexpr RowQuad lane_rowquad(const PassSegments& p, int lane) {
  const int s = ((lane >> 5) << 2) | ((((lane >> 2) ^ (lane >> 3) ^ (lane >> 4)) & 1) << 1) | ((lane >> 3) & 1);
  const int k = (int)(p.k >> (8 * s)) & 255, q = ((int)(p.q0 >> (8 * s)) & 255) + (lane & 7);
  return RowQuad{k, q >= NQ ? q - NQ : q, 1};
}
__host__ __device__ constexpr RowQuad task_rowquad(int kind, int t) {
  if (t < 0 || t >= kind_tasks(kind)) return RowQuad{1, 0, 0};
#if defined(GREB_TUNING) && defined(GREB_TASKS_ROW_MAJOR) // tools/lds_conflicts.py: the row-major enumeration this one replaced
  const int r = t / NQ, q = t % NQ;
  if (kind == kST) return RowQuad{r < 4 ? 1 + 2 * r : (r == 4 ? 41 : (r == 5 ? 39 : (r == 6 ? 45 : 43))), q, 1};
  if (kind == kFT) return RowQuad{10 + 2 * r, q, 1};
  if (kind == kS1) return RowQuad{r == 0 ? 9 : 38, r == 0 ? q : (q + 4) % NQ, 1};
  return RowQuad{r < 6 ? 26 + 2 * r : 27 + 2 * (r - 6), q, 1};
#else
  return lane_rowquad(pass_segments(kind, t / 64), t % 64);
#endif
}

// How often the deal computes each row-quad: every lane's task of every dealt pass, counted by the rows it writes.
// (A deal that drops or doubles a pass, or a task enumeration that misses a quad, would still "run".)
struct DealCover { int n[NY * NQ]; };
template <bool STRICT>
__host__ __device__ constexpr DealCover deal_cover() {
  DealCover c{};
  for (int w = 0; w < 8; ++w)
    for (int i = 0; i < 3; ++i) {
      const Pass p = deal<STRICT>(w, i);
      if (p.kind == kNone) continue;
      for (int lane = 0; lane < 64; ++lane) {
        const RowQuad rq = task_rowquad(p.kind, 64 * p.index + lane);
        for (int j = 0; j < (rq.valid ? task_rows(p.kind) : 0); ++j) ++c.n[(rq.k + j) * NQ + rq.q];
      }
    }
  return c;
}
template <bool STRICT>
__host__ __device__ constexpr bool deal_is_complete() {
  for (int w = 0; w < 8; ++w)
    for (int i = 0; i < 3; ++i) {
      const Pass p = deal<STRICT>(w, i);
      if (is_polar_wave<STRICT>(w) && p.kind != kNone) return false;
      if (p.kind != kNone && (p.index < 0 || p.index >= kind_passes(p.kind))) return false; // a pass without tasks
    }
  const DealCover c = deal_cover<STRICT>();
  for (int k = 0; k < NY; ++k)
    for (int q = 0; q < NQ; ++q) if (c.n[k * NQ + q] != (k >= 1 && k <= NY - 2 ? 1 : 0)) return false;
  return true;
}
static_assert(deal_is_complete<true>() && deal_is_complete<false>(),
              "a deal must compute every row-quad of rows 1 .. 46 exactly once and give the polar waves no bulk pass");

// A lane's bulk task of one pass, fixed for the whole launch: float offsets (inside a guarded buffer) of its own
// pair-quad and of the quads to its left and right, and (row | quad << 8).  Computed once (make_tasks) and kept in
// VGPRs: recomputing them -- a division by 24, wrap-around selects and a dozen address adds -- cost ~15 % of a
// pass's issue slots in the sub-step loop.
struct TaskAddr { int c, l, r, kq; };
// the addresses of a task (make_tasks, and greb_member.hip: member_lds_table)
__host__ __device__ constexpr TaskAddr task_addr(const RowQuad& rq) {
  const int k = rq.k, q = rq.q;
  return TaskAddr{k * RS + 4 * q, k * RS + 4 * (q == 0 ? NQ - 1 : q - 1), k * RS + 4 * (q == NQ - 1 ? 0 : q + 1),
                  rq.valid ? (k | (q << 8)) : -1};
}
struct BulkTasks { TaskAddr t[3]; };

} // namespace greb
