// greb_member.hip -- the fused GREB member engine for MI355X (gfx950, wave64), 96x48 grid.
//
// One 512-thread workgroup integrates one member-year CHUNK: a run of consecutive model steps of one ensemble member --
// the whole launch (one model year) where there are no more members than workgroups, else an item of the launch's ready
// queue (see "The deal of member-year chunks") -- point physics, 2 x 24 circulation sub-steps, Euler update, sea ice,
// monthly/annual accumulation (src/greb.f90:239-364, 528-553) without leaving the CU.
//
// Residency
//   LDS (157 KB)  X[2 buffers][48][96][{Tair,q}]  the two transported tracers, INTERLEAVED and
//                                                 double-buffered
//                 W[48][96][{wz_air,wz_vapor}]    the stencil weights (static for the run)
//                 WX, WY [48][96]                 this step's winds, scaled by the row's advection
//                                                 constants (FAST) or raw (STRICT and polar rows)
//                 row constants, Jacobi row buffers of the polar rows
//   HBM/L2        Tsurf, Tocean, cap_surf, accumulators, forcing: touched once per model step.  FAST reads the
//                 boundary data of the point physics from the set's packed forcing record (greb_kernels.h: static
//                 part + one slice per step, wind speed finished; made by pack_forcing_kernel below), STRICT from
//                 the raw arrays; the winds are staged from the raw uclim / vclim in both
//   Registers hold nothing across sub-steps.
//
// The tracer interleave makes every FAST arithmetic instruction a packed v_pk_*_f32 on an aligned
// (Tair,q) register pair (greb_pair.h): both tracers share the winds, their signs, the address
// arithmetic and the row constants.
//
// Work distribution per sub-step (measured on MI355X: the bulk is the critical path, bound by VALU issue on the
// busiest SIMD and by LDS bandwidth; a wave issues at most ~1 instruction per 4.5 cycles, a SIMD ~1 per 3):
//   a TASK works on pair-quads: 4 longitudes x (Tair,q) of one row, or of two vertically stacked rows that share
//   the six rows of their column (44 instead of 62 ds_read_b128).  The 46 non-polar rows are the "sub" family
//   (rows 1-9, 38-46: sub-cycled formulas, one sweep) and the "full" family (rows 10-37).  A PASS is 64 tasks of
//   one kind, one per lane; 3 passes of sub row-pairs, 3 of full row-pairs, 1 + 4.5 of single rows, in both arithmetic
//   modes; dealt statically to the seven (STRICT: six) bulk waves (see "The schedule") with each lane's task addresses
//   computed once per circulation call.  Which (row, quad) a lane of a pass holds follows the LDS's lane groups -- for a
//   ds_read_b128 the 16 lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, not 16 consecutive lanes --
//   so that the reads of a group fall on different banks (see RS and task_rowquad).
//   polar rows 0 / 47 (8 dependent Jacobi sweeps per diffusion call, src/greb.f90:656-717): FAST -- ONE wave, each
//   DPP row of 16 lanes x 6 longitudes one (pole, tracer) chain, neighbours by row rotates (quad_chain_substep);
//   STRICT -- one wave per pole, 48 lanes x 2 longitudes x (Tair,q), neighbours by ds_bpermute (chain_substep).
// One s_barrier per sub-step.
#include <cstdlib>

#include "greb_kernels.h"
#include "greb_pair.h"
#include "greb_physics_step.h"
#include "greb_stencil.h"

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
// LDS map, in floats
// X buffers and W carry one all-zero GUARD row below row 0 and above row NY-1: the rows k-2 .. k+2 of any bulk
// row are then five rows at constant strides from ONE base address (immediate offsets of the ds_read), and the
// missing neighbours of rows 1 and NY-2 multiply to zero without selects.
constexpr int XB = (NY + 2) * RS;   // floats per guarded buffer
constexpr int kOffX = RS;           // row 0 of X[0]; X[b] row k at kOffX + b*XB + k*RS
constexpr int kOffW = 2 * XB + RS;  // row 0 of W  [NY][NX][{wz_air,wz_vapor}]
constexpr int kOffWX = 3 * XB;      // [NP]  cu*u   (raw u in rows 0, 47 and in STRICT)
constexpr int kOffWY = kOffWX + NP; // [NP]  ccy/3*v (raw v ...)
constexpr int kOffRowK = kOffWY + NP; // [NY][kRowKWords]
constexpr int kRowKCsDif = 7;        // FAST: dif_cc/20 in the spare word of a row's constants (Circ::init)
constexpr int kLdsFloats = kOffRowK + NY * kRowKWords;
constexpr size_t kLdsBytes = (size_t)kLdsFloats * sizeof(float);

// rows 0-9 / 38-47 sub-cycled, only rows 0 and 47 iterate (default kappa +-25 %)
bool member_layout_supported(const RowTables& t, int nx, int ny) {
  if (nx != NX || ny != NY) return false;
  for (int k = 0; k < NY; ++k) {
    const bool sub = (k <= 9 || k >= 38);
    if ((t.subcycled[k] != 0) != sub) return false;
    const bool chain = (k == 0 || k == NY - 1);
    if ((t.dif_time2[k] > 1 || t.adv_time2[k] > 1) != chain) return false;
  }
  // the FAST engine runs both poles' chains in one wavefront with one (scalar) trip count; cos(-lat) = cos(lat)
  // makes the two rows' constants identical in the reference, so this never fails for its grid
  if (t.dif_time2[0] != t.dif_time2[NY - 1] || t.adv_time2[0] != t.adv_time2[NY - 1]) return false;
  return true;
}

// split a pair-quad into the two tracers' scalar quads (STRICT path)
__device__ __forceinline__ f4 comp(const q8& q, int tr) {
  return tr == 0 ? f4{{q.v[0].x, q.v[1].x, q.v[2].x, q.v[3].x}} : f4{{q.v[0].y, q.v[1].y, q.v[2].y, q.v[3].y}};
}
// interleave two fields' quads into one pair-quad
__device__ __forceinline__ q8 zip(const f4& a, const f4& b) {
  q8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.v[i] = v2{a.v[i], b.v[i]};
  return r;
}

// ---------------------------------------------------------------------------------------------
// one bulk task: pair-quad (k, q) -> X_new = (X + dX_diffuse) + dX_advec, both tracers
// ---------------------------------------------------------------------------------------------
// A lane's bulk task of one pass, fixed for the whole launch: float offsets (inside a guarded buffer) of its own
// pair-quad and of the quads to its left and right, and (row | quad << 8).  Computed once (make_tasks) and kept in
// VGPRs: recomputing them -- a division by 24, wrap-around selects and a dozen address adds -- cost ~15 % of a
// pass's issue slots in the sub-step loop.
struct TaskAddr { int c, l, r, kq; };

// a pair-quad at a float offset p (two dwordx4: the [half][quad][4] row layout of greb_pair.h)
__device__ __forceinline__ q8 ld8p(const lfloat* p) {
  const vfloat4 a = *(const __attribute__((address_space(3))) vfloat4*)p;
  const vfloat4 b = *(const __attribute__((address_space(3))) vfloat4*)(p + kHalfRow);
  q8 r;
  r.v[0] = v2{a.x, a.y}; r.v[1] = v2{a.z, a.w}; r.v[2] = v2{b.x, b.y}; r.v[3] = v2{b.z, b.w};
  return r;
}

// FAST arithmetic of one bulk row task from its loaded neighbourhood (shared by the one-row and the two-row task)
// ws: the signs of the eight winds, lane masks kept since the start of the circulation call (make_signs)
template <bool SUB>
__device__ __forceinline__ q8 fast_row(const q8& LT, const q8& CT, const q8& RT, const q8& Tm2, const q8& Tm1, const q8& Tp1,
                                       const q8& Tp2, const q8& LW, const q8& CW, const q8& RW, const q8& Wm2, const q8& Wm1,
                                       const q8& Wp1, const q8& Wp2, const f4& xq, const f4& yq, const WindSigns& ws,
                                       bool last_quad, float cs_dif, float dif_ccy, bool calm_q) {
  v2 T[12], w[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    T[j] = LT.v[j]; T[4 + j] = CT.v[j]; T[8 + j] = RT.v[j];
    w[j] = LW.v[j]; w[4 + j] = CW.v[j]; w[8 + j] = RW.v[j];
  }
  // (the latitudinal advection term is not divided by 3 at k = 1 (v>=0 part) and k = ny-2 (v<0 part), :766-769, :784-787:
  // stage_winds folds that factor into the staged v of rows 1 and NY-2, once per model step)
  // (the signs are shared by the two tracers)
  return substep_pair<SUB>(T, w, Tm2, Tm1, Tp1, Tp2, Wm2, Wm1, Wp1, Wp2, xq.v, ws.x, yq.v, ws.y, cs_dif, dif_ccy, last_quad, calm_q);
}

__device__ __forceinline__ void st8p(lfloat* o, const q8& xn) {
  vfloat4 a, b;
  a.x = xn.v[0].x; a.y = xn.v[0].y; a.z = xn.v[1].x; a.w = xn.v[1].y;
  b.x = xn.v[2].x; b.y = xn.v[2].y; b.z = xn.v[3].x; b.w = xn.v[3].y;
  *(__attribute__((address_space(3))) vfloat4*)o = a;
  *(__attribute__((address_space(3))) vfloat4*)(o + kHalfRow) = b;
}

// STRICT arithmetic of one bulk row task from its loaded neighbourhood: the reference's expression trees, both
// tracers packed -- with contraction off every v2 operation is the reference's IEEE operation on each half.  Raw winds.
__device__ __forceinline__ q8 strict_row(const q8& LT, const q8& CT, const q8& RT, const q8& Tm2, const q8& Tm1, const q8& Tp1,
                                         const q8& Tp2, const q8& LW, const q8& CW, const q8& RW, const q8& Wm2, const q8& Wm1,
                                         const q8& Wp1, const q8& Wp2, const f4& xq, const f4& yq, int k, int q,
                                         const RowK& rk, bool calm_q) {
#pragma clang fp contract(off)
  q8 xn;
  v2 T[12], w[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    T[j] = LT.v[j]; T[4 + j] = CT.v[j]; T[8 + j] = RT.v[j];
    w[j] = LW.v[j]; w[4 + j] = CW.v[j]; w[8 + j] = RW.v[j];
  }
  v2 dTx[4], dTy[4], dd[4], da[4];
  // diffusion (dif_quad<true>)
  dif_lon_strict(T, w, rk.dif_cc, dTx);
  if (rk.sub) {
    v2 T1h[4] = {T[4], T[5], T[6], T[7]};
    clamp_add(T1h, dTx);
#pragma unroll
    for (int i = 0; i < 4; ++i) dTx[i] = T1h[i] - T[4 + i]; // :718
  }
  dif_lat_strict(CT, Tm1, Tp1, Wm1, Wp1, rk.dif_ccy, k, NY, dTy);
#pragma unroll
  for (int i = 0; i < 4; ++i) dd[i] = CW.v[i] * (dTx[i] + dTy[i]); // :721
  // advection (adv_quad<true>), raw winds
  if (!rk.sub) {
    adv_lon_full_strict(T, w, xq.v, rk.adv_cc, dTx);
  } else {
    v2 T1h[4] = {T[4], T[5], T[6], T[7]};
    adv_lon_sub_strict(T, w, xq.v, rk.adv_cc, q == NQ - 1, dTx);
    clamp_add(T1h, dTx);
#pragma unroll
    for (int i = 0; i < 4; ++i) dTx[i] = T1h[i] - T[4 + i]; // :910
  }
  adv_lat_strict(CT, Tm2, Tm1, Tp1, Tp2, Wm2, Wm1, Wp1, Wp2, yq.v, rk.adv_ccy, k, NY, dTy);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    da[i] = dTx[i] + dTy[i];                       // :913
    const v2 xd = T[4 + i] + dd[i];
    v2 x = xd + da[i];                             // :549
    if (calm_q) x.y = xd.y;                        // orig :562: vapour diffused, not advected
    xn.v[i] = x;
  }
  return xn;
}

// the arithmetic of one row in either mode
template <bool STRICT, bool SUB>
__device__ __forceinline__ q8 one_row(const q8& LT, const q8& CT, const q8& RT, const q8& Tm2, const q8& Tm1, const q8& Tp1,
                                      const q8& Tp2, const q8& LW, const q8& CW, const q8& RW, const q8& Wm2, const q8& Wm1,
                                      const q8& Wp1, const q8& Wp2, const f4& xq, const f4& yq, const WindSigns& ws, int k, int q,
                                      const RowK& rk, bool calm_q) {
  if (STRICT) return strict_row(LT, CT, RT, Tm2, Tm1, Tp1, Tp2, LW, CW, RW, Wm2, Wm1, Wp1, Wp2, xq, yq, k, q, rk, calm_q);
  // FAST: rk.dif_cc holds the row's dif_cc/20 as Circ::init staged it (task_consts)
  return fast_row<SUB>(LT, CT, RT, Tm2, Tm1, Tp1, Tp2, LW, CW, RW, Wm2, Wm1, Wp1, Wp2, xq, yq, ws, q == NQ - 1, rk.dif_cc,
                       rk.dif_ccy, calm_q);
}

// the row constants a task needs: everything in STRICT; in FAST ONE word, the row's dif_cc/20 as Circ::init staged it
// (the advection constants are folded into the staged winds, and dif_ccy is the same in every row: the caller read it
// once per circulation call, role_loop) -- the full 32-byte read costs the FAST loop 3 %
template <bool STRICT>
__device__ __forceinline__ RowK task_consts(const lfloat* lds, int k, float ccy_dif) {
  if (STRICT) return row_consts((const lfloat*)(lds + kOffRowK), k);
  RowK rk{};
  rk.dif_cc = lds[kOffRowK + k * kRowKWords + kRowKCsDif];
  rk.dif_ccy = ccy_dif;
  return rk;
}

// One bulk row of one quad column.  The five rows k-2 .. k+2 of the column come from ONE base address (the guard
// rows make k-2 = -1 and k+2 = NY valid reads: zero weights in FAST, not referenced by the reference's boundary
// formulas in STRICT), the row's left and right quads from the two precomputed offsets.
template <bool STRICT, bool SUB>
__device__ __forceinline__ void row_task(lfloat* lds, int cur, const TaskAddr& ta, const WindSigns* ws, float ccy_dif,
                                         bool calm_q = false) {
  const int k = ta.kq & 255, q = ta.kq >> 8;
  const lfloat* Xc = lds + kOffX + cur * XB;
  const lfloat* Wc = lds + kOffW;
  const RowK rk = task_consts<STRICT>(lds, k, ccy_dif);
  const f4 xq = ld4(lds + kOffWX + k * NX + 4 * q), yq = ld4(lds + kOffWY + k * NX + 4 * q);
  const lfloat* xb = Xc + ta.c - 2 * RS;
  const lfloat* wb = Wc + ta.c - 2 * RS;
  const q8 Tm2 = ld8p(xb), Tm1 = ld8p(xb + RS), CT = ld8p(xb + 2 * RS), Tp1 = ld8p(xb + 3 * RS), Tp2 = ld8p(xb + 4 * RS);
  const q8 Wm2 = ld8p(wb), Wm1 = ld8p(wb + RS), CW = ld8p(wb + 2 * RS), Wp1 = ld8p(wb + 3 * RS), Wp2 = ld8p(wb + 4 * RS);
  const q8 LT = ld8p(Xc + ta.l), RT = ld8p(Xc + ta.r), LW = ld8p(Wc + ta.l), RW = ld8p(Wc + ta.r);
  const q8 xn = one_row<STRICT, SUB>(LT, CT, RT, Tm2, Tm1, Tp1, Tp2, LW, CW, RW, Wm2, Wm1, Wp1, Wp2, xq, yq, ws[0], k, q, rk,
                                     calm_q);
  st8p(lds + kOffX + (cur ^ 1) * XB + ta.c, xn); // own quad of the other buffer: same offset
}

// Two vertically adjacent bulk rows (k, k+1) of one quad column in one task: the six rows k-2 .. k+3 of the
// column are loaded once and shared -- 44 instead of 62 ds_read_b128 for the two rows.  The sub-step loop is
// co-limited by LDS bandwidth: dropping 39 % of the bulk reads (timing experiment) made it 12 % faster.
template <bool STRICT, bool SUB>
__device__ __forceinline__ void row_task2(lfloat* lds, int cur, const TaskAddr& ta, const WindSigns* ws, float ccy_dif,
                                          bool calm_q = false) {
  const int k = ta.kq & 255, q = ta.kq >> 8;
  const lfloat* Xc = lds + kOffX + cur * XB;
  const lfloat* Wc = lds + kOffW;
  const lfloat* xb = Xc + ta.c - 2 * RS;
  const lfloat* wb = Wc + ta.c - 2 * RS;
  const q8 T0 = ld8p(xb), T1 = ld8p(xb + RS), T2 = ld8p(xb + 2 * RS), T3 = ld8p(xb + 3 * RS), T4 = ld8p(xb + 4 * RS);
  const q8 W0 = ld8p(wb), W1 = ld8p(wb + RS), W2 = ld8p(wb + 2 * RS), W3 = ld8p(wb + 3 * RS), W4 = ld8p(wb + 4 * RS);
  lfloat* out = lds + kOffX + (cur ^ 1) * XB + ta.c;
  {
    const q8 LT = ld8p(Xc + ta.l), RT = ld8p(Xc + ta.r), LW = ld8p(Wc + ta.l), RW = ld8p(Wc + ta.r);
    const f4 xq = ld4(lds + kOffWX + k * NX + 4 * q), yq = ld4(lds + kOffWY + k * NX + 4 * q);
    const RowK rk = task_consts<STRICT>(lds, k, ccy_dif);
    st8p(out, one_row<STRICT, SUB>(LT, T2, RT, T0, T1, T3, T4, LW, W2, RW, W0, W1, W3, W4, xq, yq, ws[0], k, q, rk, calm_q));
  }
  __builtin_amdgcn_sched_barrier(0); // row k+1 after row k: keeps the two rows' temporaries from piling up
  {
    const q8 T5 = ld8p(xb + 5 * RS), W5 = ld8p(wb + 5 * RS); // row k+3: only the second row needs it
    const q8 LT = ld8p(Xc + ta.l + RS), RT = ld8p(Xc + ta.r + RS), LW = ld8p(Wc + ta.l + RS), RW = ld8p(Wc + ta.r + RS);
    const f4 xq = ld4(lds + kOffWX + (k + 1) * NX + 4 * q), yq = ld4(lds + kOffWY + (k + 1) * NX + 4 * q);
    const RowK rk = task_consts<STRICT>(lds, k + 1, ccy_dif);
    st8p(out + RS,
         one_row<STRICT, SUB>(LT, T3, RT, T1, T2, T4, T5, LW, W3, RW, W1, W2, W4, W5, xq, yq, ws[1], k + 1, q, rk, calm_q));
  }
}

struct BulkTasks { TaskAddr t[3]; };
// FAST: the wind signs of a lane's tasks, [pass][row of the task], as lane masks in scalar registers (greb_pair.h: wind_term)
struct BulkSigns { WindSigns s[3][2]; };

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
enum { kNone = 0, kS1 = 1, kF1 = 2, kST = 3, kFT = 4 };
struct Pass { int kind, index; };
// FAST: ONE wave runs all four polar chains (quad_chain_substep: 36-instruction sweeps, ~2 600 busy cycles per
// sub-step when it has the SIMD to itself, where two waves took ~4 400 each) and there are seven bulk waves.  The chain
// wave issues one instruction every ~5 cycles for as long as it runs; as the OLDER wave of its SIMD it leaves its
// partner little of the pipe until it is done, as the YOUNGER one (wave 6) it fills the slots its partner leaves and
// both finish together.  Measured sub-step times (tools/deal_search.py: in-kernel stamps, 512 members, one gpurun call
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

// host-visible form of the above (greb_member_deal_cover): counts[k * NQ + q], rows 0 .. NY-1
void member_deal_cover(bool strict, int* counts) {
  constexpr DealCover cs = deal_cover<true>(), cf = deal_cover<false>();
  for (int i = 0; i < NY * NQ; ++i) counts[i] = strict ? cs.n[i] : cf.n[i];
}

// the addresses of a task (make_tasks, and the table below)
__host__ __device__ constexpr TaskAddr task_addr(const RowQuad& rq) {
  const int k = rq.k, q = rq.q;
  return TaskAddr{k * RS + 4 * q, k * RS + 4 * (q == 0 ? NQ - 1 : q - 1), k * RS + 4 * (q == NQ - 1 ? 0 : q + 1),
                  rq.valid ? (k | (q << 8)) : -1};
}

// The LDS traffic of the bulk waves in one sub-step, for tools/lds_conflicts.py (greb_member_lds_table): one record of
// kLdsRecInts ints per lane of every LDS instruction of every dealt pass -- wave, the wave's pass slot, the instruction's
// number within the pass, lane, kind of access (kLds*), bytes per lane, float offset into the workgroup's LDS or -1 for a
// lane without a task.  The offsets are those of row_task / row_task2 reading buffer 0 and storing to buffer 1, from the
// deal, the enumeration and the LDS map above; the chain wave(s) of the polar rows are not in it.
enum { kLdsCol = 0, kLdsSide = 1, kLdsWind = 2, kLdsStore = 3, kLdsConst = 4, kLdsRecInts = 7 };
// ... and the map they point into: the row stride and where X[0], X[1], W (each with its two guard rows), WX, WY and the
// row constants begin and the last ends, in floats
void member_lds_map(int* words8) {
  const int m[8] = {RS, 0, XB, 2 * XB, kOffWX, kOffWY, kOffRowK, kLdsFloats};
  for (int i = 0; i < 8; ++i) words8[i] = m[i];
}
int member_lds_table(bool strict, int* out, int capacity) {
  int n = 0;
  for (int w = 0; w < 8; ++w)
    for (int i = 0; i < 3; ++i) {
      const Pass p = strict ? deal_strict(w, i) : deal_fast(w, i);
      const int rows = task_rows(p.kind);
      if (rows == 0) continue;
      int instr = 0;
      // one instruction: lane -> ta.c / ta.l / ta.r (which = 0 / 1 / 2) + off, or a wind / constant address of row k + j
      auto emit = [&](int kind, int bytes, int base, int which, int off, int j) {
        for (int lane = 0; lane < 64; ++lane, ++n) {
          if (n >= capacity) continue;
          const RowQuad rq = task_rowquad(p.kind, 64 * p.index + lane);
          const TaskAddr ta = task_addr(rq);
          const int k = (ta.kq & 255) + j, q = ta.kq >> 8;
          int a = base + off + (which == 0 ? ta.c : (which == 1 ? ta.l : ta.r));
          if (kind == kLdsWind) a = base + k * NX + 4 * q;
          if (kind == kLdsConst) a = base + k * kRowKWords + off;
          const int rec[kLdsRecInts] = {w, i, instr, lane, kind, bytes, rq.valid ? a : -1};
          for (int x = 0; x < kLdsRecInts; ++x) out[(size_t)n * kLdsRecInts + x] = rec[x];
        }
        ++instr;
      };
      auto pairquad = [&](int kind, int base, int which, int off) { // ld8p / st8p: two 16-byte accesses
        emit(kind, 16, base, which, off, 0);
        emit(kind, 16, base, which, off + kHalfRow, 0);
      };
      for (int base : {kOffX, kOffW}) // the column: rows k-2 .. k+2 (two stacked rows: .. k+3)
        for (int j = -2; j <= 1 + rows; ++j) pairquad(kLdsCol, base, 0, j * RS);
      for (int j = 0; j < rows; ++j) {
        for (int base : {kOffX, kOffW}) { pairquad(kLdsSide, base, 1, j * RS); pairquad(kLdsSide, base, 2, j * RS); }
        emit(kLdsWind, 16, kOffWX, 0, 0, j);
        emit(kLdsWind, 16, kOffWY, 0, 0, j);
        if (strict) { emit(kLdsConst, 16, kOffRowK, 0, 0, j); emit(kLdsConst, 16, kOffRowK, 0, 4, j); } // row_consts
        else emit(kLdsConst, 4, kOffRowK, 0, kRowKCsDif, j);                                             // task_consts
        pairquad(kLdsStore, kOffX + XB, 0, j * RS);
      }
    }
  return n;
}

// once per launch; the asm makes the values opaque, so the compiler keeps them instead of re-deriving them from
// the lane id inside the sub-step loop
template <bool STRICT, int WAVE>
__device__ __forceinline__ BulkTasks make_tasks(int lane) {
  __builtin_assume(lane >= 0 && lane < 64);
  BulkTasks b;
  static_for<3>([&](auto I) {
    constexpr int i = I;
    constexpr Pass p = deal<STRICT>(WAVE, i);
#if defined(GREB_TUNING) && defined(GREB_TASKS_ROW_MAJOR)
    const RowQuad rq = task_rowquad(p.kind, p.index * 64 + lane);
#else
    constexpr PassSegments ps = pass_segments(p.kind, p.index);
    constexpr int ntask = pass_tasks(p.kind, p.index);
    RowQuad rq{1, 0, 0};
    if constexpr (ntask > 0) {
      rq = lane_rowquad(ps, lane);
      if (ntask < 64 && lane >= ntask) rq = RowQuad{1, 0, 0};
    }
#endif
    TaskAddr a = task_addr(rq);
    asm volatile("" : "+v"(a.c), "+v"(a.l), "+v"(a.r), "+v"(a.kq));
    b.t[i] = a;
  });
  return b;
}

// Once per circulation call -- that is once per model step in every kernel, beside make_tasks at the top of role_loop, after
// stage_winds and the barrier behind it; nothing of this lives across a step: every lane of the wave compares the staged winds of its
// task rows with zero and the wave keeps the outcome as 64-bit lane masks, 16 scalar registers per task row.  The winds do
// not change until the next stage_winds, and a lane's tasks are fixed.  Lanes without a task in a partial pass read row 1,
// quad 0.
template <int WAVE>
__device__ __forceinline__ void make_signs(const lfloat* lds, const BulkTasks& tasks, BulkSigns& b) {
  static_for<3>([&](auto I) {
    constexpr int i = I, rows = task_rows(deal_fast(WAVE, i).kind);
    if constexpr (rows > 0) {
      const int kq = tasks.t[i].kq < 0 ? 1 : tasks.t[i].kq, k = kq & 255, q = kq >> 8;
#pragma unroll
      for (int j = 0; j < rows; ++j) {
        const f4 xq = ld4(lds + kOffWX + (k + j) * NX + 4 * q), yq = ld4(lds + kOffWY + (k + j) * NX + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned long long mx = __builtin_amdgcn_ballot_w64(xq.v[e] > 0.f), my = __builtin_amdgcn_ballot_w64(yq.v[e] > 0.f);
          asm volatile("" : "+s"(mx), "+s"(my)); // opaque: kept, not re-derived from the winds inside the sub-step loop
          b.s[i][j].x[e] = mx; b.s[i][j].y[e] = my;
        }
      }
    }
  });
}

// task i of bulk wave SLOT: kind and pass are compile-time, so a wave's sub-step is straight-line code -- no
// per-sub-step dispatch on the wave number (that dispatch, a switch on a VGPR lowered to exec-mask bookkeeping, cost
// every bulk wave ~100 issue slots per sub-step)
template <bool STRICT, int SLOT, int I>
__device__ __forceinline__ void bulk_task(lfloat* lds, int cur, const BulkTasks& tasks, const BulkSigns& signs, float ccy_dif,
                                          int dbg, bool calm_q) {
  constexpr int kind = deal<STRICT>(SLOT, I).kind, ntask = pass_tasks(kind, deal<STRICT>(SLOT, I).index);
  if constexpr (kind != kNone && ntask > 0) {
    if (ntask < 64 && tasks.t[I].kq < 0) return; // partial pass: lanes without a task
    if constexpr (kind == kS1) { if (!(dbg & 1)) row_task<STRICT, true>(lds, cur, tasks.t[I], signs.s[I], ccy_dif, calm_q); }
    else if constexpr (kind == kF1) { if (!(dbg & 2)) row_task<STRICT, false>(lds, cur, tasks.t[I], signs.s[I], ccy_dif, calm_q); }
    else if constexpr (kind == kST) { if (!(dbg & 1)) row_task2<STRICT, true>(lds, cur, tasks.t[I], signs.s[I], ccy_dif, calm_q); }
    else { if (!(dbg & 2)) row_task2<STRICT, false>(lds, cur, tasks.t[I], signs.s[I], ccy_dif, calm_q); }
  }
}
template <bool STRICT, int SLOT>
__device__ __forceinline__ void bulk_substep(lfloat* lds, int cur, const BulkTasks& tasks, const BulkSigns& signs, float ccy_dif,
                                             int dbg, bool calm_q = false) {
  bulk_task<STRICT, SLOT, 0>(lds, cur, tasks, signs, ccy_dif, dbg, calm_q);
  bulk_task<STRICT, SLOT, 1>(lds, cur, tasks, signs, ccy_dif, dbg, calm_q);
  bulk_task<STRICT, SLOT, 2>(lds, cur, tasks, signs, ccy_dif, dbg, calm_q);
}

// ---------------------------------------------------------------------------------------------
// polar rows, STRICT: one wave per pole, 48 lanes x 2 longitudes x (Tair,q), the reference's expression trees
// ---------------------------------------------------------------------------------------------
// float offset, inside a [half][quad][4] row, of the longitude pair (2l, 2l+1)
__device__ __forceinline__ int pair_off(int l) { return (l & 1) * kHalfRow + (l >> 1) * 4; }
__device__ __forceinline__ void load_win10(const lfloat* row, int l, v2 t[10]) {
  // lanes l-2 .. l+2 (mod 48) -> longitudes 2l-4 .. 2l+5
  const int lm2 = l >= 2 ? l - 2 : l + 46, lm1 = l >= 1 ? l - 1 : 47, lp1 = l <= 46 ? l + 1 : 0, lp2 = l <= 45 ? l + 2 : l - 46;
  const int idx[5] = {lm2, lm1, l, lp1, lp2};
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const vfloat4 a = *(const __attribute__((address_space(3))) vfloat4*)(row + pair_off(idx[i]));
    t[2 * i] = v2{a.x, a.y}; t[2 * i + 1] = v2{a.z, a.w};
  }
}
__device__ __forceinline__ void st_pair2(lfloat* p, v2 a, v2 b) {
  vfloat4 x; x.x = a.x; x.y = a.y; x.z = b.x; x.w = b.y;
  *(__attribute__((address_space(3))) vfloat4*)p = x;
}

__device__ __forceinline__ void chain_substep_strict(lfloat* lds, int cur, int pole, int l /* lane */, bool calm_q = false) {
  if (l >= 48) return; // idle lanes (no workgroup barrier inside this function)
  const int k = pole ? NY - 1 : 0;
  const RowK rk = row_consts((const lfloat*)(lds + kOffRowK), k);
  const lfloat* Xc = lds + kOffX + cur * XB;
  const lfloat* Wc = lds + kOffW;
  v2 T0w[10], w[10];
  load_win10(Xc + k * RS, l, T0w);
  load_win10(Wc + k * RS, l, w);
  const float u0 = lds[kOffWX + k * NX + 2 * l], u1 = lds[kOffWX + k * NX + 2 * l + 1]; // raw winds
  const float v0 = lds[kOffWY + k * NX + 2 * l], v1 = lds[kOffWY + k * NX + 2 * l + 1];
  const int k1 = pole ? k - 1 : k + 1, k2 = pole ? k - 2 : k + 2; // towards the interior
  v2 T1[2], T2[2], W1[2], W2[2];
  {
    const vfloat4 a = *(const __attribute__((address_space(3))) vfloat4*)(Xc + k1 * RS + pair_off(l));
    const vfloat4 b = *(const __attribute__((address_space(3))) vfloat4*)(Xc + k2 * RS + pair_off(l));
    const vfloat4 c = *(const __attribute__((address_space(3))) vfloat4*)(Wc + k1 * RS + pair_off(l));
    const vfloat4 d = *(const __attribute__((address_space(3))) vfloat4*)(Wc + k2 * RS + pair_off(l));
    T1[0] = v2{a.x, a.y}; T1[1] = v2{a.z, a.w}; T2[0] = v2{b.x, b.y}; T2[1] = v2{b.z, b.w};
    W1[0] = v2{c.x, c.y}; W1[1] = v2{c.z, c.w}; W2[0] = v2{d.x, d.y}; W2[1] = v2{d.z, d.w};
  }
  const v2 own[2] = {T0w[4], T0w[5]};
  const bool bug_lane = (l == 46); // its 2nd point is longitude xdim-2 (1-based), :881
  // Between two Jacobi sweeps a lane needs the new values of lanes l-2 .. l+2 (mod 48).  They travel by
  // ds_bpermute_b32 -- lane to lane through the LDS crossbar, no memory, no bank conflicts, ONE hop -- instead of a
  // ds_write + s_waitcnt + ds_read round trip through a row buffer behind the bulk waves' read traffic.  The chain
  // of 8 dependent sweeps is the floor of a sub-step: 4 700 busy cycles per sub-step with the row buffers, 4 100 so.
  const int am2 = 4 * (l >= 2 ? l - 2 : l + 46), am1 = 4 * (l >= 1 ? l - 1 : 47), ap1 = 4 * (l <= 46 ? l + 1 : 0),
            ap2 = 4 * (l <= 45 ? l + 2 : l - 46);
  auto from = [](int addr, v2 x) {
    return v2{__int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x.x))),
              __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x.y)))};
  };
  const float uu[2] = {u0, u1};

  v2 Th[2][2]; // [diffusion, advection][point]
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    // the row constants come from LDS (per lane) but are the same in every lane: a scalar trip count keeps the
    // sweep loop free of exec-mask bookkeeping
    const int time2 = __builtin_amdgcn_readfirstlane(which ? rk.adv_time2 : rk.dif_time2);
    const float cc = which ? rk.adv_cc : rk.dif_cc;
    v2 T[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) T[i] = T0w[i];
    v2 th[2] = {own[0], own[1]};
    for (int tt = 0; tt < time2; ++tt) {
      if (tt > 0) { // T[0] and T[9] are not referenced by either stencil
        T[1] = from(am2, th[1]); T[2] = from(am1, th[0]); T[3] = from(am1, th[1]);
        T[4] = th[0]; T[5] = th[1];
        T[6] = from(ap1, th[0]); T[7] = from(ap1, th[1]); T[8] = from(ap2, th[0]);
      }
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
#pragma clang fp contract(off)
        const int c = 4 + pt;
        v2 dd;
        if (which) dd = adv_lon_sub_point_strict(T, w, uu[pt], cc, c, bug_lane && pt == 1);
        else dd = div20(cc * dif_S_strict(T, w, c));
        dd = clamp_e(dd, T[c]); // :715 / :907
        th[pt] = T[c] + dd;
      }
    }
    Th[which][0] = th[0]; Th[which][1] = th[1];
  }

  // ---- latitudinal terms + update (:585-590, :756-795, :721, :913, :549)
  v2 xn[2];
  const float vv[2] = {v0, v1};
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
#pragma clang fp contract(off)
    const v2 t0 = own[pt], w0 = w[4 + pt], a1 = T1[pt], a2 = T2[pt], b1 = W1[pt], b2 = W2[pt];
    const float vm = split_m(vv[pt]), vp = split_p(vv[pt]);
    v2 dTy, aTy;
    if (pole == 0) {
      dTy = rk.dif_ccy * b1 * (-t0 + a1);                                        // :589
      aTy = div3(rk.adv_ccy * (vp * (b1 * (t0 - a1) + b2 * (t0 - a2))));         // :759-761
    } else {
      dTy = rk.dif_ccy * b1 * (a1 - t0);                                         // :590
      aTy = div3(rk.adv_ccy * (-vm * (b1 * (t0 - a1) + b2 * (t0 - a2))));        // :792-794
    }
    const v2 dd = w0 * ((Th[0][pt] - t0) + dTy); // :718, :721
    const v2 da = (Th[1][pt] - t0) + aTy;        // :910, :913
    const v2 xd = t0 + dd;
    v2 x = xd + da;                              // :549
    if (calm_q) x.y = xd.y;                      // orig :562
    xn[pt] = x;
  }
  st_pair2(lds + kOffX + (cur ^ 1) * XB + k * RS + pair_off(l), xn[0], xn[1]);
}

// ---------------------------------------------------------------------------------------------
// FAST polar rows: all four chains -- (pole, tracer) -- in ONE wave
// ---------------------------------------------------------------------------------------------
// A DPP row of 16 lanes x 6 points is one 96-point latitude circle whose periodic boundary is the row rotate
// (row_ror:1 / row_ror:15), so the four rows of a wavefront hold the four polar chains of a member: lanes 0-15
// (south pole, Tair), 16-31 (south, q), 32-47 (north, Tair), 48-63 (north, q).  The sweeps are greb_chain6.h's
// (36 instructions for all four chains; the earlier form -- one wave per pole, 48 lanes x 2 points x (Tair,q), halos
// by 12 ds_bpermute per sweep -- needed ~45 per pole and waited for the LDS crossbar in every one of the 9 sweeps:
// 4 400 busy cycles per sub-step on two waves, now ~2 100 on one).  The coefficients of the diffusion chain are fixed
// for the run and those of the advection sweep for the model step; both are rebuilt per circulation call so that
// nothing of this lives across the point-physics phase.
struct QuadChain {
  ChainK kd, ka;             // d[i] = sum_m K[i][m] e[i+m] (greb_chain6.h): zonal diffusion, zonal advection
  float w0[6], W1[6], W2[6]; // weights of the own row and of the two rows towards the interior
  float own[6];              // the lane's points: loaded once per circulation call, then carried from sub-step to sub-step
  float cv[6];               // the latitudinal advection coefficient of the point: (ccy/3) min(v,0) south, -(ccy/3) max(v,0) north
  float ccy;                 // dif_ccy
  int at[3];                 // float offsets, within a row, of the lane's three longitude pairs (+ its tracer)
  int row[3];                // float offsets, within a guarded buffer, of rows k, k1, k2
  int time2_dif, time2_adv;
  bool calm;                 // vapour lane of an experiment that diffuses vapour without advecting it
};

__device__ __forceinline__ void quad_chain_setup(const lfloat* lds, int cur, int lane, bool calm_q, QuadChain& c) {
  const int r = lane >> 4, j = lane & 15, pole = r >> 1, C = r & 1;
  const int k = pole ? NY - 1 : 0, k1 = pole ? k - 1 : k + 1, k2 = pole ? k - 2 : k + 2; // towards the interior
  const RowK rk = row_consts((const lfloat*)(lds + kOffRowK), k);
  c.time2_dif = rk.dif_time2; c.time2_adv = rk.adv_time2; c.ccy = rk.dif_ccy;
  c.calm = calm_q && C == 1;
  c.row[0] = k * RS; c.row[1] = k1 * RS; c.row[2] = k2 * RS;
#pragma unroll
  for (int t = 0; t < 3; ++t) c.at[t] = pair_off(3 * j + t) + C;
  const lfloat* Wc = lds + kOffW;
  // (static_for: compile-time indices from the start -- arrays indexed by the variable of a `#pragma unroll` loop are
  // still dynamically indexed when the compiler decides what may live in registers)
  float w[12]; // longitudes 6j-3 .. 6j+8
  static_for<12>([&](auto I) {
    constexpr int i = I;
    int x = 6 * j - 3 + i;
    x = x < 0 ? x + NX : (x >= NX ? x - NX : x);
    w[i] = Wc[c.row[0] + pair_off(x >> 1) + (x & 1) * 2 + C];
  });
  const float third = rk.adv_ccy * (1.f / 3.f), csd = rk.dif_cc * 0.05f, csa = rk.adv_cc * 0.05f;
  float Kd[6][6], Ka[6][6];
  static_for<6>([&](auto I) {
    constexpr int i = I, p = 3 + i;
    const int o = c.at[i >> 1] + (i & 1) * 2;
    c.w0[i] = w[p];
    c.own[i] = lds[kOffX + cur * XB + c.row[0] + o];
    c.W1[i] = Wc[c.row[1] + o];
    c.W2[i] = Wc[c.row[2] + o];
    const float u = lds[kOffWX + k * NX + 6 * j + i], v = lds[kOffWY + k * NX + 6 * j + i]; // raw winds in the polar rows
    // south pole: only the v<0 part couples (rows 1,2); north pole: only the v>=0 part (rows 46,45)  (:759-761, :792-794)
    c.cv[i] = pole == 0 ? third * fminf(v, 0.f) : -third * fmaxf(v, 0.f);
    // 6(Pp[c] - Pm[c-1]) + 3(Pp[c+1] - Pm[c-2]) + (Pp[c+2] - Pm[c-3]), :595-600 in edge-flux form
    Kd[i][0] = -csd * w[p - 3]; Kd[i][1] = (-3.f * csd) * w[p - 2]; Kd[i][2] = (-6.f * csd) * w[p - 1];
    Kd[i][3] = (6.f * csd) * w[p + 1]; Kd[i][4] = (3.f * csd) * w[p + 2]; Kd[i][5] = csd * w[p + 3];
    // -up (10 Pp[c] + 4 Pp[c+1] + Pp[c+2]) - um (10 Pm[c-1] + 4 Pm[c-2] + Pm[c-3]), :845-851
    const float um = csa * fmaxf(u, 0.f), up = csa * fminf(u, 0.f);
    Ka[i][0] = -um * w[p - 3]; Ka[i][1] = (-4.f * um) * w[p - 2]; Ka[i][2] = (-10.f * um) * w[p - 1];
    Ka[i][3] = (-10.f * up) * w[p + 1]; Ka[i][4] = (-4.f * up) * w[p + 2]; Ka[i][5] = -up * w[p + 3];
    if (i == 3 && j == 15) { // longitude xdim-2 (1-based), :881: the 4* term vanishes, the 1* term is w(1)*(T(xdim-1)-T(1))
      Ka[i][4] = -up * w[p + 3]; Ka[i][5] = -up * w[p + 3];
    }
  });
  c.kd = chain_pack(Kd);
  c.ka = chain_pack(Ka);
}

__device__ __forceinline__ void quad_chain_substep(lfloat* lds, int cur, QuadChain& c) {
  const lfloat* Xc = lds + kOffX + cur * XB;
  // (the own row is this wave's alone: what it stored last sub-step is what it would read now, so the chain starts
  // without an LDS round trip; the neighbour rows are requested here and not needed before the epilogue)
  float own[6], T1[6], T2[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int o = c.at[i >> 1] + (i & 1) * 2;
    own[i] = c.own[i];
    T1[i] = Xc[c.row[1] + o];
    T2[i] = Xc[c.row[2] + o];
  }
  float Td[6], Ta[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) { Td[i] = own[i]; Ta[i] = own[i]; }
  chain_run6<true>(Td, c.kd, c.time2_dif); // :656-717
  chain_run6<true>(Ta, c.ka, c.time2_adv); // :861-909 (one sweep at this grid)
  // ---- latitudinal terms + update (:585-590, :756-795, :721, :913, :549)
  lfloat* out = lds + kOffX + (cur ^ 1) * XB + c.row[0];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const float g1 = c.W1[i] * (T1[i] - own[i]);
    const float d2 = c.W2[i] * (own[i] - T2[i]);
    const float ddy = c.ccy * g1;
    const float day = c.cv[i] * (d2 - g1);
    const float dd = c.w0[i] * ((Td[i] - own[i]) + ddy);
    float da = (Ta[i] - own[i]) + day;
    if (c.calm) da = 0.f; // orig :562
    c.own[i] = (own[i] + dd) + da;
    out[c.at[i >> 1] + (i & 1) * 2] = c.own[i];
  }
}

// stage this step's winds (src/greb.f90:203-216, 732): raw for STRICT and for the polar rows,
// otherwise scaled by the row's advection constants, so that a row task multiplies by the staged wind alone:
//   x = c*u, c = ccx/3 (full rows) or ccx2/20 (sub-cycled rows);  y = ccy/3 * v (rows 1 and NY-2: see below)
// REMAT (the switch-aware FAST kernels, whose sub-step loop exists twice): the thread's addresses are derived anew every
// model step -- a few instructions -- instead of living in registers across the sub-steps, where that kernel has none left.
template <bool STRICT, bool REMAT = false>
__device__ __forceinline__ void stage_winds(lfloat* lds, const float* __restrict__ u, const float* __restrict__ v,
                                            const RowTables* __restrict__ tab) {
  int tid0 = threadIdx.x;
  if (REMAT) asm volatile("" : "+v"(tid0));
  // All of a thread's wind quads are requested before the first is waited for (unconditional loads at clamped
  // indices, predicated stores): as a plain load-scale-store loop the three iterations were three dependent round
  // trips, 2 700 cycles per model step.  The row's constants come from the LDS copy staged at init.
  constexpr int kIt = (NP / 4 + kThreads - 1) / kThreads;
  f4 uq[kIt], vq[kIt];
#pragma unroll
  for (int j = 0; j < kIt; ++j) {
    const int i = min(tid0 + j * kThreads, NP / 4 - 1);
    uq[j] = ld4(u + 4 * i); vq[j] = ld4(v + 4 * i);
  }
#pragma unroll
  for (int j = 0; j < kIt; ++j) {
    const int i = tid0 + j * kThreads;
    if (i < NP / 4) {
      const int k = i / NQ;
      if (!(STRICT || k == 0 || k == NY - 1)) {
        const RowK rk = row_consts((const lfloat*)(lds + kOffRowK), k);
        const float cu = rk.sub ? rk.adv_cc * 0.05f : rk.adv_cc * (1.f / 3.f);
        const float cv = rk.adv_ccy * (1.f / 3.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) { uq[j].v[e] *= cu; vq[j].v[e] *= cv; }
        // The latitudinal advection term is not divided by 3 for the v>=0 part of row 1 and the v<0 part of row NY-2
        // (:766-769, :784-787).  The factor 3 goes onto that part of the staged wind here, once per model step, instead
        // of onto the split halves in every sub-cycled row task: with y' = 3y where y has the part's sign and y' = y
        // elsewhere, max(y',0) and y' - max(y',0) are the bits of 3 max(y,0) and y - max(y,0) (row 1), or of max(y,0)
        // and 3 (y - max(y,0)) (row NY-2); the product still feeds a multiply, so no contraction changes either.  (The
        // row tasks no longer form the two parts: wind_term selects by the sign of y', which is the sign of y.)
        if (k == 1 || k == NY - 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float y = vq[j].v[e];
            vq[j].v[e] = (k == 1 ? y > 0.f : y < 0.f) ? 3.f * y : y;
          }
        }
      }
      st4(lds + kOffWX + 4 * i, uq[j]); st4(lds + kOffWY + 4 * i, vq[j]);
    }
  }
  (void)tab;
}

// the circulation loop shared by the member kernel and its test mirror
template <bool STRICT>
struct Circ {
  __device__ __forceinline__ void init(lfloat* lds, const float* wz_air, const float* wz_vapor,
                                       const RowTables* __restrict__ tab) {
    // The thread id as a value of this call: the member kernel runs its prologue once per (member, chunk) item, and
    // addresses made from threadIdx.x itself are made once in front of that loop and then held -- spilled -- across the
    // whole body.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    // guard rows of X[0], X[1], W: zero, never written again
    for (int i = tid; i < 6 * RS; i += kThreads) {
      const int g = i / RS, o = i % RS; // buffer g >> 1, lower / upper guard g & 1
      lds[(g >> 1) * XB + (g & 1) * (NY + 1) * RS + o] = 0.f;
    }
    stage_row_consts(lds + kOffRowK, *tab, 0, NY, tid);
    // FAST: the diffusion constant as the bulk tasks use it, dif_cc/20, in the row's spare word -- the same single fp32
    // multiply the tasks did (each thread rescales the rows it has just staged: LDS operations of a thread stay in order)
    if (!STRICT)
      for (int k = tid; k < NY; k += blockDim.x)
        lds[kOffRowK + k * kRowKWords + kRowKCsDif] = lds[kOffRowK + k * kRowKWords] * 0.05f;
    for (int i = tid; i < NP / 4; i += kThreads)
      st8(lds + kOffW + (i / NQ) * RS, i % NQ, zip(ld4(wz_air + 4 * i), ld4(wz_vapor + 4 * i)));
  }

  // One wave's share of `nsub` sub-steps, one s_barrier after each (every wave of the workgroup executes the same
  // number of barriers, each in its own loop).  WAVE is compile-time: the loop body is the wave's own straight-line
  // task sequence.  dbg: timing experiments only (tools/microbench_circ.py): bit0/1/2 skip sub / full / chain work.
  // NOT_CALM: the caller knows calm_q to be false (see substeps): the loop is then compiled as the default instantiation
  // compiles it.
  template <int WAVE, bool NOT_CALM>
  __device__ __forceinline__ void role_loop(lfloat* lds, int cur, int nsub, int lane, int dbg, bool calm_runtime
#ifdef GREB_TUNING
                                            , bool stamp, unsigned long long& busy
#endif
  ) {
    const bool calm_q = NOT_CALM ? false : calm_runtime;
    // the lane's task addresses: derived once per circulation call (not per launch -- values that live across the
    // point-physics phase, where the register pressure peaks, come back as scratch reloads inside this loop)
    constexpr bool kPolar = is_polar_wave<STRICT>(WAVE);
    BulkTasks tasks;
    BulkSigns signs;
    QuadChain quad;
    if constexpr (!kPolar) tasks = make_tasks<STRICT, WAVE>(lane);
    else if constexpr (!STRICT) quad_chain_setup(lds, cur, lane, calm_q, quad);
    if constexpr (!kPolar && !STRICT) make_signs<WAVE>(lds, tasks, signs);
    // FAST bulk waves: dif_ccy, the one row constant that is the same in every row, as a scalar for the whole call
    float ccy_dif = 0.f;
    if constexpr (!kPolar && !STRICT) ccy_dif = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lds[kOffRowK + 2])));
#pragma unroll 1
    for (int tt = 0; tt < nsub; ++tt) {
#ifdef GREB_TUNING
      const unsigned long long t0 = stamp ? __builtin_amdgcn_s_memtime() : 0;
#endif
      if constexpr (kPolar && STRICT) { if (!(dbg & 4)) chain_substep_strict(lds, cur, WAVE - 2, lane, calm_q); }
      else if constexpr (kPolar) { if (!(dbg & 4)) quad_chain_substep(lds, cur, quad); }
      else bulk_substep<STRICT, WAVE>(lds, cur, tasks, signs, ccy_dif, dbg, calm_q);
#ifdef GREB_TUNING
      if (stamp) busy += __builtin_amdgcn_s_memtime() - t0;
#endif
      __syncthreads();
      cur ^= 1;
    }
  }
  // `nsub` sub-steps starting from buffer `cur`; the caller continues with buffer cur ^ (nsub & 1)
  __device__ __forceinline__ void substeps(lfloat* lds, int cur, int nsub, int dbg = 0, bool calm_q = false
#ifdef GREB_TUNING
                                           , bool stamp = false, unsigned long long* busy = nullptr
#endif
  ) {
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane)); // opaque: nothing derived from it is hoisted out of the model-step loop
    // FAST: a launch whose member does not have the vapour-diffusion-only switch takes a copy of the loop in which calm_q
    // is the constant false.  With the switch as a run-time select inside the update (greb_pair.h: da.y = 0) the compiler
    // fuses the multiply-adds around it differently, and a member WITHOUT switches in a switch-aware launch then differs
    // in the last bits from the same member in the default instantiation; so, the two are the same code.  (STRICT has no
    // contraction: one loop.)
#ifdef GREB_TUNING
    unsigned long long b = 0;
#define GREB_ROLE(W) case W: if (!STRICT && !calm_q) role_loop<W, true>(lds, cur, nsub, lane, dbg, false, stamp, b); \
                             else role_loop<W, false>(lds, cur, nsub, lane, dbg, calm_q, stamp, b); break;
#else
#define GREB_ROLE(W) case W: if (!STRICT && !calm_q) role_loop<W, true>(lds, cur, nsub, lane, dbg, false); \
                             else role_loop<W, false>(lds, cur, nsub, lane, dbg, calm_q); break;
#endif
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) { // a scalar branch per circulation call
      GREB_ROLE(0) GREB_ROLE(1) GREB_ROLE(2) GREB_ROLE(3) GREB_ROLE(4) GREB_ROLE(5) GREB_ROLE(6) GREB_ROLE(7)
    }
#undef GREB_ROLE
#ifdef GREB_TUNING
    if (busy) *busy += b;
#endif
  }
};

// ---------------------------------------------------------------------------------------------
// test mirror of circulation() (src/greb.f90:528-553): one field per workgroup; the field is
// loaded into both tracer slots so the engine's code path is exercised unchanged
// ---------------------------------------------------------------------------------------------
template <bool STRICT>
__global__ __launch_bounds__(kThreads) void circulation_g96_kernel(const float* __restrict__ Xin,
                                                                   const float* __restrict__ wz,
                                                                   const float* __restrict__ ug,
                                                                   const float* __restrict__ vg,
                                                                   float* __restrict__ dX,
                                                                   const RowTables* __restrict__ tab, int nsub,
                                                                   int dbg) {
  extern __shared__ __align__(16) float lds_raw[];
  lfloat* lds = (lfloat*)lds_raw;
  const size_t fo = (size_t)blockIdx.x * NP;
  Circ<STRICT> c;
  c.init(lds, wz + fo, wz + fo, tab);
  for (int i = threadIdx.x; i < NP / 4; i += kThreads) {
    const f4 x = ld4(Xin + fo + 4 * i);
    st8(lds + kOffX + (i / NQ) * RS, i % NQ, zip(x, x));
  }
  __syncthreads(); // stage_winds reads the row constants init() staged
  stage_winds<STRICT>(lds, ug + fo, vg + fo, tab);
  __syncthreads();
  c.substeps(lds, 0, nsub, dbg);
  const int cur = nsub & 1;
  for (int i = threadIdx.x; i < NP / 4; i += kThreads) {
    const f4 a = comp(ld8(lds + kOffX + cur * XB + (i / NQ) * RS, i % NQ), 0), b = ld4(Xin + fo + 4 * i);
    st4(dX + fo + 4 * i, f4{{a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2], a.v[3] - b.v[3]}}); // :551
  }
}

hipError_t launch_circulation_g96(const float* X, const float* wz, const float* u, const float* v, float* dX,
                                  const RowTables* tab_dev, int batch, int nsub, bool strict, hipStream_t s) {
  auto kern = strict ? circulation_g96_kernel<true> : circulation_g96_kernel<false>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(batch), dim3(kThreads), kLdsBytes, s, X, wz, u, v, dX, tab_dev, nsub,
                     tuning_int("GREB_DEBUG_SKIP", 0)); // -DGREB_TUNING builds only
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// the member kernel
// ---------------------------------------------------------------------------------------------
// V: the variant (greb_kernels.h: which exist, which are legal, which one a launch takes); a variant contains nothing of a
// feature it does not name.  What each feature means here:
// kVExp: the member's switch word (a.xsw, or a.xsw_m[m] where the members of a launch differ) is read once
// and is block-uniform: it drives the point physics, the vapour-diffusion-only form of the sub-steps and the member's OWN
// sub-step count -- a member without circulation does none while its neighbours do 24 (every wave of a workgroup runs the
// same count, so the barriers inside Circ::substeps stay matched).
// kVBudget: the monthly means of the step's thirteen flux terms go out beside the five standard records (a pass of their own).
// kVForce: the member's CO2 pattern, insolation table and scale act in the point physics (greb_physics_step.h: member_force).
// Its words are read anew every model step, into scalar registers, so that nothing of it lives across the sub-steps.
// kVBound: the thirteen boundary fields are those of the member's set.  Only the set index, one scalar register, lives
// across the sub-steps: the pointers are fetched from the set table where they are used (greb_physics_step.h:
// member_boundary), as the other variants fetch theirs from the kernel arguments.
//
// The deal of member-year chunks.  A launch of more members than workgroups (MemberArgs::queue set) cuts every member's
// steps into the chunks of MemberArgs::chunks and deals (member, chunk) items to the workgroups from a ready queue: a CU
// that is done early -- the CUs' clocks differ by several per cent -- takes the next item instead of idling until the
// slowest CU has finished its last whole member, and an ensemble that is no multiple of the CU count does not pay a whole
// round for its remainder.  Everything a member carries from step to step is in global memory after every step (state,
// acc, corr, the budget sums) and the step's clock follows from it0 + s, so a chunk is the launch's body run for the steps
// [s0, s1) of member m: prologue (Circ::init, the tracers from `state`), step loop, nothing else.
// The queue: `q_capacity` = members x chunks item words behind a head and a tail counter, re-made on the stream before
// every launch with chunk 0 of every member in the first `members` slots.  A workgroup takes the next INDEX (atomic add on
// head), leaves when that is beyond the capacity, else waits until the slot is filled; having run the chunk it pushes the
// member's next one (atomic add on tail, store of the item).  A slot below the capacity is always filled in the end: by
// the image, or by a workgroup that holds an item and is therefore running -- nothing depends on which workgroups are
// resident or in what order they start.  The wait is bounded all the same (kCircSpinTicks); a workgroup that gives up sets
// q_status, which ends every other wait, and the host reports it (greb_engine.cpp: finish_years).
// A member's next chunk usually runs on another XCD, whose L2 may hold lines of that member from an earlier chunk: the
// push is a release at agent scope behind a workgroup barrier, the pop an acquire at agent scope in front of the first
// load of the member's data.  Only scalars (m, s0, s1) depend on the item.
constexpr int kLdsItemWord = kLdsFloats; // behind the map above
constexpr size_t kLdsBytesLaunch = kLdsBytes + 16;
static_assert(kLdsBytesLaunch <= 160 * 1024, "the item word must fit the CU's LDS beside the member");

__device__ __forceinline__ int item_member(unsigned item) { return (int)((item - 1u) >> 4); }
__device__ __forceinline__ int item_chunk(unsigned item) { return (int)((item - 1u) & 15u); }
__device__ __forceinline__ __attribute__((address_space(3))) unsigned* item_words(lfloat* lds) {
  return (__attribute__((address_space(3))) unsigned*)(lds + kLdsItemWord);
}
// word i of the two, block-uniform, read anew wherever it is used
__device__ __forceinline__ unsigned item_word(lfloat* lds, int i) {
  return (unsigned)__builtin_amdgcn_readfirstlane((int)*(volatile __attribute__((address_space(3))) unsigned*)(item_words(lds) + i));
}
// the next item of this workgroup, in every thread (block-uniform); 0: none -- the queue is drained, or the wait was given up
__device__ __forceinline__ unsigned pop_item(const MemberArgs& a, lfloat* lds) {
  __attribute__((address_space(3))) unsigned* word = item_words(lds) + 2; // (a word of its own: see member_kernel on the other two)
  if (threadIdx.x == 0) {
    unsigned item = 0u;
    const unsigned idx = __hip_atomic_fetch_add(a.queue + kQHead, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (idx < a.q_capacity) {
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        item = __hip_atomic_load(a.queue + kQItems + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (item != 0u) break;
        if (__hip_atomic_load(a.q_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break; // somebody gave up
        if (__builtin_amdgcn_s_memrealtime() - t0 > kCircSpinTicks) {
          __hip_atomic_store(a.q_status + 1, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(a.q_status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        __builtin_amdgcn_s_sleep(64); // ~4 000 cycles between two polls
      }
    }
    *word = item;
  }
  __syncthreads(); // (the word is not written again before every thread has passed the barrier behind the prologue)
  const unsigned item = (unsigned)__builtin_amdgcn_readfirstlane((int)*word);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return item;
}

// after the last step of a chunk: hand the member on
__device__ __forceinline__ void push_next(const MemberArgs& a, unsigned item) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // every wave's stores of the chunk ...
  __syncthreads();
  if (threadIdx.x == 0 && item_chunk(item) + 1 < a.chunks.n) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // ... in front of the item
    const unsigned slot = __hip_atomic_fetch_add(a.queue + kQTail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot < a.q_capacity) // (item + 1: the same member's next chunk)
      __hip_atomic_store(a.queue + kQItems + slot, item + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool STRICT, unsigned V>
__global__ __launch_bounds__(kThreads) void member_kernel(MemberArgs a_launch) {
  constexpr bool FLUX = V & kVFlux, EXP = V & kVExp, BUDGET = V & kVBudget, FORCE = V & kVForce, BOUND = V & kVBound;
  extern __shared__ __align__(16) float lds_raw[];
  lfloat* lds = (lfloat*)lds_raw;
  const int tid = threadIdx.x;
  const bool dealt = a_launch.queue != nullptr;
#pragma unroll 1
  for (;;) { // one (member, chunk) item per trip; a launch that is not dealt makes one trip
  // The kernel arguments of a trip, through a pointer that is opaque to the compiler: read through the parameter itself,
  // every argument the body uses is loaded once in front of this loop and held in a scalar register for the whole launch
  // (they are loop-invariant), across the sub-steps too -- 50 more scalar registers spilled and, in their wake, scratch.
  const __attribute__((address_space(4))) MemberArgs* a_trip =
      (const __attribute__((address_space(4))) MemberArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a_trip));
  const MemberArgs& a = *(const MemberArgs*)a_trip;
  // The item and the step its chunk ends at live in two LDS words: the step loop reads its bound there once per model step,
  // and what follows the loop reads the item again, so that neither holds a scalar register across the sub-steps.
  int m = blockIdx.x, s0 = 0;
  {
    int s1 = a.nsteps;
    unsigned item = ((unsigned)m << 4) + 1u;
    if (dealt) {
      item = pop_item(a, lds);
      if (item == 0u) break;
      m = item_member(item);
#pragma unroll
      for (int c = 0; c < kMaxChunks; ++c) { // (constant indices: the kernel arguments stay where they are)
        if (c + 1 == item_chunk(item)) s0 = a.chunks.end[c];
        if (c == item_chunk(item)) s1 = a.chunks.end[c];
      }
    }
    if (tid == 0) { item_words(lds)[0] = item; item_words(lds)[1] = (unsigned)s1; } // read behind the prologue's barrier
  }
#ifdef GREB_TUNING
  const unsigned long long tl_r0 = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0, tl_c0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
#endif
  float* state = a.state + (size_t)m * 5 * NP;
  float* acc = a.acc + (size_t)m * 6 * NP;
  float* corr = a.corr + (size_t)a.corr_index[m] * 3 * kNT * NP;
  const RowTables* tab = a.tabs + a.tab_index[m];

#ifdef GREB_TUNING
  // timing experiment (GREB_DEBUG_PHYS >> 8 = units of 1024 cycles): workgroup b starts (b mod 8) units late, so that
  // the point-physics phases of the CUs -- the only memory traffic of a step -- do not coincide
  for (int i = 0; i < (a.dbg >> 8) * (m & 7); ++i) __builtin_amdgcn_s_sleep(16);
#endif
  Circ<STRICT> circ;
  const int bset = member_bset<BOUND>(a, m);
  {
    const BoundPtr B = member_boundary<BOUND>(a, bset);
    circ.init(lds, BOUND ? (const float*)B->wz_air : a.wz_air, BOUND ? (const float*)B->wz_vapor : a.wz_vapor, tab);
  }
  {
    int t = tid;
    asm volatile("" : "+v"(t)); // (as in Circ::init)
    for (int i = t; i < NP / 4; i += kThreads)
      st8(lds + kOffX + (i / NQ) * RS, i % NQ, zip(ld4(state + NP + 4 * i), ld4(state + 3 * NP + 4 * i))); // (Tair, q)
  }
  int cur = 0;
  const unsigned xsw = EXP ? member_switches(a, m) : 0u;
  const int nsub = (EXP && (xsw & kXNoCirc)) ? 0 : a.nsub;
  // vapour diffused but not advected (orig :560-564) -- unless its transport is off altogether (:554-555 come first): the
  // increment is then dropped in the point physics, and the sub-steps run as they do without the switch, so that Tair, which
  // shares the FAST loop with q, has the bits it has under NO_VAPOR_TRANSPORT alone (Circ::substeps on the two loops)
  const bool q_dif_only = EXP && (xsw & kXQDiffOnly) && !(xsw & kXNoQTransport);
  // the flux-phase CO2 (:104) may be the member's own; read here, so that the step loop reads nothing new
  const float co2_flux = FLUX ? (a.co2_flux_m ? a.co2_flux_m[m] : a.co2_flux) : 0.f;
  __syncthreads();
#ifdef GREB_TUNING
  // diagnostic stamps (tools/stamp_member.py): shader-clock cycles this wave spent in each phase of the launch, its
  // busy time inside the sub-steps (barrier release -> arrival at the next barrier) and the launch's wall time in
  // s_memrealtime ticks (100 MHz) -- in-kernel clock = cycles / ticks x 100 MHz
  const bool stamp = a.stamps != nullptr;
  unsigned long long st_wind = 0, st_circ = 0, st_busy = 0, st_phys = 0;
  const unsigned long long st_c0 = stamp ? __builtin_amdgcn_s_memtime() : 0, st_r0 = stamp ? __builtin_amdgcn_s_memrealtime() : 0;
#define GREB_STAMP(var) const unsigned long long var = stamp ? __builtin_amdgcn_s_memtime() : 0
#else
#define GREB_STAMP(var)
#endif

#pragma unroll 1
  for (int s = s0; s < (int)item_word(lds, 1); ++s) {
    const long long it = a.it0 + s;
    const StepClock ck = step_clock<FLUX>(a, it, NP);
    const int ityr = ck.ityr, yr_rel = ck.yr_rel;
    const size_t off = ck.off;

    GREB_STAMP(t_a);
    {
      const BoundPtr B = member_boundary<BOUND>(a, bset);
      stage_winds<STRICT, EXP && !STRICT>(lds, (BOUND ? (const float*)B->uclim : a.uclim) + off,
                                          (BOUND ? (const float*)B->vclim : a.vclim) + off, tab);
    }
    __syncthreads();
    GREB_STAMP(t_b);

    // ---- circulation of Tair and q: 24 sub-steps (:543-550)
#ifdef GREB_TUNING
    circ.substeps(lds, cur, nsub, 0, q_dif_only, stamp, &st_busy);
#else
    circ.substeps(lds, cur, nsub, 0, q_dif_only);
#endif
    cur ^= nsub & 1;
    GREB_STAMP(t_c);

    // ---- point physics on the OLD state + Euler update (:254-268 / :328-361)
    const Phys P = a.phys[m];
    const float co2 = FLUX ? co2_flux : a.co2[(size_t)m * a.co2_stride + a.co2_year0 + yr_rel]; // :924
    const MemberForce mf = member_force<FORCE>(a, m, ck);
    const BoundPtr B = member_boundary<BOUND>(a, bset);
    // FAST: boundary data from the set's forcing record, everything else by scalar base + one 32-bit offset per quad
    constexpr int ROUTE = STRICT ? kRouteArrays : kRouteRecord;
    const float* rec = nullptr;
    if constexpr (!STRICT) rec = member_record(a, bset);
    lfloat* Xf = lds + kOffX + cur * XB;       // the tracers after the 24 sub-steps
    lfloat* red = lds + kOffX + (cur ^ 1) * XB; // idle buffer: annual-mean reduction scratch
    // Each thread takes whole quads (4 consecutive longitudes): every load/store of the ~26
    // fields a point touches is one dwordx4 and all of a quad's loads are in flight together.
    // 1152 quads on 512 threads: two full passes and a quarter-full one.  Measured with the stamp build
    // (GREB_DEBUG_PHYS): the first pass of a step costs 13 400 cycles, the other two together 12 500 -- the phase is
    // VALU-bound (1 170 instructions per quad) plus a cold start of ~5 000 cycles; giving the last 512 points to
    // all threads as single points (a second code path) measured 38 700 cycles against 25 900; the per-member operands of
    // the next pass requested one pass ahead (56 more live VGPRs): 37 100; warm-up loads for the phase's 28 arrays
    // issued under the sub-steps: no change; the next step's winds fetched before the phase and stored after it (24 live
    // VGPRs, wind staging 2 600 -> 250 cycles): the phase itself 35 000.  I-cache misses are nil (SQC_ICACHE_MISSES 41
    // per member-year).  What the slower variants share: vector-memory operations retire in order, so the loop's waits
    // for its loads also wait for the previous pass's stores; in the form below the compiler gets away with
    // s_waitcnt vmcnt(6) where the variants end up at vmcnt(0).  (All A/B runs in one gpurun call: boxes differ.)
    // Also measured: the next quad's operands requested BETWEEN the arithmetic of the current quad and its stores
    // (physics_load / physics_compute / physics_store, the inputs dead by then): 116 + 56 live VGPRs of operands and
    // results still spill 68 registers at the 256 cap, and the phase takes 41 600 cycles instead of 24 900.
    // BUDGET: a pass of its own over the step's quads BEFORE the update pass, while the old state and the transported
    // tracers are still in place: it evaluates the physics functions once more and only accumulates (the state outputs,
    // the corrections and the monthly sums of physics_load / physics_compute are dead here and compiled out).  Adding the
    // thirteen terms inside the update pass -- each by its own load, add and store, as the any-grid kernel does -- spills
    // 19 (EXP: 37) VGPRs of the FAST kernel to scratch at the 256 cap; in this form it has none.  A thread takes the
    // same quads in both passes, so the two need no barrier between them.
    if constexpr (BUDGET) {
      const BudgetSink bs = budget_sink<true>(a, m, ck);
#pragma unroll 1
      for (int qd = tid; qd < NP / 4; qd += kThreads) {
        const q8 xpair = ld8(Xf + (qd / NQ) * RS, qd % NQ);
        const PhysIn in = physics_load<V, ROUTE>(a, qd, ck, state, acc, corr, xsw, mf, B, rec);
        (void)physics_compute<STRICT, V | kVBudget, ROUTE>(a, P, in, co2, comp(xpair, 0), comp(xpair, 1), xsw, bs, 4 * qd, mf);
      }
    }
#pragma unroll 1
    for (int qd = tid; qd < NP / 4; qd += kThreads) {
#ifdef GREB_TUNING
      if ((a.dbg & 4) && qd >= kThreads) break; // timing experiment: one pass of the three
#endif
      const q8 xpair = ld8(Xf + (qd / NQ) * RS, qd % NQ);
      f4 oTa, oq, tsm;
      physics_quad<STRICT, V & ~kVBudget, ROUTE>(a, P, m, qd, ck, co2, state, acc, corr, comp(xpair, 0), comp(xpair, 1), oTa, oq, tsm, xsw, mf, B, rec);
      st8(Xf + (qd / NQ) * RS, qd % NQ, zip(oTa, oq));
      if (ityr == kNT) st4(red + 4 * qd, tsm);
    }
    if (ityr == kNT) {
      __syncthreads();
      if (STRICT) {
        if (tid == 0 && a.yearly) {
#pragma clang fp contract(off)
          float sum = 0.f; // the reference's sum() lowers to a sequential fp32 loop; same order here
          for (int i = 0; i < NP; ++i) sum += red[i];
          float* y = a.yearly + ((size_t)m * a.yearly_years + (a.yearly_year0 + yr_rel)) * 2;
          y[0] = sum / (float)NP - 273.15f;                                               // :954
          y[1] = red[(a.ipy - 1) * NX + (a.ipx - 1)] - 273.15f;
        }
      } else if (a.yearly) { // FAST: per-lane partial sums, wavefront shuffle reduction, 8 wave totals through LDS
        int t0 = tid;
        if (EXP) asm volatile("" : "+v"(t0)); // (as in stage_winds: the address is not kept across the year's sub-steps)
        float part = 0.f;
        for (int i = t0; i < NP; i += kThreads) part += red[i];
        part = wave_sum(part);
        const float point = red[(a.ipy - 1) * NX + (a.ipx - 1)];
        __syncthreads(); // everyone has read red[]; its first words now carry the wave totals
        if ((tid & 63) == 0) red[tid >> 6] = part;
        __syncthreads();
        if (tid == 0) {
          float sum = 0.f;
          for (int w = 0; w < kThreads / 64; ++w) sum += red[w];
          float* y = a.yearly + ((size_t)m * a.yearly_years + (a.yearly_year0 + yr_rel)) * 2;
          y[0] = sum / (float)NP - 273.15f;                                               // :954
          y[1] = point - 273.15f;
        }
      }
    }
    __syncthreads();
#ifdef GREB_TUNING
    if (stamp) {
      const unsigned long long t_d = __builtin_amdgcn_s_memtime();
      st_wind += t_b - t_a; st_circ += t_c - t_b; st_phys += t_d - t_c;
    }
#endif
  }
#ifdef GREB_TUNING
  if (stamp && (tid & 63) == 0) {
    unsigned long long* o = a.stamps + ((size_t)m * (kThreads / 64) + (tid >> 6)) * 8;
    o[0] = __builtin_amdgcn_s_memtime() - st_c0; o[1] = __builtin_amdgcn_s_memrealtime() - st_r0;
    o[2] = st_wind; o[3] = st_circ; o[4] = st_busy; o[5] = st_phys; o[6] = (unsigned long long)((int)item_word(lds, 1) - s0); o[7] = (unsigned long long)nsub;
  }
  // ... and the item's lifetime (tools/stamp_member.py tail): behind the wave records, per (member, chunk), start and end in
  // s_memrealtime ticks, the XCC and hardware ids, shader cycles of the whole item and of its prologue, its steps
  if (stamp && tid == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const int chunk = item_chunk(item_word(lds, 0));
    unsigned long long* o = a.stamps + (size_t)a.stamp_members * (kThreads / 64) * 8 + ((size_t)m * kMaxChunks + chunk) * 8;
    o[0] = tl_r0; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = ((unsigned long long)xcc << 32) | hw;
    o[3] = __builtin_amdgcn_s_memtime() - tl_c0; o[4] = st_c0 - tl_c0; o[5] = (unsigned long long)s0; o[6] = (unsigned long long)item_word(lds, 1);
    o[7] = (unsigned long long)blockIdx.x;
  }
#endif
  // all five state fields were written back every step
  if (!dealt) break;
  push_next(a, item_word(lds, 0)); // (behind the step loop's closing barrier: every thread's stores of this chunk are issued)
  }
}

// The forcing record of one boundary set (greb_kernels.h): one thread per (step, point).  The wind-speed term is
// wind_speed<false>, the expression hydro<false> evaluates: the bits are those the member kernel used to compute itself.
static_assert(kFrNx == NX && kFrNy == NY, "the forcing record is the fused kernel's grid");
__global__ __launch_bounds__(256) void pack_forcing_kernel(BoundarySet b, float* __restrict__ rec) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)kNT * NP) return;
  const unsigned step = i / NP, p = i - step * NP, row = p / NX, lon = p - row * NX;
  const unsigned prev = step > 0 ? step - 1 : kNT - 1; // StepClock::offm
  const float zt = b.z_topo[p];
  if (step == 0) { // the static part, in front
    float* o = rec + forcing_record_offset((int)row, 0, (int)lon);
    o[forcing_record_offset(0, kFrZtopo, 0)] = zt;
    o[forcing_record_offset(0, kFrGlacier, 0)] = b.glacier[p];
    o[forcing_record_offset(0, kFrZocean, 0)] = b.z_ocean[p];
    o[forcing_record_offset(0, kFrWzAir, 0)] = b.wz_air[p];
  }
  float* o = rec + kFrStaticFloats + (size_t)step * kFrStepFloats + forcing_record_offset((int)row, kFrStaticFields, (int)lon);
  o[forcing_record_offset(0, kFrTclim, 0)] = b.tclim[i];
  o[forcing_record_offset(0, kFrCld, 0)] = b.cldclim[i];
  o[forcing_record_offset(0, kFrMld, 0)] = b.mldclim[i];
  o[forcing_record_offset(0, kFrMldPrev, 0)] = b.mldclim[(size_t)prev * NP + p];
  o[forcing_record_offset(0, kFrSwet, 0)] = b.swetclim[i];
  o[forcing_record_offset(0, kFrWind, 0)] = wind_speed<false>(b.uclim[i], b.vclim[i], zt);
}

hipError_t launch_pack_forcing(const BoundarySet& b, float* rec, hipStream_t s) {
  hipLaunchKernelGGL(pack_forcing_kernel, dim3((kNT * NP + 255) / 256), dim3(256), 0, s, b, rec);
  return hipGetLastError();
}

template <bool STRICT, unsigned V>
struct MemberFamily { static auto kernel() { return &member_kernel<STRICT, V>; } };

// workgroups: those of a dealt launch (a.queue set, made for n_members members by the caller); ignored otherwise
hipError_t launch_member_kernel(const MemberArgs& a, int n_members, bool strict, hipStream_t s, int workgroups) {
  if (a.nx != NX || a.ny != NY) return hipErrorInvalidValue;
  if (a.queue && (workgroups < 1 || !a.q_status || a.chunks.n < 1 || a.chunks.n > kMaxChunks || n_members > kMaxDealtMembers ||
                  a.q_capacity != (unsigned)n_members * (unsigned)a.chunks.n || a.chunks.end[a.chunks.n - 1] != a.nsteps))
    return hipErrorInvalidValue;
  if (!strict && !a.bsets) return hipErrorInvalidValue; // the FAST kernels read their forcing record behind the set table
  unsigned v;
  if (hipError_t e = select_variant(a, &v); e != hipSuccess) return e;
  const auto kern = pick_variant<MemberFamily>(strict, v);
  if (!kern) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytesLaunch);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.queue ? workgroups : n_members), dim3(kThreads), kLdsBytesLaunch, s, a);
  return hipGetLastError();
}

} // namespace greb
