// greb_member_bulk.h -- the bulk rows 1 .. 46 of the fused member kernel's sub-step: the arithmetic of one row task in
// either mode, and a wave's tasks as greb_member_deal.h deals them (make_tasks, make_signs, bulk_substep)
#pragma once

#include "greb_member_deal.h"
#include "greb_member_lds.h"

namespace greb {

// ---------------------------------------------------------------------------------------------
// one bulk task: pair-quad (k, q) -> X_new = (X + dX_diffuse) + dX_advec, both tracers
// ---------------------------------------------------------------------------------------------
// (TaskAddr, a lane's task of one pass: greb_member_deal.h; ld8p / st8p, a pair-quad at a float offset: greb_member_lds.h)

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

// FAST: the wind signs of a lane's tasks, [pass][row of the task], as lane masks in scalar registers (greb_pair.h: wind_term)
struct BulkSigns { WindSigns s[3][2]; };

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

} // namespace greb
