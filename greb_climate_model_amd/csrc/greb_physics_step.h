// greb_physics_step.h -- one model step of point physics + Euler update + accumulation for one
// quad (4 consecutive longitudes) of one member (src/greb.f90:254-268 scenario, :328-361 flux
// correction, :945 / :974-984 accumulation).  Shared by the fused 96x48 member kernel (tracers in
// LDS) and the any-grid multi-launch engine (tracers in HBM): the caller supplies the tracers after
// the 24 circulation sub-steps (xTa, xq) and stores the new ones (oTa, oq).
#pragma once
#include "greb_kernels.h"

namespace greb {

__device__ __constant__ int kMonthEnd[12] = {31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334, 365};
__device__ __constant__ int kMonthDays[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31}; // :42

struct StepClock {
  int ityr, mon, yr_rel; // step in year (1-based), month ending today (0-based) or -1, years since launch start
  size_t off, offm;      // offsets of climatology slices ityr and ityr-1 (:507-508)
};
template <bool FLUX>
__device__ __forceinline__ StepClock step_clock(const MemberArgs& a, long long it, int np) {
  StepClock c;
  c.ityr = (int)((it - 1) % kNT) + 1;               // :252
  const int jday = (int)(((it - 1) / 2) % 365) + 1; // :251
  c.off = (size_t)(c.ityr - 1) * np;
  c.offm = (size_t)(c.ityr > 1 ? c.ityr - 2 : kNT - 1) * np;
  c.yr_rel = (int)((it - 1) / kNT - (a.it0 - 1) / kNT);
  c.mon = -1;
  if (!FLUX && (it % 2 == 0))
    for (int mm = 0; mm < 12; ++mm) if (jday == kMonthEnd[mm]) c.mon = mm; // :975-976
  return c;
}

// The experiment switches of member m (block-uniform): its own word where the launch carries one per member, else the
// launch's.
__device__ __forceinline__ unsigned member_switches(const MemberArgs& a, int m) {
  return (unsigned)__builtin_amdgcn_readfirstlane((int)(a.xsw_m ? a.xsw_m[m] : a.xsw));
}

// Per-member forcing (kVForce variants, scenario phase only; greb_engine_set_member_forcing): the member's four words
// and what they select from the engine's shared tables, for one model step.  Everything here is block-uniform and read
// once per step into scalar registers -- nothing of it lives across the circulation sub-steps; what is per point is the
// pattern's weight quad (PhysIn::fw) and the three operations of forced_co2.  The same launches carry prescribed SST
// (greb_engine_set_member_sst): the member's two words and its pattern's season factor are read here likewise; what is per
// point is done in prescribe_sst.  And stochastic heat flux (greb_engine_set_member_noise): the member's four words, its
// pattern's season factor and cell words and the step's hold block (`it`: the scenario clock, 1-based) are read here; the
// Philox state of a quad lives and dies in physics_load (noise_quad).
struct MemberForce {
  const float* space; // the member's CO2 pattern [np]; null: none, CO2 is the member's scalar
  const float* solar; // the member's insolation table [730][ny] (the engine's own where the member names none)
  float season;       // the pattern's seasonal factor of this step
  float ref, scale;   // CO2 where the weight is 0; factor on the insolation
  // prescribed SST (greb_engine_set_member_sst): what the member's ocean surface is held to in this step
  const float* sst_anom;   // the member's anomaly pattern [np]; null: the ocean surface is free
  const float* sst_weight; // its nudging weights [np]; null: 1 everywhere
  float sst_season, sst_amp; // the pattern's seasonal factor of this step; the member's amplitude
  // stochastic heat flux (greb_engine_set_member_noise, greb_noise.h): what the member's TF of this step is raised by
  NoiseStep noise;           // noise.sigma null: the member takes no noise
};
__device__ __forceinline__ float uniform_f(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
template <bool FORCE>
__device__ __forceinline__ MemberForce member_force(const MemberArgs& a, int m, const StepClock& ck, long long it) {
  MemberForce f{nullptr, a.sw_solar, 1.f, 0.f, 1.f, nullptr, nullptr, 1.f, 0.f, NoiseStep{}};
  if (FORCE && a.noise_m) { // (a member without a pattern: this one scalar test per step)
    const MemberNoise w = a.noise_m[m];
    if (__builtin_amdgcn_readfirstlane(w.pattern) >= 0)
      f.noise = noise_step(w, a.n_sigma, a.n_season, a.n_cells, a.np, a.ny, ck.ityr, (unsigned long long)(it - 1));
  }
  if (FORCE && a.sst_m) { // (a member without a pattern: this one scalar test per step)
    const MemberSst w = a.sst_m[m];
    const int k = __builtin_amdgcn_readfirstlane(w.pattern);
    if (k >= 0) {
      f.sst_anom = a.s_anom + (size_t)k * a.np;
      if (a.s_weight) f.sst_weight = a.s_weight + (size_t)k * a.np;
      f.sst_season = uniform_f(a.s_season[(size_t)k * kNT + (ck.ityr - 1)]);
      f.sst_amp = uniform_f(w.amp);
    }
  }
  if (FORCE) {
    const MemberForcing w = a.force_m[m];
    const int k = __builtin_amdgcn_readfirstlane(w.co2_pattern), t = __builtin_amdgcn_readfirstlane(w.solar_table);
    f.ref = uniform_f(w.co2_ref); f.scale = uniform_f(w.solar_scale);
    if (k >= 0) {
      f.space = a.f_space + (size_t)k * a.np;
      f.season = uniform_f(a.f_season[(size_t)k * kNT + (ck.ityr - 1)]);
    }
    if (t >= 0) f.solar = a.f_solar + (size_t)t * kNT * a.ny;
  }
  return f;
}
// CO2 of one point under a pattern: the lerp whose ends are exact -- weight 1 gives co2 bit for bit, weight 0 gives ref
__device__ __forceinline__ float forced_co2(const MemberForce& f, float w_space, float co2) {
#pragma clang fp contract(off)
  const float w = w_space * f.season;
  const float part = w * co2;
  const float rest = (1.f - w) * f.ref;
  return part + rest;
}

// Prescribed SST of one quad (kVForce variants, scenario phase only; include/greb_engine.h: "prescribed SST"): the ocean
// points (zt < 0) of Ts are blended towards tclp + anom * season * amp by the weight w -- the lerp of forced_co2, whose ends
// are exact: w = 1 gives the target bit for bit, w = 0 leaves Ts.  Without a weight table the target itself is taken, which
// is what the lerp gives at w = 1.  plus1: the member also has GREB_X_SST_PLUS1, which acts first (greb.original.model.f90:226)
// -- it is applied HERE for a prescribed member, and physics_compute leaves it alone.  Called from physics_load, where Ts,
// zt and tclp are in hand: the anomaly and weight quads die here, PhysIn gains nothing that lives into physics_compute.
__device__ __forceinline__ void prescribe_sst(const MemberForce& F, bool plus1, const f4& zt, const f4& tclp, const f4& anom, const f4& w,
                                              f4& Ts) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float t = Ts.v[e];
    if (plus1) t = tclp.v[e] + 1.0f;
    const float a = (anom.v[e] * F.sst_season) * F.sst_amp;
    const float target = tclp.v[e] + a;
    if (F.sst_weight) {
      const float part = w.v[e] * target;
      const float rest = (1.f - w.v[e]) * t;
      t = part + rest;
    } else t = target;
    if (zt.v[e] < 0.0f) Ts.v[e] = t;
  }
}

// one fp32 add per element, never contracted with what made its operands
__device__ __forceinline__ f4 add4_exact(const f4& a, const f4& b) {
#pragma clang fp contract(off)
  f4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r.v[e] = a.v[e] + b.v[e];
  return r;
}

// Boundary sets (kVBound variants, both phases; greb_engine_set_member_boundary): the member's entry of the set table.
// The set index is block-uniform and read once into a scalar register; the entry's pointers are fetched where they are
// used, by scalar loads through a constant-address-space pointer -- as the default kernels fetch theirs from the kernel
// arguments -- so that none of the thirteen lives across the circulation sub-steps.  member_boundary makes the entry's
// address opaque at every call: loads through it stay behind the call.
typedef const BoundarySet __attribute__((address_space(4)))* BoundPtr;
template <bool BOUND>
__device__ __forceinline__ int member_bset(const MemberArgs& a, int m) {
  return BOUND ? __builtin_amdgcn_readfirstlane(a.bset_m[m]) : 0;
}
template <bool BOUND>
__device__ __forceinline__ BoundPtr member_boundary(const MemberArgs& a, int bset) {
  unsigned long long p = 0;
  if (BOUND) {
    p = (unsigned long long)(a.bsets + bset);
    asm volatile("" : "+s"(p));
  }
  return (BoundPtr)p;
}
// field `f` of the member's set, or the launch's own
#define GREB_BF(f) (BOUND ? (const float*)B->f : a.f)

// Where a quad's operands come from (a compile-time route of physics_load / physics_compute / physics_store, not a variant):
// kRouteArrays: one base pointer per array, any grid (the STRICT member kernel and the any-grid kernels);
// kRouteRecord: the FAST fused 96x48 member kernel -- boundary data from the set's forcing record (greb_kernels.h), the
// wind-speed term finished; everything else by a scalar base plus ONE opaque 32-bit byte offset per quad, so that every
// access takes the scalar-base form and no 64-bit address lives across the quad's arithmetic.
enum { kRouteArrays, kRouteRecord };
// the record of the member's set (bset: 0 without kVBound), fetched from the set table where it is used, as
// member_boundary fetches the set's pointers: one scalar load per model step, nothing of it lives across the sub-steps
__device__ __forceinline__ const float* member_record(const MemberArgs& a, int bset) {
  unsigned long long p = (unsigned long long)((const float* const*)(a.bsets + kSetTableEntries) + bset);
  asm volatile("" : "+s"(p));
  return *(const float* const __attribute__((address_space(4)))*)p;
}
// base + byte offset, the offset opaque to the optimiser (else it rebuilds a 64-bit induction variable per array)
__device__ __forceinline__ const float* at_bytes(const float* base, unsigned boff) { return (const float*)((const char*)base + boff); }
__device__ __forceinline__ float* at_bytes(float* base, unsigned boff) { return (float*)((char*)base + boff); }
__device__ __forceinline__ unsigned opaque_v(unsigned x) { asm("" : "+v"(x)); return x; }

// One quad in three pieces -- load, compute, store -- so that a caller with several quads per thread can request the
// next quad's operands BETWEEN the arithmetic of the current one and its stores (vector-memory operations retire in
// order: loads issued behind a quad's stores wait for those stores as well).
// V: the variant (greb_kernels.h).  kVExp: the member's sensitivity-experiment switches `xsw` (member_switches) are
// honoured; without it they are compiled out.
struct PhysIn {
  f4 Ts, Ta, To, q, cap;                      // state
  f4 zt, gl, zo, ez;                          // static fields
  f4 tcl, cld, mld, mldm, swet, u, v;         // forcing of the step (mldm: previous step, :507-508); u, v: kRouteArrays only
  f4 wind;                                    // kRouteRecord only: the wind-speed term of hydro instead of u and v
  f4 c0, c1, c2;                              // flux: Toclim, qclim, -- ; scenario: TF, qF, ToF
  f4 acc0, acc1, acc2, acc3, acc4, acc5;      // monthly sums, annual Tsurf sum
  f4 qcl, tclp;                               // experiments only
  f4 fw;                                      // FORCE only: the CO2 pattern's weights
  float solar;
};
struct PhysOut { // everything the stores need: the inputs are dead once this exists
  f4 Ts, Ta, To, q, cap, TF, qF, ToF, tsmn;
  f4 s0, s1, s2, s3, s4; // the monthly sums including this step (:974)
};

// kRouteRecord (96x48; rec: the record of the member's set, member_record).  The quad's row comes from qd, the grid being
// known; boundary data the record does not hold (the rare reads below) comes from the raw arrays.
template <unsigned V>
__device__ __forceinline__ PhysIn physics_load_record(const MemberArgs& a, int qd, const StepClock& ck, const float* __restrict__ state,
                                                      const float* __restrict__ acc, const float* __restrict__ corr, unsigned xsw_member,
                                                      const MemberForce& F, BoundPtr B, const float* __restrict__ rec) {
  constexpr bool FLUX = V & kVFlux, EXP = V & kVExp, FORCE = V & kVForce, BOUND = V & kVBound;
  constexpr int NQ = kFrNx / 4, np = kFrNx * kFrNy;
  const int row = qd / NQ;
  const size_t off = ck.off, offm = ck.offm;
  const unsigned xsw = EXP ? xsw_member : 0u;
  const unsigned bo = opaque_v(16u * (unsigned)qd);                                                      // the quad in an [np] array
  const unsigned lon4 = 4u * (unsigned)(qd - row * NQ);
  const unsigned ro_static = opaque_v((forcing_record_offset(row, 0, 0) + lon4) * 4u);              // ... in the record's static part
  const unsigned ro = opaque_v((forcing_record_offset(row, kFrStaticFields, 0) + lon4) * 4u);       // ... in the step's slice
  const float* slice = rec + kFrStaticFloats + (size_t)(ck.ityr - 1) * kFrStepFloats;
  auto fr = [&](int field) {
    return ld4(at_bytes(field < kFrStaticFields ? rec : slice, field < kFrStaticFields ? ro_static : ro) + forcing_record_offset(0, field, 0));
  };
  PhysIn i;
  i.Ts = ld4(at_bytes(state, bo)); i.Ta = ld4(at_bytes(state + np, bo)); i.To = ld4(at_bytes(state + 2 * np, bo));
  i.q = ld4(at_bytes(state + 3 * np, bo)); i.cap = ld4(at_bytes(state + 4 * np, bo));
  i.zt = fr(kFrZtopo); i.gl = fr(kFrGlacier); i.zo = fr(kFrZocean); i.ez = fr(kFrWzAir);
  i.tcl = fr(kFrTclim); i.cld = fr(kFrCld); i.mld = fr(kFrMld); i.mldm = fr(kFrMldPrev); i.swet = fr(kFrSwet); i.wind = fr(kFrWind);
  const unsigned so = opaque_v(4u * (unsigned)row);
  if (FORCE) {
#pragma clang fp contract(off)
    i.solar = *at_bytes(F.solar + (size_t)(ck.ityr - 1) * kFrNy, so) * F.scale; // one rounding, then sw = solar * (1 - albedo)
  } else i.solar = *at_bytes(a.sw_solar + (size_t)(ck.ityr - 1) * kFrNy, so);
  if (FLUX) { i.c0 = ld4(at_bytes(GREB_BF(toclim), bo)); i.c1 = ld4(at_bytes(GREB_BF(qclim) + off, bo)); i.c2 = zero4(); }
  else {
    i.c0 = ld4(at_bytes(corr + off, bo)); i.c1 = ld4(at_bytes(corr + (size_t)kNT * np + off, bo));
    i.c2 = ld4(at_bytes(corr + (size_t)2 * kNT * np + off, bo));
    if (FORCE && F.noise.sigma) // TF' = fl(TF + N): the step's flux correction of :258 with the member's noise
      i.c0 = add4_exact(i.c0, noise_quad(F.noise, *(const int*)at_bytes((const float*)F.noise.rowcell, so), (int)lon4, ld4(at_bytes(F.noise.sigma, bo))));
  }
  i.acc0 = i.acc1 = i.acc2 = i.acc3 = i.acc4 = zero4();
#ifdef GREB_TUNING
  const bool no_acc = a.dbg & 1; // timing experiments (tools/stamp_member.py, GREB_DEBUG_PHYS)
#else
  constexpr bool no_acc = false;
#endif
  i.acc5 = no_acc ? zero4() : ld4(at_bytes(acc + 5 * np, bo));
  if (!FLUX && !no_acc) {
    i.acc0 = ld4(at_bytes(acc, bo)); i.acc1 = ld4(at_bytes(acc + np, bo)); i.acc2 = ld4(at_bytes(acc + 2 * np, bo));
    i.acc3 = ld4(at_bytes(acc + 3 * np, bo)); i.acc4 = ld4(at_bytes(acc + 4 * np, bo));
  }
  i.qcl = zero4(); i.tclp = zero4();
  if (EXP && (xsw & kXLwLinear)) i.qcl = FLUX ? i.c1 : ld4(at_bytes(GREB_BF(qclim) + off, bo));
  if (EXP && !FLUX && (xsw & kXSstPlus1)) i.tclp = ld4(at_bytes(GREB_BF(tclim) + offm, bo));
  i.fw = zero4();
  if (FORCE && F.space) i.fw = ld4(at_bytes(F.space, bo));
  if (FORCE && F.sst_anom) {
    const bool plus1 = (xsw & kXSstPlus1) != 0;
    const f4 tclp = plus1 ? i.tclp : ld4(at_bytes(GREB_BF(tclim) + offm, bo));
    prescribe_sst(F, plus1, i.zt, tclp, ld4(at_bytes(F.sst_anom, bo)), F.sst_weight ? ld4(at_bytes(F.sst_weight, bo)) : zero4(), i.Ts);
  }
  return i;
}

template <unsigned V, int ROUTE = kRouteArrays>
__device__ __forceinline__ PhysIn physics_load(const MemberArgs& a, int qd, const StepClock& ck, const float* __restrict__ state,
                                               const float* __restrict__ acc, const float* __restrict__ corr, unsigned xsw_member,
                                               const MemberForce& F, BoundPtr B, const float* __restrict__ rec = nullptr) {
  constexpr bool FLUX = V & kVFlux, EXP = V & kVExp, FORCE = V & kVForce, BOUND = V & kVBound;
  static_assert(variant_valid(V), "no such variant of the step kernels");
  if constexpr (ROUTE == kRouteRecord) return physics_load_record<V>(a, qd, ck, state, acc, corr, xsw_member, F, B, rec);
  const int nx = a.nx, ny = a.ny, np = a.np, p0 = 4 * qd;
  const size_t off = ck.off, offm = ck.offm;
  const unsigned xsw = EXP ? xsw_member : 0u;
  PhysIn i;
  i.Ts = ld4(state + p0); i.Ta = ld4(state + np + p0); i.To = ld4(state + 2 * np + p0); i.q = ld4(state + 3 * np + p0);
  i.cap = ld4(state + 4 * np + p0);
  i.zt = ld4(GREB_BF(z_topo) + p0); i.gl = ld4(GREB_BF(glacier) + p0); i.zo = ld4(GREB_BF(z_ocean) + p0); i.ez = ld4(GREB_BF(wz_air) + p0);
  i.tcl = ld4(GREB_BF(tclim) + off + p0); i.cld = ld4(GREB_BF(cldclim) + off + p0); i.mld = ld4(GREB_BF(mldclim) + off + p0);
  i.mldm = ld4(GREB_BF(mldclim) + offm + p0); i.swet = ld4(GREB_BF(swetclim) + off + p0); i.u = ld4(GREB_BF(uclim) + off + p0);
  i.v = ld4(GREB_BF(vclim) + off + p0);
  if (FORCE) {
#pragma clang fp contract(off)
    i.solar = F.solar[(size_t)(ck.ityr - 1) * ny + p0 / nx] * F.scale; // one rounding, then sw = solar * (1 - albedo)
  } else i.solar = a.sw_solar[(size_t)(ck.ityr - 1) * ny + p0 / nx]; // a quad never straddles rows
  if (FLUX) { i.c0 = ld4(GREB_BF(toclim) + p0); i.c1 = ld4(GREB_BF(qclim) + off + p0); i.c2 = zero4(); }
  else {
    i.c0 = ld4(corr + off + p0); i.c1 = ld4(corr + (size_t)kNT * np + off + p0); i.c2 = ld4(corr + (size_t)2 * kNT * np + off + p0);
    if (FORCE && F.noise.sigma) { // TF' = fl(TF + N): the step's flux correction of :258 with the member's noise
      const int row = p0 / nx;
      i.c0 = add4_exact(i.c0, noise_quad(F.noise, F.noise.rowcell[row], p0 - row * nx, ld4(F.noise.sigma + p0)));
    }
  }
  i.acc0 = i.acc1 = i.acc2 = i.acc3 = i.acc4 = zero4();
#ifdef GREB_TUNING
  const bool no_acc = a.dbg & 1; // timing experiments (tools/stamp_member.py, GREB_DEBUG_PHYS)
#else
  constexpr bool no_acc = false;
#endif
  i.acc5 = no_acc ? zero4() : ld4(acc + 5 * np + p0);
  if (!FLUX && !no_acc) {
    i.acc0 = ld4(acc + p0); i.acc1 = ld4(acc + np + p0); i.acc2 = ld4(acc + 2 * np + p0); i.acc3 = ld4(acc + 3 * np + p0);
    i.acc4 = ld4(acc + 4 * np + p0);
  }
  i.qcl = zero4(); i.tclp = zero4(); // experiments only: qclim(ityr) for the linear emissivity, Tclim of the previous step
  if (EXP && (xsw & kXLwLinear)) i.qcl = FLUX ? i.c1 : ld4(GREB_BF(qclim) + off + p0);
  if (EXP && !FLUX && (xsw & kXSstPlus1)) i.tclp = ld4(GREB_BF(tclim) + offm + p0);
  i.fw = zero4();
  if (FORCE && F.space) i.fw = ld4(F.space + p0);
  if (FORCE && F.sst_anom) {
    const bool plus1 = (xsw & kXSstPlus1) != 0;
    const f4 tclp = plus1 ? i.tclp : ld4(GREB_BF(tclim) + offm + p0);
    prescribe_sst(F, plus1, i.zt, tclp, ld4(F.sst_anom + p0), F.sst_weight ? ld4(F.sst_weight + p0) : zero4(), i.Ts);
  }
  return i;
}

// Budget output (kVBudget variants, scenario phase only): where the thirteen flux terms of a step go.  Block-uniform:
// the member's running sums [kNBudget][np], and -- on the last step of a month -- the month's record and its step count
// (:974-984; step_clock is the one source of month ends for both record kinds).
struct BudgetSink {
  float* sum;
  float* rec; // null unless a month ends with this step
  float ndm;
};
template <bool BUDGET>
__device__ __forceinline__ BudgetSink budget_sink(const MemberArgs& a, int m, const StepClock& ck) {
  BudgetSink b{nullptr, nullptr, 1.f};
  if (BUDGET) {
    b.sum = a.bsum + (size_t)m * kNBudget * a.np;
    if (ck.mon >= 0) {
      b.ndm = (float)(kMonthDays[ck.mon] * 2);
      b.rec = a.brec + (((size_t)m * a.brec_years + (a.brec_year0 + ck.yr_rel)) * 12 + ck.mon) * kNBudget * a.np;
    }
  }
  return b;
}
// One term of one point into its sum, by its own load, add and store as soon as the term exists: nothing of the budget
// lives across the physics of a quad (the FAST member kernel has no register to spare there).  At a month's end the mean
// leaves non-temporally, as the five standard records do, and the sum restarts from zero.
template <bool BUDGET>
__device__ __forceinline__ void budget_add(const BudgetSink& b, int np, int term, int p, float x) {
  if (BUDGET) {
#pragma clang fp contract(off)
    float* s = b.sum + (size_t)term * np + p;
    float v = *s + x;
    if (b.rec) {
      __builtin_nontemporal_store(v / b.ndm, b.rec + (size_t)term * np + p);
      v = 0.f;
    }
    *s = v;
  }
}

// the point physics and the Euler update of the quad (src/greb.f90:254-268 scenario, :328-361 flux correction);
// xTa, xq: the tracers after the 24 circulation sub-steps.  BUDGET: the terms of the update are also added to the member's
// budget sums (bs; p0: the quad's first point) -- under a member's switches they are what the update really used.
// FORCE: CO2 is the member's scalar blended per point with its reference by the pattern's weight (forced_co2); the insolation
// came forced from physics_load.
template <bool STRICT, unsigned V, int ROUTE = kRouteArrays>
__device__ __forceinline__ PhysOut physics_compute(const MemberArgs& a, const Phys& P, const PhysIn& in, float co2, const f4& xTa,
                                                   const f4& xq, unsigned xsw_member, const BudgetSink& bs, int p0,
                                                   const MemberForce& F) {
  constexpr bool FLUX = V & kVFlux, EXP = V & kVExp, BUDGET = V & kVBudget, FORCE = V & kVForce;
  static_assert(variant_valid(V), "no such variant of the step kernels");
  const unsigned xsw = EXP ? xsw_member : 0u;
  const int np = a.np;
  PhysOut o;
  o.TF = o.qF = o.ToF = zero4();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)
    float Ts1 = in.Ts.v[e];
    const float Ta1 = in.Ta.v[e], To1 = in.To.v[e], q1 = in.q.v[e], cap = in.cap.v[e];
    const float zt = in.zt.v[e], gl = in.gl.v[e], ez = in.ez.v[e], tcl = in.tcl.v[e], cld = in.cld.v[e], mld = in.mld.v[e];
    // (a prescribed member's switch has acted in physics_load, before the blend: prescribe_sst)
    if (EXP && !FLUX && (xsw & kXSstPlus1) && !(FORCE && F.sst_anom) && zt < 0.0f) Ts1 = in.tclp.v[e] + 1.0f; // greb.original.model.f90:226
    // A member without circulation (greb.original.model.f90:553) whose launch transported it with the others -- the band
    // and strip kernels run every member alike -- drops both increments here: +0, which is what its own zero sub-steps
    // give (xTa == Ta1 bit for bit).
    const bool calm = EXP && (xsw & kXNoCirc);
    const float dTa_crcl = calm ? 0.f : xTa.v[e] - Ta1; // :551
    const float dq_crcl = (calm || (EXP && (xsw & kXNoQTransport))) ? 0.f : xq.v[e] - q1; // greb.original.model.f90:554-555
    budget_add<BUDGET>(bs, np, kBdTaCrcl, p0 + e, dTa_crcl); budget_add<BUDGET>(bs, np, kBdqCrcl, p0 + e, dq_crcl);
    float albedo, sw, LWsurf, LWdown, em, Qlat, Qlat_air, dq_eva, dq_rain, dT_ocean, dTo;
    sw_radiation<STRICT>(P, Ts1, zt, gl, cld, in.solar, albedo, sw, xsw);
    budget_add<BUDGET>(bs, np, kBsw, p0 + e, sw);
    const float co2_e = (FORCE && F.space) ? forced_co2(F, in.fw.v[e], co2) : co2;
    lw_radiation<STRICT>(P, Ts1, Ta1, q1, co2_e, ez, cld, tcl, LWsurf, LWdown, em, xsw, in.qcl.v[e]);
    budget_add<BUDGET>(bs, np, kBLWsurf, p0 + e, LWsurf); budget_add<BUDGET>(bs, np, kBLWdown, p0 + e, LWdown);
    const float LWabs = em * LWsurf; // the product of :260
    budget_add<BUDGET>(bs, np, kBLWabs, p0 + e, LWabs);
    const float Qsens = P.ct_sens * (Ta1 - Ts1); // :295
    budget_add<BUDGET>(bs, np, kBQsens, p0 + e, Qsens);
    if constexpr (ROUTE == kRouteRecord) hydro_wind<STRICT>(P, Ts1, q1, in.wind.v[e], ez, in.swet.v[e], Qlat, Qlat_air, dq_eva, dq_rain, xsw);
    else hydro<STRICT>(P, Ts1, q1, in.u.v[e], in.v.v[e], zt, ez, in.swet.v[e], Qlat, Qlat_air, dq_eva, dq_rain, xsw);
    budget_add<BUDGET>(bs, np, kBQlat, p0 + e, Qlat); budget_add<BUDGET>(bs, np, kBQlatAir, p0 + e, Qlat_air);
    budget_add<BUDGET>(bs, np, kBdqEva, p0 + e, dq_eva); budget_add<BUDGET>(bs, np, kBdqRain, p0 + e, dq_rain);
    deep_ocean<STRICT>(P, Ts1, To1, zt, mld, in.mldm.v[e], in.zo.v[e], dT_ocean, dTo, xsw);
    budget_add<BUDGET>(bs, np, kBdTocean, p0 + e, dT_ocean); budget_add<BUDGET>(bs, np, kBdTo, p0 + e, dTo);
    const float LWup = LWdown; // :432
    float Ts0, Ta0, To0, q0;
    if (FLUX) {
      const float dTs = fdiv<STRICT>(P.dt * (sw + LWsurf - LWdown + Qlat + Qsens), cap);                    // :333
      Ts0 = Ts1 + dTs + dT_ocean;                                                              // :334
      const float dTa = fdiv<STRICT>(P.dt * (LWup + LWdown - em * LWsurf + Qlat_air - Qsens), P.cap_air);   // :336
      Ta0 = Ta1 + dTa + dTa_crcl;                                                              // :337
      To0 = To1 + dTo;                                                                         // :339
      const float dq = P.dt * (dq_eva + dq_rain);                                              // :341
      q0 = q1 + dq + dq_crcl;                                                                  // :342
      const float TF = fdiv<STRICT>((tcl - Ts0) * cap, P.dt);                                               // :344-345
      Ts0 = Ts1 + dTs + dT_ocean + fdiv<STRICT>(TF * P.dt, cap);                                            // :347
      const float ToF = in.c0.v[e] - To0;                                                      // :349
      To0 = To1 + dTo + ToF;                                                                   // :351
      const float qF = in.c1.v[e] - q0;                                                        // :353
      q0 = q1 + dq + dq_crcl + qF;                                                             // :355
      o.TF.v[e] = TF; o.qF.v[e] = qF; o.ToF.v[e] = ToF;
    } else {
      const float TF = in.c0.v[e], qF = in.c1.v[e], ToF = in.c2.v[e];
      Ts0 = Ts1 + dT_ocean + fdiv<STRICT>(P.dt * (sw + LWsurf - LWdown + Qlat + Qsens + TF), cap);          // :258
      Ta0 = Ta1 + dTa_crcl + fdiv<STRICT>(P.dt * (LWup + LWdown - em * LWsurf + Qlat_air - Qsens), P.cap_air); // :260
      To0 = To1 + dTo + ToF;                                                                   // :262
      float dq = P.dt * (dq_eva + dq_rain) + dq_crcl + qF;                                     // :264
      if (dq <= -q1) dq = -0.9f * q1;                                                          // :265
      q0 = q1 + dq;                                                                            // :266
    }
    o.Ts.v[e] = Ts0; o.Ta.v[e] = Ta0; o.To.v[e] = To0; o.q.v[e] = q0;
    o.cap.v[e] = seaice<STRICT>(P, Ts0, zt, gl, mld, cap, xsw);                                              // :268/:357
    o.tsmn.v[e] = in.acc5.v[e] + Ts0;                                                          // :945
    o.s0.v[e] = in.acc0.v[e] + Ts0; o.s1.v[e] = in.acc1.v[e] + Ta0; o.s2.v[e] = in.acc2.v[e] + To0; // :974
    o.s3.v[e] = in.acc3.v[e] + q0; o.s4.v[e] = in.acc4.v[e] + albedo;
  }
  return o;
}

// state write-back, correction / accumulation / monthly records (:974-984), annual mean (:945-956).  Returns the
// annual-mean Tsurf quad in tsmn_mean when ityr == 730 (the caller feeds the global-mean sum, :954).
// kRouteRecord: the same stores through the quad's opaque byte offset
template <bool FLUX>
__device__ __forceinline__ void physics_store_record(const MemberArgs& a, int m, int qd, const StepClock& ck,
                                                     const PhysOut& o, float* __restrict__ state, float* __restrict__ acc,
                                                     float* __restrict__ corr, f4& tsmn_mean) {
  constexpr int np = kFrNx * kFrNy;
  const int mon = ck.mon;
  const size_t off = ck.off;
  const unsigned bo = opaque_v(16u * (unsigned)qd);
#ifdef GREB_TUNING
  const bool no_acc = a.dbg & 1, no_wb = a.dbg & 2;
#else
  constexpr bool no_acc = false, no_wb = false;
#endif
  if (!no_wb) {
    st4(at_bytes(state, bo), o.Ts); st4(at_bytes(state + np, bo), o.Ta); st4(at_bytes(state + 2 * np, bo), o.To);
    st4(at_bytes(state + 3 * np, bo), o.q); st4(at_bytes(state + 4 * np, bo), o.cap);
  }
  if (FLUX) {
    st4(at_bytes(corr + off, bo), o.TF); st4(at_bytes(corr + (size_t)kNT * np + off, bo), o.qF);
    st4(at_bytes(corr + (size_t)2 * kNT * np + off, bo), o.ToF);
  } else {
#pragma clang fp contract(off)
    f4 s0 = o.s0, s1 = o.s1, s2 = o.s2, s3 = o.s3, s4 = o.s4;
    if (mon >= 0) { // :975-984
      const float ndm = (float)(kMonthDays[mon] * 2);
      float* rec = a.monthly + (((size_t)m * a.monthly_years + (a.year_out0 + ck.yr_rel)) * 12 + mon) * 5 * np;
      f4 r0, r1, r2, r3, r4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r0.v[e] = s0.v[e] / ndm; r1.v[e] = s1.v[e] / ndm; r2.v[e] = s2.v[e] / ndm; r3.v[e] = s3.v[e] / ndm; r4.v[e] = s4.v[e] / ndm;
      }
      st4_nt(at_bytes(rec, bo), r0); st4_nt(at_bytes(rec + np, bo), r1); st4_nt(at_bytes(rec + 2 * np, bo), r2);
      st4_nt(at_bytes(rec + 3 * np, bo), r3); st4_nt(at_bytes(rec + 4 * np, bo), r4);
      s0 = s1 = s2 = s3 = s4 = zero4();
    }
    if (!no_acc) {
      st4(at_bytes(acc, bo), s0); st4(at_bytes(acc + np, bo), s1); st4(at_bytes(acc + 2 * np, bo), s2);
      st4(at_bytes(acc + 3 * np, bo), s3); st4(at_bytes(acc + 4 * np, bo), s4);
    }
  }
  if (ck.ityr == kNT) { // :948-956
#pragma clang fp contract(off)
    f4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t.v[e] = o.tsmn.v[e] / (float)kNT;
    tsmn_mean = t;
    if (!no_acc) st4(at_bytes(acc + 5 * np, bo), zero4());
  } else {
    if (!no_acc) st4(at_bytes(acc + 5 * np, bo), o.tsmn);
  }
}

template <bool FLUX, int ROUTE = kRouteArrays>
__device__ __forceinline__ void physics_store(const MemberArgs& a, int m, int qd, const StepClock& ck,
                                              const PhysOut& o, float* __restrict__ state, float* __restrict__ acc,
                                              float* __restrict__ corr, f4& tsmn_mean) {
  if constexpr (ROUTE == kRouteRecord) { physics_store_record<FLUX>(a, m, qd, ck, o, state, acc, corr, tsmn_mean); return; }
  const int np = a.np, p0 = 4 * qd, mon = ck.mon;
  const size_t off = ck.off;
#ifdef GREB_TUNING
  const bool no_acc = a.dbg & 1, no_wb = a.dbg & 2;
#else
  constexpr bool no_acc = false, no_wb = false;
#endif
  if (!no_wb) {
    st4(state + p0, o.Ts); st4(state + np + p0, o.Ta); st4(state + 2 * np + p0, o.To); st4(state + 3 * np + p0, o.q);
    st4(state + 4 * np + p0, o.cap);
  }
  if (FLUX) {
    st4(corr + off + p0, o.TF); st4(corr + (size_t)kNT * np + off + p0, o.qF); st4(corr + (size_t)2 * kNT * np + off + p0, o.ToF);
  } else {
#pragma clang fp contract(off)
    f4 s0 = o.s0, s1 = o.s1, s2 = o.s2, s3 = o.s3, s4 = o.s4;
    if (mon >= 0) { // :975-984
      const float ndm = (float)(kMonthDays[mon] * 2);
      float* rec = a.monthly + (((size_t)m * a.monthly_years + (a.year_out0 + ck.yr_rel)) * 12 + mon) * 5 * np;
      f4 r0, r1, r2, r3, r4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r0.v[e] = s0.v[e] / ndm; r1.v[e] = s1.v[e] / ndm; r2.v[e] = s2.v[e] / ndm; r3.v[e] = s3.v[e] / ndm; r4.v[e] = s4.v[e] / ndm;
      }
      // written once, read by nobody on the device: keep the records out of the L2 / MALL the state lives in
      st4_nt(rec + p0, r0); st4_nt(rec + np + p0, r1); st4_nt(rec + 2 * np + p0, r2); st4_nt(rec + 3 * np + p0, r3); st4_nt(rec + 4 * np + p0, r4);
      s0 = s1 = s2 = s3 = s4 = zero4();
    }
    if (!no_acc) { st4(acc + p0, s0); st4(acc + np + p0, s1); st4(acc + 2 * np + p0, s2); st4(acc + 3 * np + p0, s3); st4(acc + 4 * np + p0, s4); }
  }
  if (ck.ityr == kNT) { // :948-956
#pragma clang fp contract(off)
    f4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t.v[e] = o.tsmn.v[e] / (float)kNT;
    tsmn_mean = t;
    if (!no_acc) st4(acc + 5 * np + p0, zero4());
  } else {
    if (!no_acc) st4(acc + 5 * np + p0, o.tsmn);
  }
}

// the three pieces in a row (one quad per thread: the any-grid engine)
template <bool STRICT, unsigned V, int ROUTE = kRouteArrays>
__device__ __forceinline__ void physics_quad(const MemberArgs& a, const Phys& P, int m, int qd, const StepClock& ck,
                                             float co2, float* __restrict__ state, float* __restrict__ acc,
                                             float* __restrict__ corr, const f4& xTa, const f4& xq, f4& oTa_out,
                                             f4& oq_out, f4& tsmn_mean, unsigned xsw, const MemberForce& F, BoundPtr B,
                                             const float* __restrict__ rec = nullptr) {
  constexpr bool FLUX = V & kVFlux, BUDGET = V & kVBudget;
  const PhysIn in = physics_load<V, ROUTE>(a, qd, ck, state, acc, corr, xsw, F, B, rec);
  const PhysOut o = physics_compute<STRICT, V, ROUTE>(a, P, in, co2, xTa, xq, xsw, budget_sink<BUDGET>(a, m, ck), 4 * qd, F);
  physics_store<FLUX, ROUTE>(a, m, qd, ck, o, state, acc, corr, tsmn_mean);
  oTa_out = o.Ta; oq_out = o.q;
}
#undef GREB_BF

} // namespace greb
