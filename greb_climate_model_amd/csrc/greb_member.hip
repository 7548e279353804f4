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
//
// Where the parts live (this file is the one translation unit of all of them):
//   greb_member_grid.h   grid constants and the padded row stride RS
//   greb_member_lds.h    the LDS map, comp / zip, ld8p / st8p
//   greb_member_deal.h   "The schedule": the two deal tables with their measurements, the task enumeration
//                        (task_rowquad), the completeness static_assert, task_addr -- constexpr, host and device
//   greb_member_bulk.h   the arithmetic of a bulk row task, make_tasks, make_signs, bulk_substep
//   greb_member_polar.h  the polar rows: chain_substep_strict, QuadChain
//   greb_member_queue.h  the ready queue of a dealt launch: item words, pop_item, push_next
//   here                 member_layout_supported, the host-visible tables of the deal and the LDS traffic (a variant
//                        build of this one source covers the kernel and its tables), stage_winds, Circ, the test
//                        mirror, member_kernel, pack_forcing_kernel and the launchers
// What a -DGREB_TUNING build adds (in-kernel stamps, timing experiments) is still #ifdef blocks inside Circ and
// member_kernel: gathered into types they changed the tuning library's kernels (profiles/member_split_ab.json).
#include <cstdlib>

#include "greb_kernels.h"
#include "greb_pair.h"
#include "greb_physics_step.h"
#include "greb_stencil.h"

#include "greb_member_lds.h"
#include "greb_member_deal.h"
#include "greb_member_bulk.h"
#include "greb_member_polar.h"
#include "greb_member_queue.h"

namespace greb {

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

// host-visible form of the deal's cover (greb_member_deal.h: deal_cover; greb_member_deal_cover): counts[k * NQ + q],
// rows 0 .. NY-1
void member_deal_cover(bool strict, int* counts) {
  constexpr DealCover cs = deal_cover<true>(), cf = deal_cover<false>();
  for (int i = 0; i < NY * NQ; ++i) counts[i] = strict ? cs.n[i] : cf.n[i];
}

// The LDS traffic of the bulk waves in one sub-step, for tools/lds_conflicts.py (greb_member_lds_table): one record of
// kLdsRecInts ints per lane of every LDS instruction of every dealt pass -- wave, the wave's pass slot, the instruction's
// number within the pass, lane, kind of access (kLds*), bytes per lane, float offset into the workgroup's LDS or -1 for a
// lane without a task.  The offsets are those of row_task / row_task2 reading buffer 0 and storing to buffer 1, from the
// deal, the enumeration and the LDS map of the headers; the chain wave(s) of the polar rows are not in it.
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
// The queue, its protocol and its fences: greb_member_queue.h (pop_item, push_next).

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
    const MemberForce mf = member_force<FORCE>(a, m, ck, it);
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
    // s_waitcnt vmcnt(6) where the variants end up at vmcnt(0).  (All A/B runs in one GPU session: boxes differ.)
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
