// greb_kernels.h -- launch interface between the C-ABI host code (greb_host.h) and the HIP
// kernels (greb_kernels.hip).  Internal; the public surface is include/greb_engine.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <utility>
#include <vector>

#include "greb_device.h"
#include "greb_noise.h"

namespace greb {

constexpr int kNT = 730;

// Timing-experiment knobs (skip a family of tasks, shorten the sub-step loop, tile sizes) exist only in a
// -DGREB_TUNING build (greb_climate_model_amd/build.py: build_lib(tuning=True) -> libgreb_hip_tuning.so, used by
// tools/).  The release library never reads the environment: a stray variable cannot change the physics.
#ifdef GREB_TUNING
inline int tuning_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
#else
constexpr int tuning_int(const char*, int dflt) { return dflt; }
#endif

// Kernels whose dynamic LDS size depends on the call (grid, band size, member count) are all allowed the SAME maximum:
// the attribute is per kernel, not per launch, and two host threads driving two engines side by side
// (ensemble.run_beside) must not lower it between each other's set and launch.  What a launch occupies is the size it
// passes, not this ceiling.
constexpr int kMaxDynamicLds = 160 * 1024;

// greb_member_forcing of include/greb_engine.h as the kernels read it: four words per member
struct MemberForcing {
  int co2_pattern;   // -1: CO2 is the member's scalar; else the pattern whose weights blend it with co2_ref
  float co2_ref;     // CO2 where the weight is 0
  int solar_table;   // -1: MemberArgs::sw_solar; else a table of MemberArgs::f_solar
  float solar_scale; // multiplies the table
};

// greb_member_sst of include/greb_engine.h as the kernels read it: two words per member
struct MemberSst {
  int pattern; // -1: the member's ocean surface is free; else the pattern it is held to
  float amp;   // multiplies the pattern's anomaly
};

// One boundary set (greb_engine_add_boundary_set) as the kernels read it: the nine input fields of greb_fields that a set
// may replace and the four derived from them, each pointer either the set's own array or the engine's.  Entry 0 of the
// table is the engine's own data.
struct BoundarySet {
  const float *z_topo, *glacier;
  const float *tclim, *qclim, *uclim, *vclim, *mldclim, *cldclim, *swetclim;
  const float *toclim, *z_ocean, *wz_air, *wz_vapor;
};
constexpr int kBoundaryFields = 13; // pointers of a BoundarySet; the first kBoundaryInputs are inputs, the rest derived
constexpr int kBoundaryInputs = 9;
constexpr int kMaxBoundarySets = 16;

// Forcing record of one boundary set (FAST fused 96x48 member kernel only): everything the point physics of
// the default scenario and flux-correction quads reads from boundary data, packed in two parts: the four static fields
// [row 0..47][field][96], then the step's fields [step 0..729][row 0..47][field][96] -- so that a quad's operands sit at a
// scalar base (the static part, the step's slice) plus a 32-bit lane offset (row and quad) plus the field's instruction
// immediate.  kFrWind is the wind-speed term of hydro (greb_device.h: wind_speed), evaluated once per set by the pack
// kernel instead of per member and step.
constexpr int kFrNx = 96, kFrNy = 48;
enum { kFrZtopo, kFrGlacier, kFrZocean, kFrWzAir, kFrStaticFields,
       kFrTclim = kFrStaticFields, kFrCld, kFrMld, kFrMldPrev, kFrSwet, kFrWind, kFrFields };
constexpr int kFrStepFields = kFrFields - kFrStaticFields;
// offset in floats of (row, field, longitude) inside the field's part -- the static part or one step's slice: host (pack
// launch, read-back, layout query) and device
constexpr unsigned forcing_record_offset(int row, int field, int lon) {
  return field < kFrStaticFields ? ((unsigned)row * kFrStaticFields + (unsigned)field) * kFrNx + (unsigned)lon
                                 : ((unsigned)row * kFrStepFields + (unsigned)(field - kFrStaticFields)) * kFrNx + (unsigned)lon;
}
constexpr unsigned kFrStaticFloats = forcing_record_offset(kFrNy, 0, 0), kFrStepFloats = forcing_record_offset(kFrNy, kFrStaticFields, 0);
constexpr size_t kFrBytes = ((size_t)kFrStaticFloats + (size_t)kNT * kFrStepFloats) * sizeof(float);
static_assert(forcing_record_offset(0, kFrFields - 1, 0) * sizeof(float) <= 4095 && forcing_record_offset(0, kFrStaticFields - 1, 0) * sizeof(float) <= 4095,
              "a field's offset must fit the immediate of a global load");
static_assert(kFrBytes < (1ull << 31), "offsets into a record are 32-bit");

// The chunks a dealt launch of the fused member kernel cuts every member's steps into (greb_member.hip): chunk c is the
// steps [end[c - 1], end[c]) of the launch, end[-1] = 0.  Host-built, the same for every member.
constexpr int kMaxChunks = 10;
struct ChunkTable { int n; int end[kMaxChunks]; };
// The schedules: kChunksHalving -- each chunk half of what is left, so that the LAST one, which sets what the launch's
// tail can still cost, is short while the chunks, each of which pays the kernel's prologue, stay few: 365 / 183 / 91 / 46 /
// 23 / 12 / 10 of a year's 730 steps (other step counts in proportion); kChunksEqual -- ten equal chunks; kChunksQuarters
// -- the halving schedule with its first half cut in two: 183 / 182 / 183 / 91 / 46 / 23 / 12 / 10, so that the members of
// an incomplete last round start after a quarter of a year, not after half of one.
enum { kChunksHalving = 0, kChunksEqual = 1, kChunksQuarters = 2, kNChunkSchedules };
inline ChunkTable chunk_table(int schedule, int nsteps) {
  constexpr int kHalving[7] = {365, 548, 639, 685, 708, 720, 730};
  constexpr int kQuarters[8] = {183, 365, 548, 639, 685, 708, 720, 730};
  ChunkTable t{};
  const int n = schedule == kChunksEqual ? kMaxChunks : (schedule == kChunksQuarters ? 8 : 7);
  for (int c = 0; c < n; ++c) {
    const long long e = schedule == kChunksEqual ? (long long)nsteps * (c + 1) / n
                                                 : (long long)nsteps * (schedule == kChunksQuarters ? kQuarters[c] : kHalving[c]) / 730;
    if (e > (t.n ? t.end[t.n - 1] : 0)) t.end[t.n++] = (int)e; // (a launch of a few steps: no empty chunks)
  }
  return t;
}
// the queue's words in front of its items, and an item: (member << 4 | chunk) + 1, 0 = not pushed yet
enum { kQHead = 0, kQTail = 1, kQItems = 4 };
constexpr int kMaxDealtMembers = 1 << 27;

// Everything the fused member kernel needs (passed by value as a kernel argument).
struct MemberArgs {
  int nx, ny, np;
  // shared static fields (HBM, read-only)
  const float *z_topo, *glacier, *sw_solar;
  const float *tclim, *qclim, *uclim, *vclim, *mldclim, *cldclim, *swetclim;
  const float *toclim, *z_ocean, *wz_air, *wz_vapor;
  // per member
  float* state;          // [nm][5][np]   Ts, Ta, To, q, cap_surf
  float* acc;            // [nm][6][np]   Tmm, Tamm, Tomm, qmm, apmm (src/greb.f90:149), tsmn (:145)
  float* corr;           // [ncorr][3][730][np]  TF_correct, qF_correct, ToF_correct (:110)
  const int* corr_index; // [nm] -> which correction set a member reads/writes
  const RowTables* tabs; // [ntab]
  const int* tab_index;  // [nm]
  const Phys* phys;      // [nm]
  // run control
  int flux_phase;        // 1: qflux_correction (:311-364), 0: scenario (:228-234 + time_loop)
  long long it0;         // `it` of the first step of this launch (1-based)
  int nsteps;
  int nsub;              // max(1,nint(dt/dt_crcl)) = 24 (:543)
  const float* co2;      // scenario: [nm][co2_stride] annual series; flux: unused
  int co2_stride;
  int co2_year0;         // index into the series of the year containing it0
  float co2_flux;
  float* monthly;        // [nm][rec_stride_years][12][5][np]; record for (year_out, month)
  int monthly_years;     // years per member in `monthly`
  int year_out0;         // output-year index of the year containing it0
  float* yearly;         // [nm][yearly_years][2] or nullptr
  int yearly_years, yearly_year0;
  int ipx, ipy;          // 1-based
  unsigned xsw;          // experiment switches (kX*, greb_device.h); 0 = complete model
  // -DGREB_TUNING builds only (null otherwise; the release kernels contain no stamp code): per member and wave, 8
  // cycle totals of one launch -- see tools/stamp_member.py
  unsigned long long* stamps;
  int dbg;               // -DGREB_TUNING builds only: timing experiments (results wrong): bit 0 point physics without the
                         // accumulators, bit 1 without the state write-back, bit 2 a single pass instead of three
  // per-member experiment control (read by the kVExp variants only; greb_physics_step.h: member_switches)
  const unsigned* xsw_m;   // [nm] experiment switches of each member; null: xsw applies to all
  const float* co2_flux_m; // [nm] flux-phase CO2 of each member; null: co2_flux applies to all
  // budget output (read by the kVBudget variants only; null otherwise: greb_physics_step.h, budget_sink)
  float* bsum;             // [nm][kNBudget][np] running sums of the month's flux terms
  float* brec;             // [nm][brec_years][12][kNBudget][np] monthly means of the terms
  int brec_years;          // years per member in `brec`
  int brec_year0;          // index there of the year containing it0
  // per-member forcing (read by the kVForce variants only, which a launch takes when force_m is set; scenario phase
  // only: greb_physics_step.h, member_force).  Appended: the offsets of everything above are those of a build without it.
  const MemberForcing* force_m; // [nm] each member's four words; null: no member of the launch is forced
  const float* f_space;         // [n_patterns][np]  CO2 weights in [0, 1]
  const float* f_season;        // [n_patterns][730] their seasonal factor (all ones where the caller gave none)
  const float* f_solar;         // [n_solar][730][ny] insolation tables
  // boundary sets (read by the kVBound variants only, which a launch takes when bset_m is set; both phases:
  // greb_physics_step.h, member_boundary).  Appended likewise.
  const BoundarySet* bsets;     // [1 + sets made]; entry 0 holds the thirteen pointers above
  const int* bset_m;            // [nm] each member's set; null: every member of the launch is on the engine's own data
  // the ready queue of a dealt launch (greb_member.hip: "The deal of member-year chunks", greb_member_queue.h; null: workgroup b integrates
  // member b for the whole launch).  Appended likewise.
  unsigned* queue;              // kQ* words, then `q_capacity` item words
  unsigned* q_status;           // [4], sticky: [0] != 0: a workgroup gave up waiting for an item, [1] the slot it waited for
  unsigned q_capacity;          // members x chunks: the ring never wraps within a launch
  ChunkTable chunks;            // the steps of the launch cut into chunks, the same for every member
  int stamp_members;            // -DGREB_TUNING builds only: members the stamp buffer was made for (the item records follow theirs)
  // prescribed SST (read by the kVForce variants only, beside force_m; scenario phase only: greb_physics_step.h,
  // member_force and prescribe_sst).  Appended likewise.
  const MemberSst* sst_m;       // [nm] each member's two words; null: no member of the launch is prescribed
  const float* s_anom;          // [n_sst][np]  anomalies in K
  const float* s_weight;        // [n_sst][np]  nudging weights in [0, 1]; null: 1 everywhere
  const float* s_season;        // [n_sst][730] the anomalies' seasonal factor (all ones where the caller gave none)
  // stochastic heat flux (read by the kVForce variants only, beside force_m; scenario phase only: greb_noise.h,
  // greb_physics_step.h: member_force and physics_load).  Appended likewise.
  const MemberNoise* noise_m;   // [nm] each member's four words; null: no member of the launch is noisy
  const float* n_sigma;         // [n_noise][np]  standard deviations in W/m2
  const float* n_season;        // [n_noise][730] their seasonal factor (all ones where the caller gave none)
  const int* n_cells;           // [n_noise][kNoiseRows + ny] log2(cell_x), hold, each row's first cell (greb_noise.h)
};

// The set table on the device: kSetTableEntries BoundarySet, then as many forcing-record pointers (entry 0: the engine's
// own data).  The FAST fused member kernel reads its record pointer there in every variant (greb_physics_step.h:
// member_record), so its launches carry MemberArgs::bsets also where no member is on a set; MemberArgs stays as it was.
constexpr int kSetTableEntries = kMaxBoundarySets + 1;
constexpr size_t kSetTableBytes = kSetTableEntries * (sizeof(BoundarySet) + sizeof(const float*));
inline const float** set_table_records(BoundarySet* table) { return (const float**)(table + kSetTableEntries); }

// GREB_NBUDGET, GREB_B_*: the flux terms of one step in the order of include/greb_engine.h
enum { kBsw, kBLWsurf, kBLWdown, kBLWabs, kBQsens, kBQlat, kBQlatAir, kBdqEva, kBdqRain, kBdTocean, kBdTo, kBdTaCrcl, kBdqCrcl, kNBudget };

// ---- Variants of the step kernels.  member_kernel (greb_member.hip) and physics_step_kernel (greb_kernels.hip) are
// templates over <bool STRICT, unsigned V>: V is a mask of the features compiled in, and a launch takes the instantiation
// whose features its MemberArgs ask for (select_variant).  A new variant is one entry of kVariants and its branch there.
// kVFlux: flux-correction phase (:311-364), else scenario; kVExp: honours the experiment switches (xsw, xsw_m);
// kVBudget: budget output (bsum, brec); kVForce: per-member forcing (force_m), prescribed SST (sst_m) and stochastic
// heat flux (noise_m); kVBound: boundary sets (bsets, bset_m)
enum : unsigned { kVFlux = 1, kVExp = 2, kVBudget = 4, kVForce = 8, kVBound = 16 };
// The flux-correction phase delivers no budget and is not forced; forcing and boundary sets exist in the switch-aware
// kernels only; a boundary-aware scenario kernel is forcing-aware (without a forced member its launch carries words that
// force nothing).
constexpr bool variant_valid(unsigned v) {
  const bool flux = v & kVFlux, exp = v & kVExp, budget = v & kVBudget, force = v & kVForce, bound = v & kVBound;
  return v < 32u && !(budget && flux) && (!force || (exp && !flux)) && (!bound || (exp && (flux || force)));
}
// every variant that is built
constexpr unsigned kVariants[] = {0u, kVFlux, kVExp, kVFlux | kVExp, kVBudget, kVExp | kVBudget, kVExp | kVForce,
                                  kVExp | kVBudget | kVForce, kVFlux | kVExp | kVBound, kVExp | kVForce | kVBound,
                                  kVExp | kVBudget | kVForce | kVBound};
constexpr int kNVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));

// The variant a launch takes, decided by what it carries, in this order: a member on a boundary set, a forced member, budget
// output, experiment switches (of every member or of some), the phase.  Every member of the launch runs that one kernel.
// hipErrorInvalidValue, *v unwritten, for arguments that contradict each other.
inline hipError_t select_variant(const MemberArgs& a, unsigned* v) {
  const bool flux = a.flux_phase != 0, budget = a.bsum != nullptr;
  if (budget && (flux || !a.brec)) return hipErrorInvalidValue;
  unsigned r = (flux ? kVFlux : 0u) | (budget ? kVBudget : 0u);
  if (a.bset_m) {
    if (!a.bsets || (!flux && !a.force_m)) return hipErrorInvalidValue;
    r |= kVExp | kVBound | (flux ? 0u : kVForce);
  } else if (a.force_m) {
    if (flux) return hipErrorInvalidValue;
    r |= kVExp | kVForce;
  } else if (a.xsw || a.xsw_m) r |= kVExp;
  *v = r;
  return hipSuccess;
}
// greb_engine_describe's name for it (budget output is chosen per call, on top of the family)
inline const char* variant_family(unsigned v) {
  return (v & kVBound) ? "boundary" : (v & kVForce) ? "forcing" : (v & kVExp) ? "switches" : "default";
}
// The instantiation of a kernel family for (strict, v), or null where v is not in kVariants: Family<STRICT, V>::kernel() is
// the address of the family's kernel<STRICT, V>, and the walk compares v with the very constant it instantiates with.
template <template <bool, unsigned> class Family, size_t... I>
auto pick_variant(bool strict, unsigned v, std::index_sequence<I...>) {
  decltype(Family<false, 0u>::kernel()) k = nullptr;
  ((kVariants[I] == v ? (void)(k = strict ? Family<true, kVariants[I]>::kernel() : Family<false, kVariants[I]>::kernel()) : (void)0), ...);
  return k;
}
template <template <bool, unsigned> class Family>
auto pick_variant(bool strict, unsigned v) { return pick_variant<Family>(strict, v, std::make_index_sequence<kNVariants>{}); }

// fused engine (greb_member.hip): 96x48 with the default sub-cycling layout -- rows 0-9 and 38-47
// sub-cycled, only the two polar rows iterating; whole member resident in one CU
bool member_layout_supported(const RowTables& tab, int nx, int ny);
// how often the member kernel's static deal computes each row-quad of the 96x48 grid: counts[48 * 24]
void member_deal_cover(bool strict, int* counts);
// the LDS accesses of the bulk waves in one sub-step (greb_member.hip): records of 7 ints, at most `capacity` written;
// returns the number of records there are
int member_lds_table(bool strict, int* out, int capacity);
void member_lds_map(int* words8);
hipError_t launch_member_kernel(const MemberArgs& a, int n_members, bool strict, hipStream_t s, int workgroups = 0);
// the forcing record (kFrBytes at `rec`) of the set whose thirteen device arrays `b` names (greb_member.hip)
hipError_t launch_pack_forcing(const BoundarySet& b, float* rec, hipStream_t s);
hipError_t launch_circulation_g96(const float* X, const float* wz, const float* u, const float* v, float* dX,
                                  const RowTables* tab_dev, int batch, int nsub, bool strict, hipStream_t s);

// batched single-routine kernels, any grid with nx % 4 == 0, ny <= kMaxNy
// tab_host: the same table on the host (the 384-wide row-strip kernel takes its row constants by value)
hipError_t launch_diffusion(const float* T1, const float* wz, float* dX, const RowTables* tab_dev,
                            const RowTables& tab_host, int nx, int ny, int batch, bool strict, hipStream_t s);
// greb_rows.hip: the diffusion sweep of a 384-wide grid as wavefront-sized row strips (FAST and STRICT).
// The launch orders of the row-strip kernels (rows_tasks, step_rows_tasks, circ_rows_tasks) are host code of their own:
// greb_strip_order.cpp.
bool rows_supported(const RowTables& t, int nx, int ny);
struct RowsTask { int field, rows; }; // rows = k0 | k1 << 8 | kRowsUp: the task updates rows [k0, k1); field < 0: no task
constexpr int kRowsUp = 1 << 20;       // the strip walks south to north (else north to south)
struct RowsTuning {
  int chain_target;    // instructions per chain strip
  int chain_span;      // per cent of the launch over which the chain strips are spread
  int parts[4];        // strips the streaming region of a field is cut into, level 0 (most fields) .. 3 (the last fields)
  int level_tasks[4];  // about how many tasks levels 1..3 hold ([0] unused)
};
// measured on MI355X, batch 1 024 (tools/rows_ab.sh; settled clocks): streaming cut 4 / 5 / 6 / 8 / 12 strips per field
// 0.1738 / 0.1707 / 0.1697 / 0.1685 / 0.1678 ms per launch; chain span 50 / 60 / 70 / 80 / 100 %: 0.1724 / 0.1717 / 0.1691 /
// 0.181 / 0.209; without the fine levels 0.1724 against 0.1691
inline RowsTuning rows_default_tuning() { return RowsTuning{3000, 70, {8, 8, 16, 39}, {0, 0, 2048, 1024}}; }
void rows_tasks(const RowTables& t, int ny, int batch, const RowsTuning& tu, std::vector<RowsTask>& tasks);
void rows_release_cache();
hipError_t launch_diffusion_rows(const float* T1, const float* wz, float* dX, const RowTables& t, int ny, int batch,
                                 bool strict, hipStream_t s);
// greb_step_rows.hip: the engine's circulation sub-step on a 384- or 192-wide grid as wavefront-sized row strips, one launch each
bool step_rows_supported(const RowTables* tabs, int n_tabs, int nx, int ny);
constexpr int kStepRowsSlotsPerCu = 8; // wavefronts of the row-strip circulation kernels a CU holds (177-201 VGPRs: two per SIMD; 19.5 KB of LDS each)
void step_rows_tasks(const RowTables* tabs, const int* tab_index, int n_members, int ny, int n_slots,
                     std::vector<RowsTask>& tasks);
constexpr int kStepFieldBits = 16;  // a sub-step task's field word: field | row-table index << 16 (at most 32 767 members)
constexpr int kStepHeadTasks = 16; // the first tasks of the launch order travel in the kernel arguments (see StepArgs)
hipError_t step_rows_make_tasks(const RowTables* tabs_host, const int* tab_index_host, int n_members, int ny,
                                int n_slots, RowsTask** dev, int* n, RowsTask* head /* [kStepHeadTasks] */);
hipError_t launch_substep_rows(const float* X, const float* W2, const float* u, const float* v, float* Xnew,
                               const RowTables* tabs_dev, const int* tab_index_dev, const RowsTask* tasks, const RowsTask* head_host,
                               int n_tasks, int n_simd, int nx, int ny, bool strict, hipStream_t s, bool calm_vapor);
// greb_circ_rows.hip: the circulation CALL (all its sub-steps, src/greb.f90:546-550) on a 384-wide grid in ONE launch.
// The strips of a field hand their rows to each other through memory flags, so every task of the launch must be
// resident at once: the caller passes the wavefront slots it may use and the builder never makes more tasks than that.
struct CircTask {
  int field;   // (2 * member + tracer) | the member's row-table index << kStepFieldBits
  int rows;    // k0 | k1 << 8 | kCircChain: rows [k0, k1)
  int dep[4];  // the tasks that own rows k0-2, k0-1, k1, k1+1 of the same field (each listed once; -1: none)
  int issue;   // the builder's cost estimate in cycles (diagnostic)
  int pad;
};
constexpr int kCircChain = 1 << 21;        // the task is ONE row whose zonal chains live in registers for the whole call
constexpr int kChainTaskMinSweeps = 64;    // rows with at least this many dependent diffusion sweeps become chain tasks
constexpr unsigned kCircSpinTicks = 100u * 1000u * 1000u; // a strip waits at most this long for a neighbour: 1 s of the 100 MHz clock
void circ_rows_tasks(const RowTables* tabs, const int* tab_index, int n_members, int ny, int n_slots,
                     std::vector<CircTask>& tasks);
struct CircOrder {
  CircTask* tasks = nullptr;  // device
  unsigned* flags = nullptr;  // device, [n]: sub-steps completed by each task since the order was made
  unsigned* ctrl = nullptr;   // device, [8]: [0] abort (sticky), [1] task, [2] sub-step, [3] flag seen, [4] flag wanted
  int n = 0;
  unsigned epoch = 0;         // what every flag reads between two launches
};
hipError_t circ_rows_make_order(const RowTables* tabs_host, const int* tab_index_host, int n_members, int ny, int n_slots,
                                CircOrder* out);
void circ_rows_free_order(CircOrder* o);
// X[0] / X[1]: sub-step s reads X[s & 1] and writes X[(s + 1) & 1]; the result is in X[nsub & 1]
hipError_t launch_circulation_rows(float* X0, float* X1, const float* W2, const float* u, const float* v,
                                   const RowTables* tabs_dev, CircOrder& order, int n_simd, int nx, int ny, int nsub, bool strict,
                                   hipStream_t s, bool calm_vapor);
// after the stream has been synchronised: 0, or -1 with the strip that gave up waiting in msg[0..4] (ctrl[1..5])
int circ_rows_status(const CircOrder& o, unsigned* diag5);
hipError_t launch_advection(const float* T1, const float* wz, const float* u, const float* v, float* dX,
                            const RowTables* tab_dev, int nx, int ny, int batch, bool strict, hipStream_t s);
// 24 sub-steps; 96x48 uses the fused LDS loop of the engine, other grids launch per sub-step
hipError_t launch_circulation(const float* X, const float* wz, const float* u, const float* v, float* dX,
                              float* scratch /* 3*batch*np */, const RowTables* tab_dev, const RowTables& tab_host,
                              int nx, int ny, int batch, int nsub, bool strict, hipStream_t s);

// any-grid multi-launch engine (greb_kernels.hip)
hipError_t launch_substep_fused(const float* X, const float* W2, const float* u, const float* v, float* Xnew,
                                const RowTables* tabs, const int* tab_index, int nx, int ny, int n_members,
                                bool strict, hipStream_t s, bool calm_vapor = false);
hipError_t launch_physics_step(const MemberArgs& a, const float* X, float* Xout, float* red, int n_members,
                               bool strict, hipStream_t s);
hipError_t launch_yearly(const float* red, float* yearly, int np, int nx, int ipx, int ipy, int yearly_years,
                         int year_index, int n_members, bool strict, hipStream_t s);
hipError_t launch_pack_tracers(const float* state, float* X, int np, int n_members, hipStream_t s);
// greb_noise.hip: N of one member (words w) and one scenario step (0-based) at every point, out [ny][nx] on the device
hipError_t launch_noise_field(const MemberNoise& w, const float* n_sigma, const float* n_season, const int* n_cells, int nx, int ny,
                              long long step, float* out, hipStream_t s);

struct PointArgs {
  int nx, ny, np, ityr;
  float co2;
  const float *z_topo, *glacier, *sw_solar, *tclim, *uclim, *vclim, *mldclim, *cldclim, *swetclim;
  const float *z_ocean, *wz_air;
  Phys phys;
  unsigned xsw;       // experiment switches
  const float* qclim; // for kXLwLinear
  const float* in5; // Ts, Ta, To, q, cap_surf
  float* out15;
};
hipError_t launch_point_physics(const PointArgs& a, hipStream_t s);

} // namespace greb
