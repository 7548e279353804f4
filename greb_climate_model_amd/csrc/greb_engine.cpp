// greb_engine.cpp -- the C ABI of include/greb_engine.h over the HIP kernels (greb_kernels.hip).
//
// Host-side responsibilities (everything the reference does once per run outside the time loops):
//   * per-row grid tables, src/greb.f90:578-582, 652-654, 749-753, 838-840 (fp32, same expression
//     order, glibc cosf like the flang-built reference)
//   * derived fields of greb_model's preamble, src/greb.f90:176-216, and Toclim, :1088-1094
//   * device residency: inputs are copied to HBM once in create; state, corrections and
//     accumulators live in HBM between launches and in LDS/registers inside a launch
//   * one launch of the fused member kernel per model year (730 steps) per phase
// There is NO CPU fallback: without a HIP device create() fails with GREB_E_NOGPU.
#include "../../include/greb_engine.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "greb_kernels.h"
#include "greb_diag.h"
#include "greb_clim.h"
#include "greb_ens.h"

using namespace greb;

namespace {

thread_local std::string g_last_error; // for failures before an engine exists

int fail(greb_engine* e, int code, const std::string& msg);

#define HIP_TRY(e, expr)                                                                      \
  do {                                                                                        \
    hipError_t _err = (expr);                                                                 \
    if (_err != hipSuccess)                                                                   \
      return fail((e), (int)_err, std::string(#expr) + ": " + hipGetErrorString(_err));       \
  } while (0)

int nint_f(float x) { return (int)lroundf(x); }

// src/greb.f90:578-582, 652-654 (diffusion), 749-753, 838-840 (advection)
void compute_row_tables(const greb_params& p, float kappa, int nx, int ny, RowTables& g) {
  std::memset(&g, 0, sizeof(g));
  const float dlon = 360.f / (float)nx, dlat = 180.f / (float)ny; // :43-44
  const float deg = 2.f * p.pi * 6.371e6f / 360.f;                // :578
  const float dx = dlon, dy = dlat, dyy = dy * deg;               // :579
  const float dtc = (float)p.dt_crcl;
  g.dif_ccy = kappa * dtc / (dyy * dyy); // :581
  g.adv_ccy = dtc / dyy / 2.f;           // :752
  for (int k = 0; k < ny; ++k) {
    const float lat = dlat * (float)(k + 1) - dlat / 2.f - 90.f;    // :580
    const float dxlat = dx * deg * cosf(2.f * p.pi / 360.f * lat);  // :580
    g.dif_ccx[k] = kappa * dtc / (dxlat * dxlat);                   // :582
    g.adv_ccx[k] = dtc / dxlat / 2.f;                               // :753
    g.subcycled[k] = !(dxlat > 2.5e5f);                             // :592, :799
    {
      float dd = (float)nint_f(dtc / (1.f * (dxlat * dxlat) / kappa)); // :652
      if (dd < 1.f) dd = 1.f;
      const int dtdff2 = (int)(dtc / dd);
      // dtdff2 == 0 (384x192 polar rows) is undefined behaviour in the reference (NINT(Inf));
      // the flang x86-64 build yields time2 = 1, ccx2 = 0 -- defined so here.
      int t2 = dtdff2 == 0 ? 1 : nint_f(dtc / (float)dtdff2); // :653
      g.dif_time2[k] = t2 < 1 ? 1 : t2;
      g.dif_ccx2[k] = kappa * (float)dtdff2 / (dxlat * dxlat); // :654
    }
    {
      float dd = (float)nint_f(dtc / (dxlat / 10.0f / 1.f)); // :838
      if (dd < 1.f) dd = 1.f;
      const int dtdff2 = (int)(dtc / dd);
      int t2 = dtdff2 == 0 ? 1 : nint_f(dtc / (float)dtdff2); // :839
      g.adv_time2[k] = t2 < 1 ? 1 : t2;
      g.adv_ccx2[k] = (float)dtdff2 / dxlat / 2.f; // :840
    }
  }
}

// a member's namelist (greb_member_config::p) -> what the kernels read
Phys make_phys(const greb_params& p) {
  Phys P;
  P.sig = p.sig; P.ct_sens = p.ct_sens;
  P.da_ice = p.da_ice; P.a_no_ice = p.a_no_ice; P.a_cloud = p.a_cloud;
  P.Tl_ice1 = p.Tl_ice1; P.Tl_ice2 = p.Tl_ice2; P.To_ice1 = p.To_ice1; P.To_ice2 = p.To_ice2;
  P.co_turb = p.co_turb; P.ce = p.ce; P.cq_latent = p.cq_latent; P.cq_rain = p.cq_rain;
  P.z_air = p.z_air; P.r_qviwv = p.r_qviwv; P.rho_air = p.rho_air;
  for (int i = 0; i < 10; ++i) P.p_emi[i] = p.p_emi[i];
  P.cap_ocean = p.cp_ocean * p.rho_ocean;          // :186
  P.cap_land = p.cp_land * p.rho_land * p.d_land;  // :187
  P.cap_air = p.cp_air * p.rho_air * p.d_air;      // :188
  P.dt = (float)p.dt;
  return P;
}

template <typename T>
hipError_t dev_alloc(T** p, size_t n) { return hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)); }

// How the row strips run the circulation of the first `nrun` members: the two launch orders and which form runs.
struct StripPlan {
  RowsTask* step_tasks = nullptr;        // one launch per sub-step (greb_step_rows.hip): the launch order on the device ...
  int n_step = 0;
  RowsTask head[kStepHeadTasks] = {};    // ... and its first tasks, passed by value
  CircOrder circ;                        // one launch per call: tasks, flags, abort word (n == 0: not resident as a whole)
  int form = 0;                          // 0 undecided, 1 one launch per sub-step, 2 one launch per call
  float ms_substep = 0.f, ms_call = 0.f; // the trial: three model steps of each form
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

void free_plan(StripPlan& p) {
  if (p.step_tasks) (void)hipFree(p.step_tasks);
  circ_rows_free_order(&p.circ);
  for (hipEvent_t ev : p.ev) if (ev) (void)hipEventDestroy(ev);
  p = StripPlan{};
}

} // namespace

struct greb_engine {
  greb_params p{};
  int nx = 0, ny = 0, np = 0, nm = 0, device = 0;
  bool strict = false;
  unsigned xsw = 0; // sensitivity-experiment switches (GREB_X_*) of every member, where they are uniform
  std::vector<unsigned> h_xsw;    // [nm] each member's switches
  bool xsw_uniform = true;        // all equal: the kernels take `xsw`; else the per-member words on the device
  unsigned* xsw_dev = nullptr;    // [nm], current whenever !xsw_uniform
  float* co2_flux_dev = nullptr;  // [nm] flux-phase CO2 where a member's differs from the engine-wide value (else null)
  int n_phys_sets = 1;            // distinct physics parameter sets among the members (describe)
  bool shared_corr = true; // all members alike (physics, kappa, co2_flux, switches) -> one flux-correction set
  bool fused = true;       // every member has the 96x48 default sub-cycling layout -> fused member kernel
  float *Xa = nullptr, *Xb = nullptr, *red = nullptr, *W2 = nullptr; // any-grid (multi-launch) engine work arrays
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;               // device -> host delivery of a scenario run's output units (run_years)
  hipEvent_t ev_done[2] = {nullptr, nullptr};      // a unit is complete in output slot i (compute stream)
  hipEvent_t ev_free[2] = {nullptr, nullptr};      // output slot i is copied out (copy stream)
  // device
  float *z_topo = nullptr, *glacier = nullptr, *sw_solar = nullptr;
  float *tclim = nullptr, *qclim = nullptr, *uclim = nullptr, *vclim = nullptr, *mldclim = nullptr,
        *cldclim = nullptr, *swetclim = nullptr;
  float *toclim = nullptr, *z_ocean = nullptr, *wz_air = nullptr, *wz_vapor = nullptr;
  float *state = nullptr, *acc = nullptr, *corr = nullptr;
  int *corr_index = nullptr, *tab_index = nullptr;
  RowTables* tabs = nullptr;
  Phys* phys = nullptr;
  float* co2_dev = nullptr; size_t co2_cap = 0;
  float* monthly_dev = nullptr; size_t monthly_cap = 0;
  float* bsum = nullptr;                               // run_budget: [nm][GREB_NBUDGET][np] running sums, made on the first budget run
  float* budget_dev = nullptr; size_t budget_cap = 0;  // run_budget: two one-year staging slots of budget records
  long long budget_runs = 0;                           // run_budget calls so far (describe)
  // per-member forcing (set_forcing_tables, set_member_forcing): scenario phase only
  int n_patterns = 0, n_solar = 0;
  float *f_space = nullptr, *f_season = nullptr, *f_solar = nullptr; // [n_patterns][np], [n_patterns][730], [n_solar][730][ny]
  std::vector<greb_member_forcing> h_force;            // [nm], or empty: no member forcing set
  MemberForcing* force_dev = nullptr;                  // [nm], current whenever forced_members > 0
  int forced_members = 0;                              // members that name a pattern or a table or scale the insolation
  // boundary sets (add_boundary_set, set_member_boundary): both phases
  struct BoundSet {
    float* dev[kBoundaryFields] = {};    // the set's thirteen device arrays in BoundarySet's order: its own or the engine's
    bool own[kBoundaryFields] = {};      // which of them this set allocated
    unsigned over = 0;                   // bit i: input field i (< kBoundaryInputs) is overridden
    float* frec = nullptr;               // the set's forcing record (greb_kernels.h), kFrBytes; FAST fused engine only
    // what the initial state is made of (:190-197), np floats each: tclim[729], qclim[729], toclim, z_topo, mldclim[0]
    std::vector<float> t_last, q_last, toclim, z_topo, mld0;
  };
  std::vector<BoundSet> bound;                         // [1 + sets made]; [0]: the engine's own data
  std::vector<int> h_bset;                             // [nm] each member's set, or empty: every member 0
  int members_on_sets = 0;                             // members that name a set above 0
  BoundarySet* bsets_dev = nullptr;                    // the set table (greb_kernels.h: kSetTableBytes), made with the engine where it
                                                       // keeps forcing records, else with the first set
  int* bset_dev = nullptr;                             // [nm], current whenever members_on_sets > 0
  MemberForcing* neutral_force_dev = nullptr;          // [nm] {-1, ., -1, 1}: what a BOUND scenario launch takes when no member is forced
  float* yearly_dev = nullptr; size_t yearly_cap = 0;
  float* diag_out = nullptr; size_t diag_out_cap = 0; // run_diag: zonal means and annual maps of two years (one per staging slot)
  float* diag_reg = nullptr; size_t diag_reg_cap = 0; // run_diag: the region series of the whole call
  float* clim_out = nullptr; size_t clim_out_cap = 0; // run_clim: the products of two periods (one per output slot)
  float* ens_out = nullptr; size_t ens_out_cap = 0;   // run_ens: the group statistics of two years (one per output slot)
  // host copies needed later
  std::vector<RowTables> h_tabs;
  std::vector<int> h_tab_index;
  bool strips = false;                                      // 384- or 192-wide grid on the row strips (greb_step_strip.h)
  enum { kCallNever, kCallTrial, kCallAlways } call = kCallNever; // the circulation call in ONE launch (greb_circ_rows.hip):
                                                            // never (GREB_F_NO_PERSISTENT), where the trial finds it
                                                            // faster, or wherever it can run (GREB_F_PERSISTENT)
  int cus = 0;                                              // compute units of the device (4 SIMDs each)
  int slots_granted = -1;                                   // wavefront slots of the device this engine may fill (-1: not asked yet)
  std::map<int, StripPlan> plans;                           // how the strips run, per number of members run
  std::vector<Phys> h_phys;
  // model clock
  long long it_flux = 0; // steps done in the flux phase
  long long it_scnr = 0; // steps done in the scenario
  unsigned long long* stamps = nullptr; // -DGREB_TUNING builds only: device buffer for the member kernel's stamps
  std::string last_error;
};

namespace {
int fail(greb_engine* e, int code, const std::string& msg) {
  if (e) e->last_error = msg;
  g_last_error = msg;
  return code;
}

int nsub_of(const greb_params& p) {
  int t = nint_f((float)p.dt / (float)p.dt_crcl); // :543
  return t < 1 ? 1 : t;
}

MemberArgs base_args(greb_engine* e) {
  MemberArgs a{};
  a.nx = e->nx; a.ny = e->ny; a.np = e->np;
  a.z_topo = e->z_topo; a.glacier = e->glacier; a.sw_solar = e->sw_solar;
  a.tclim = e->tclim; a.qclim = e->qclim; a.uclim = e->uclim; a.vclim = e->vclim;
  a.mldclim = e->mldclim; a.cldclim = e->cldclim; a.swetclim = e->swetclim;
  a.toclim = e->toclim; a.z_ocean = e->z_ocean; a.wz_air = e->wz_air; a.wz_vapor = e->wz_vapor;
  a.state = e->state; a.acc = e->acc; a.corr = e->corr; a.corr_index = e->corr_index;
  a.tabs = e->tabs; a.tab_index = e->tab_index; a.phys = e->phys;
  a.nsub = nsub_of(e->p);
  a.nsub = tuning_int("GREB_DEBUG_NSUB", a.nsub); // -DGREB_TUNING builds only
  a.co2_flux = e->p.co2_flux;
  a.ipx = e->p.ipx; a.ipy = e->p.ipy;
  a.xsw = e->xsw_uniform ? e->xsw : 0u;
  a.xsw_m = e->xsw_uniform ? nullptr : e->xsw_dev;
  a.co2_flux_m = e->co2_flux_dev;
  a.stamps = e->stamps;
  a.dbg = tuning_int("GREB_DEBUG_PHYS", 0);
  // no transport at all where EVERY member is without circulation: the tracers come back unchanged.  A member without
  // it beside members with it does zero sub-steps of its own (fused kernel) or drops its increments (point physics).
  unsigned all = GREB_X_NO_CIRCULATION;
  for (unsigned x : e->h_xsw) all &= x;
  if (all) a.nsub = 0;
  // a member on a boundary set: the launch carries the set table and takes the boundary-aware kernels
  if (e->members_on_sets > 0) { a.bsets = e->bsets_dev; a.bset_m = e->bset_dev; }
  else if (e->bound[0].frec) a.bsets = e->bsets_dev; // the FAST fused member kernel finds its forcing record behind the set table
  return a;
}

// scenario launches only: with a forced member the launch carries the forcing and takes the forcing-aware kernels
void apply_forcing(const greb_engine* e, MemberArgs& a) {
  // (the boundary-aware scenario kernels are forcing-aware: without a forced member they get words that force nothing)
  if (e->forced_members <= 0 && e->members_on_sets > 0) a.force_m = e->neutral_force_dev;
  if (e->forced_members <= 0) return;
  a.force_m = e->force_dev;
  a.f_space = e->f_space; a.f_season = e->f_season; a.f_solar = e->f_solar;
}

// Where a scenario year's records go: year mon_y of mon_years in `mon` and, where the run has a budget, its budget
// records to year bud_y of bud_years in `bud`.
struct YearOut {
  float* mon; int mon_years, mon_y;
  float* bud = nullptr; int bud_years = 0, bud_y = 0;
};

// Scenario year y of a run of `years` (run_years), its records going to `o`.
MemberArgs scenario_args(greb_engine* e, int years, int y, const YearOut& o) {
  MemberArgs a = base_args(e);
  a.flux_phase = 0;
  a.it0 = e->it_scnr + 1 + (long long)y * kNT; a.nsteps = kNT;
  a.co2 = e->co2_dev; a.co2_stride = years; a.co2_year0 = y;
  a.monthly = o.mon; a.monthly_years = o.mon_years; a.year_out0 = o.mon_y;
  a.yearly = e->yearly_dev; a.yearly_years = years; a.yearly_year0 = y;
  if (o.bud) { a.bsum = e->bsum; a.brec = o.bud; a.brec_years = o.bud_years; a.brec_year0 = o.bud_y; }
  apply_forcing(e, a);
  return a;
}

bool is_forced(const greb_member_forcing& f) { return f.co2_pattern >= 0 || f.solar_table >= 0 || !(f.solar_scale == 1.f); }

// vapour diffused but not advected (GREB_X_VAPOR_DIFFUSION_ONLY): on the any-grid engine a property of the launch, so
// every member has it or none (checked where switches are set)
bool calm_vapor(const greb_engine* e) { return (e->h_xsw[0] & GREB_X_VAPOR_DIFFUSION_ONLY) != 0; }

// the transport kernels of the any-grid engine run all members of a launch alike
int check_transport_switches(greb_engine* e, const char* who, bool fused, const unsigned* sw, int n) {
  if (fused) return 0;
  for (int m = 1; m < n; ++m)
    if ((sw[m] ^ sw[0]) & GREB_X_VAPOR_DIFFUSION_ONLY)
      return fail(e, GREB_E_UNSUPPORTED,
                  std::string(who) + ": member " + std::to_string(m) + " differs from member 0 in GREB_X_VAPOR_DIFFUSION_ONLY, "
                  "which the any-grid engine applies to a whole launch -- run the two groups as two engines beside each "
                  "other (ensemble.run_beside)");
  return 0;
}

bool all_equal(const unsigned* sw, int n) {
  for (int m = 1; m < n; ++m) if (sw[m] != sw[0]) return false;
  return true;
}

// the greb_params fields that feed data shared by every member (row-table geometry, wz_air / wz_vapor, the clock)
int check_member_config(const char* who, const greb_params& p, const greb_member_config& c, int m) {
  const char* bad = nullptr;
  auto differ = [](float a, float b) { return std::memcmp(&a, &b, sizeof(float)) != 0; }; // (bitwise: a NaN equals itself)
  if (differ(c.p.pi, p.pi)) bad = "pi";
  else if (differ(c.p.z_air, p.z_air)) bad = "z_air";
  else if (differ(c.p.z_vapor, p.z_vapor)) bad = "z_vapor";
  else if (c.p.dt != p.dt) bad = "dt";
  else if (c.p.dt_crcl != p.dt_crcl) bad = "dt_crcl";
  else if (c.p.ipx != p.ipx) bad = "ipx";
  else if (c.p.ipy != p.ipy) bad = "ipy";
  else if (c.p.year0 != p.year0) bad = "year0";
  if (bad)
    return fail(nullptr, GREB_E_INVALID, std::string(who) + ": member " + std::to_string(m) + ": " + bad +
                                             " differs from the engine-wide greb_params (it feeds data every member shares)");
  if (c.switches & ~0xffu)
    return fail(nullptr, GREB_E_INVALID, std::string(who) + ": member " + std::to_string(m) + ": unknown switch bits");
  return 0;
}

int ensure(greb_engine* e, float** buf, size_t* cap, size_t n) {
  if (*cap >= n) return 0;
  if (*buf) HIP_TRY(e, hipFree(*buf));
  *buf = nullptr; *cap = 0;
  HIP_TRY(e, dev_alloc(buf, n));
  *cap = n;
  return 0;
}

// The wavefront slots of a device that one-launch circulation calls may fill, across the engines of this process.
// Such a launch waits inside the kernel for its own tasks, so all of them must be resident at once; two engines driven
// side by side (ensemble.run_beside: config 5's 62 + 2 members) share the device, and the sum of what they launch must fit.
// Every engine that may take the one-launch form registers with its member count when it is created; an engine's grant
// is fixed the first time it needs one: its share of the slots by members among the engines registered then, and never
// more than what the grants already made leave.  An engine that gets too little for its tasks takes one launch per
// sub-step, which waits for nothing.  (Another PROCESS on the same device is outside this ledger: there the bounded
// waits turn a launch that is not co-resident into an error, never a hang.)
struct SlotLedger {
  std::mutex mu;
  struct Entry { greb_engine* e; int device, members, granted; };
  std::vector<Entry> entries;
} g_slots;

void ledger_register(greb_engine* e) {
  std::lock_guard<std::mutex> lock(g_slots.mu);
  g_slots.entries.push_back({e, e->device, e->nm, 0});
}
void ledger_release(greb_engine* e) {
  std::lock_guard<std::mutex> lock(g_slots.mu);
  for (size_t i = 0; i < g_slots.entries.size(); ++i)
    if (g_slots.entries[i].e == e) { g_slots.entries.erase(g_slots.entries.begin() + (long)i); break; }
}
int ledger_grant(greb_engine* e, int device_slots) {
  std::lock_guard<std::mutex> lock(g_slots.mu);
  long long members = 0, taken = 0;
  SlotLedger::Entry* mine = nullptr;
  for (auto& x : g_slots.entries) {
    if (x.device != e->device) continue;
    members += x.members;
    if (x.e == e) mine = &x; else taken += x.granted;
  }
  if (!mine) return 0;
  const long long share = (long long)device_slots * mine->members / std::max<long long>(1, members);
  mine->granted = (int)std::max<long long>(0, std::min<long long>(share, device_slots - taken));
  return mine->granted;
}

// after the stream has been synchronised: did a one-launch circulation call give up waiting?
int check_circulation(greb_engine* e) {
  for (auto& kv : e->plans) {
    unsigned d[5] = {0, 0, 0, 0, 0};
    const int rc = circ_rows_status(kv.second.circ, d);
    if (rc == -1) {
      char buf[384];
      std::snprintf(buf, sizeof(buf),
                    "circulation launch given up: task %u waited more than %.1f s in sub-step %u for a neighbouring strip "
                    "(its count read %u, wanted %u) -- the launch was not resident as a whole (another process on the "
                    "device?); results are invalid, recreate the engine with GREB_F_NO_PERSISTENT",
                    d[0], kCircSpinTicks / 1e8, d[1], d[2], d[3]);
      return fail(e, GREB_E_STATE, buf);
    }
    if (rc) return fail(e, GREB_E_STATE, "circulation launch: status word unreadable");
  }
  return 0;
}

// The row strips' plan for `nrun` members: both launch orders where the form is still to be measured, the one that runs
// where it is not.  Made the first time a year of that many members runs; nothing of it is host work per model step.
int make_strip_plan(greb_engine* e, int nrun, StripPlan& p) {
  if (e->cus <= 0) HIP_TRY(e, hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, e->device));
  // the whole circulation call (its nsub sub-steps) in ONE launch where every task of it can be resident at once ...
  if (e->call != greb_engine::kCallNever) {
    static const int slots_per_cu = tuning_int("GREB_CIRC_SLOTS_PER_CU", kStepRowsSlotsPerCu); // -DGREB_TUNING builds only (occupancy experiments: <= 8)
    if (e->slots_granted < 0) e->slots_granted = ledger_grant(e, e->cus * std::min(slots_per_cu, kStepRowsSlotsPerCu));
    HIP_TRY(e, circ_rows_make_order(e->h_tabs.data(), e->h_tab_index.data(), nrun, e->ny, e->slots_granted, &p.circ));
  }
  p.form = p.circ.n == 0 ? 1 : (e->call == greb_engine::kCallAlways ? 2 : 0); // (n == 0: the grant is too small for this many fields)
  // ... else one launch per sub-step
  if (p.form != 2) {
    static const int step_slots = tuning_int("GREB_STEP_SLOTS_PER_CU", kStepRowsSlotsPerCu); // -DGREB_TUNING builds only (occupancy experiments)
    HIP_TRY(e, step_rows_make_tasks(e->h_tabs.data(), e->h_tab_index.data(), nrun, e->ny, e->cus * step_slots, &p.step_tasks,
                                    &p.n_step, p.head));
  }
  if (p.form == 0)
    for (hipEvent_t& ev : p.ev) HIP_TRY(e, hipEventCreate(&ev));
  return 0;
}

// One model year (730 steps) for the first `nrun` members, `a` describing that year.
//   fused layout : one launch of the member kernel
//   other grids  : 24 fused band sub-steps + 1 point-physics launch per model step
//   row strips   : the 24 sub-steps in one launch or one launch each (StripPlan) + 1 point-physics launch per model step
int run_year(greb_engine* e, const MemberArgs& a, int nrun) {
  if (e->fused) {
    HIP_TRY(e, launch_member_kernel(a, nrun, e->strict, e->stream));
    return 0;
  }
  const size_t np = (size_t)e->np;
  StripPlan* plan = nullptr;
  if (e->strips && a.nsub > 0) {
    auto it = e->plans.find(nrun);
    if (it == e->plans.end()) {
      StripPlan p;
      if (int rc = make_strip_plan(e, nrun, p)) { free_plan(p); return rc; }
      it = e->plans.emplace(nrun, p).first;
    }
    plan = &it->second;
  }
  // Which of the two wins depends on how many fields there are and what shares a SIMD with what (one member: 15.1 against
  // 18.7 us per sub-step; 40 members: 29.6 against 25.8; 62: 36.0 against 38.7), and the two are bit-identical row by
  // row (tests/test_gpu_parity.py), so the engine MEASURES: the first eight model steps of the first year run two warm-up
  // steps, three timed steps of one form and three of the other between events on its own stream, and the faster form
  // runs from then on.  The results do not depend on the choice.
  static const int steps = tuning_int("GREB_DEBUG_NSTEPS", kNT); // -DGREB_TUNING builds only: a short stretch for counter passes
  bool trial = plan && plan->form == 0 && steps >= 16;
  int form = plan && plan->form != 1 ? 2 : 1; // (undecided without a trial: one launch per call)
  HIP_TRY(e, launch_pack_tracers(e->state, e->Xa, e->np, nrun, e->stream));
  for (int s = 0; s < steps; ++s) {
    const long long it = a.it0 + s;
    const int ityr = (int)((it - 1) % kNT) + 1;
    const size_t off = (size_t)(ityr - 1) * np;
    float *cur = e->Xa, *nxt = e->Xb;
    if (trial) { // steps 0-1 warm up, 2-4 one launch per sub-step, 5-7 one launch per call
      if (s == 2 || s == 5 || s == 8) HIP_TRY(e, hipEventRecord(plan->ev[s == 2 ? 0 : (s == 5 ? 1 : 2)], e->stream));
      if (s == 8) {
        HIP_TRY(e, hipEventSynchronize(plan->ev[2]));
        HIP_TRY(e, hipEventElapsedTime(&plan->ms_substep, plan->ev[0], plan->ev[1]));
        HIP_TRY(e, hipEventElapsedTime(&plan->ms_call, plan->ev[1], plan->ev[2]));
        form = plan->form = plan->ms_call <= plan->ms_substep ? 2 : 1;
        trial = false;
      } else form = (s >= 2 && s < 5) ? 1 : 2;
    }
    if (form == 2) {
      HIP_TRY(e, launch_circulation_rows(e->Xa, e->Xb, e->W2, e->uclim + off, e->vclim + off, e->tabs, plan->circ, e->cus * 4, e->nx, e->ny,
                                         a.nsub, e->strict, e->stream, calm_vapor(e)));
      if (a.nsub & 1) cur = e->Xb;
    } else
    for (int tt = 0; tt < a.nsub; ++tt) {
      if (plan)
        HIP_TRY(e, launch_substep_rows(cur, e->W2, e->uclim + off, e->vclim + off, nxt, e->tabs, e->tab_index, plan->step_tasks,
                                       plan->head, plan->n_step, e->cus * 4, e->nx, e->ny, e->strict, e->stream, calm_vapor(e)));
      else
        HIP_TRY(e, launch_substep_fused(cur, e->W2, e->uclim + off, e->vclim + off, nxt, e->tabs, e->tab_index, e->nx,
                                        e->ny, nrun, e->strict, e->stream, calm_vapor(e)));
      float* t = cur; cur = nxt; nxt = t;
    }
    MemberArgs b = a;
    b.it0 = it; b.nsteps = 1; // the step kernel derives its clock from it0; year indices are those of `a`
    HIP_TRY(e, launch_physics_step(b, cur, e->Xa, e->red, nrun, e->strict, e->stream));
    if (ityr == kNT && a.yearly)
      HIP_TRY(e, launch_yearly(e->red, a.yearly, e->np, e->nx, a.ipx, a.ipy, a.yearly_years, a.yearly_year0, nrun, e->strict, e->stream));
  }
  return 0;
}
} // namespace

extern "C" {

void greb_params_default(greb_params* p) {
  // src/greb.f90:49-53, 68-104; constant expressions folded in fp32 like the compiler does
  std::memset(p, 0, sizeof(*p));
  p->pi = 3.1416f; p->sig = 5.6704e-8f; p->rho_ocean = 999.1f; p->rho_land = 2600.f; p->rho_air = 1.2f;
  p->cp_ocean = 4186.f; p->cp_land = 926.222f; p->cp_air = 1005.f; p->eps = 1.f;
  p->d_ocean = 50.f; p->d_land = 2.f; p->d_air = 5000.f; p->ct_sens = 22.5f; p->da_ice = 0.25f;
  p->a_no_ice = 0.1f; p->a_cloud = 0.35f;
  p->Tl_ice1 = 273.15f - 10.f; p->Tl_ice2 = 273.15f; p->To_ice1 = 273.15f - 7.f; p->To_ice2 = 273.15f - 1.7f;
  p->co_turb = 5.0f; p->kappa = 8e5f; p->ce = 2e-3f; p->cq_latent = 2.257e6f;
  p->cq_rain = -0.1f / 24.f / 3600.f; p->z_air = 8400.f; p->z_vapor = 5000.f; p->r_qviwv = 2.6736e3f;
  const float pe[10] = {9.0721f, 106.7252f, 61.5562f, 0.0179f, 0.0028f, 0.0570f, 0.3462f, 2.3406f, 0.7032f, 1.0662f};
  std::memcpy(p->p_emi, pe, sizeof(pe));
  p->co2_flux = 298.f;
  p->ipx = 1; p->ipy = 1; p->year0 = 1940; p->dt = 12 * 3600; p->dt_crcl = 1800;
}

const char* greb_engine_last_error(const greb_engine* e) {
  return e ? e->last_error.c_str() : g_last_error.c_str();
}

const char* greb_device_info(int device) {
  static thread_local std::string s;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) {
    s = "{\"error\": \"no HIP device\"}";
    return s.c_str();
  }
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, device) != hipSuccess) { s = "{\"error\": \"hipGetDeviceProperties\"}"; return s.c_str(); }
  char buf[512];
  std::snprintf(buf, sizeof(buf),
                "{\"name\": \"%s\", \"arch\": \"%s\", \"cus\": %d, \"clock_mhz\": %d, \"mem_clock_mhz\": %d, "
                "\"hbm_gb\": %.1f, \"lds_per_block\": %zu, \"l2_mb\": %.1f, \"wave\": %d}",
                pr.name, pr.gcnArchName, pr.multiProcessorCount, pr.clockRate / 1000, pr.memoryClockRate / 1000,
                pr.totalGlobalMem / 1073741824.0, pr.sharedMemPerBlock, pr.l2CacheSize / 1048576.0, pr.warpSize);
  s = buf;
  return s.c_str();
}

} // extern "C"

namespace {
// The derived fields of greb_model's preamble (host, once per engine and per boundary set that replaces their source):
// Toclim :1088-1094 from tclim, z_ocean :179-183 from mldclim, wz_air / wz_vapor :201-202 from z_topo.  A null source
// leaves its outputs alone.
void derive_fields(const greb_params& p, size_t np, const float* z_topo, const float* tclim, const float* mldclim, float* toclim,
                   float* z_ocean, float* wz_air, float* wz_vapor) {
  for (size_t i = 0; i < np; ++i) {
    if (tclim) {
      float mn = tclim[i];
      for (int t = 0; t < kNT; ++t) { const float v = tclim[(size_t)t * np + i]; if (v < mn) mn = v; }
      if (mn - 273.15f < -1.7f) mn = -1.7f + 273.15f;
      toclim[i] = mn;
    }
    if (mldclim) {
      float mx = 0.f;
      for (int t = 0; t < kNT; ++t) { const float d = mldclim[(size_t)t * np + i]; if (d > mx) mx = d; }
      z_ocean[i] = 3.0f * mx;
    }
    if (z_topo) {
      wz_air[i] = expf(-z_topo[i] / p.z_air);
      wz_vapor[i] = expf(-z_topo[i] / p.z_vapor);
    }
  }
}

// the initial state of one member (:194-197) and its initial cap_surf (:190-191) on the data of one boundary set
void initial_state(const greb_engine::BoundSet& b, const Phys& P, size_t np, float* st) {
  for (size_t i = 0; i < np; ++i) {
    st[i] = b.t_last[i]; st[np + i] = st[i]; st[2 * np + i] = b.toclim[i]; st[3 * np + i] = b.q_last[i];
    float c = 0.f;
    if (b.z_topo[i] > 0.f) c = P.cap_land;
    if (b.z_topo[i] <= 0.f) c = P.cap_ocean * b.mld0[i];
    st[4 * np + i] = c;
  }
}

const char* const kBoundaryNames[kBoundaryFields] = {"z_topo", "glacier", "tclim", "qclim", "uclim", "vclim", "mldclim", "cldclim",
                                                     "swetclim", "toclim", "z_ocean", "wz_air", "wz_vapor"};
enum { kBfZtopo, kBfGlacier, kBfTclim, kBfQclim, kBfUclim, kBfVclim, kBfMld, kBfCld, kBfSwet, kBfToclim, kBfZocean, kBfWzAir, kBfWzVapor };
size_t boundary_floats(int field, size_t np) { return (field >= kBfTclim && field <= kBfSwet) ? np * kNT : np; }

BoundarySet set_entry(const greb_engine::BoundSet& x) {
  return BoundarySet{x.dev[0], x.dev[1], x.dev[2], x.dev[3], x.dev[4], x.dev[5], x.dev[6], x.dev[7], x.dev[8], x.dev[9], x.dev[10],
                     x.dev[11], x.dev[12]};
}
// The FAST fused member kernel reads boundary data from one packed record per set (greb_kernels.h: forcing record).
bool uses_forcing_records(const greb_engine* e) { return e->fused && !e->strict; }
// The record of set `b`, whose arrays are on the device: made there, on the engine's stream -- ahead of every launch that
// reads it -- and entered into slot `id` of the record pointers behind the set table.  On failure nothing is left behind
// and *what names the step.
hipError_t make_forcing_record(greb_engine* e, const greb_engine::BoundSet& b, BoundarySet* table, size_t id, float** rec,
                               const char** what) {
  *rec = nullptr;
  *what = "hipMalloc of the set's forcing record";
  hipError_t err = dev_alloc(rec, kFrBytes / sizeof(float));
  if (err != hipSuccess) { *rec = nullptr; return err; }
  *what = "packing the set's forcing record";
  err = launch_pack_forcing(set_entry(b), *rec, e->stream);
  if (err == hipSuccess) { *what = "hipMemcpy"; err = hipMemcpy(set_table_records(table) + id, rec, sizeof(float*), hipMemcpyHostToDevice); }
  if (err != hipSuccess) { (void)hipStreamSynchronize(e->stream); (void)hipFree(*rec); *rec = nullptr; }
  return err;
}

// An engine whose members share one flux-correction set gives every member a copy of it -- on a NEW buffer: the engine is
// untouched, and the caller frees the buffer if anything later fails.
hipError_t copy_shared_corrections(greb_engine* e, float** corr, const char** what) {
  const size_t nm = (size_t)e->nm, set = (size_t)3 * kNT * e->np;
  hipError_t err = hipStreamSynchronize(e->stream);
  *what = "hipStreamSynchronize";
  if (err != hipSuccess) return err;
  *what = "hipMalloc of the members' correction sets";
  if ((err = dev_alloc(corr, nm * set)) != hipSuccess) return err;
  *what = "hipMemcpy";
  for (size_t m = 0; m < nm; ++m)
    if ((err = hipMemcpy(*corr + m * set, e->corr, set * sizeof(float), hipMemcpyDeviceToDevice)) != hipSuccess) return err;
  return hipSuccess;
}
// The engine takes them: its correction index -- one small copy, the LAST step of a call that can fail -- then the buffer.
hipError_t adopt_member_corrections(greb_engine* e, float* corr) {
  std::vector<int> corr_index((size_t)e->nm);
  for (int m = 0; m < e->nm; ++m) corr_index[(size_t)m] = m;
  hipError_t err = hipMemcpy(e->corr_index, corr_index.data(), corr_index.size() * sizeof(int), hipMemcpyHostToDevice);
  if (err != hipSuccess) return err;
  (void)hipFree(e->corr);
  e->corr = corr;
  e->shared_corr = false;
  return hipSuccess;
}

// greb_engine_create_members, and greb_engine_create through it (`who` names the entry in messages)
int create_engine(const char* who, const greb_params* p, int nx, int ny, const greb_fields* f, int n_members,
                  const greb_member_config* members, int device, unsigned flags, greb_engine** out) {
  if (!p || !f || !out || !members || n_members < 1 || nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy)
    return fail(nullptr, GREB_E_INVALID, std::string(who) + ": bad argument");
  for (int m = 0; m < n_members; ++m)
    if (int rc = check_member_config(who, *p, members[m], m)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
    return fail(nullptr, GREB_E_NOGPU, std::string(who) + ": no HIP device (the engine has no CPU path)");
  bool fused = true;
  std::vector<unsigned> switches((size_t)n_members);
  for (int m = 0; m < n_members; ++m) {
    RowTables t; compute_row_tables(*p, members[m].p.kappa, nx, ny, t);
    fused = fused && member_layout_supported(t, nx, ny);
    switches[(size_t)m] = members[m].switches;
  }
  fused = fused && !(flags & GREB_F_MULTILAUNCH);
  if (p->ipx < 1 || p->ipx > nx || p->ipy < 1 || p->ipy > ny)
    return fail(nullptr, GREB_E_INVALID, std::string(who) + ": ipx/ipy outside the grid");
  if (int rc = check_transport_switches(nullptr, who, fused, switches.data(), n_members)) return rc;
  greb_engine* e = new (std::nothrow) greb_engine();
  if (!e) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  *out = e; // returned even on failure so last_error can be read; caller destroys
  e->p = *p; e->nx = nx; e->ny = ny; e->np = nx * ny; e->nm = n_members; e->device = device;
  e->strict = (flags & GREB_F_STRICT) != 0;
  e->fused = fused;
  e->h_xsw = switches;
  e->xsw_uniform = all_equal(switches.data(), n_members);
  e->xsw = e->xsw_uniform ? switches[0] : 0u;
  const size_t np = (size_t)e->np, n3 = np * kNT, nm = (size_t)n_members;
  HIP_TRY(e, hipSetDevice(device));
  HIP_TRY(e, hipStreamCreate(&e->stream));

  auto up = [&](float** d, const float* h, size_t n) -> hipError_t {
    hipError_t err = dev_alloc(d, n);
    if (err != hipSuccess) return err;
    return hipMemcpy(*d, h, n * sizeof(float), hipMemcpyHostToDevice);
  };
  HIP_TRY(e, up(&e->z_topo, f->z_topo, np));
  HIP_TRY(e, up(&e->glacier, f->glacier, np));
  HIP_TRY(e, up(&e->sw_solar, f->sw_solar, (size_t)kNT * ny));
  HIP_TRY(e, up(&e->tclim, f->tclim, n3));
  HIP_TRY(e, up(&e->qclim, f->qclim, n3));
  HIP_TRY(e, up(&e->uclim, f->uclim, n3));
  HIP_TRY(e, up(&e->vclim, f->vclim, n3));
  HIP_TRY(e, up(&e->mldclim, f->mldclim, n3));
  HIP_TRY(e, up(&e->cldclim, f->cldclim, n3));
  HIP_TRY(e, up(&e->swetclim, f->swetclim, n3));

  // derived fields (host, once): Toclim :1088-1094, z_ocean :179-183, wz_* :201-202
  std::vector<float> toclim(np), z_ocean(np), wz_air(np), wz_vapor(np);
  derive_fields(*p, np, f->z_topo, f->tclim, f->mldclim, toclim.data(), z_ocean.data(), wz_air.data(), wz_vapor.data());
  HIP_TRY(e, up(&e->toclim, toclim.data(), np));
  HIP_TRY(e, up(&e->z_ocean, z_ocean.data(), np));
  HIP_TRY(e, up(&e->wz_air, wz_air.data(), np));
  HIP_TRY(e, up(&e->wz_vapor, wz_vapor.data(), np));
  { // boundary set 0: the engine's own data
    const size_t last = (size_t)(kNT - 1) * np;
    greb_engine::BoundSet b0;
    float* const dev[kBoundaryFields] = {e->z_topo, e->glacier, e->tclim, e->qclim, e->uclim, e->vclim, e->mldclim, e->cldclim,
                                         e->swetclim, e->toclim, e->z_ocean, e->wz_air, e->wz_vapor};
    for (int i = 0; i < kBoundaryFields; ++i) b0.dev[i] = dev[i];
    b0.t_last.assign(f->tclim + last, f->tclim + last + np); b0.q_last.assign(f->qclim + last, f->qclim + last + np);
    b0.toclim = toclim; b0.z_topo.assign(f->z_topo, f->z_topo + np); b0.mld0.assign(f->mldclim, f->mldclim + np);
    e->bound.push_back(std::move(b0));
  }
  if (uses_forcing_records(e)) { // the forcing record of the engine's own data; an allocation failure is an engine error
    const BoundarySet own = set_entry(e->bound[0]);
    HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(&e->bsets_dev), kSetTableBytes));
    HIP_TRY(e, hipMemset(e->bsets_dev, 0, kSetTableBytes));
    HIP_TRY(e, hipMemcpy(e->bsets_dev, &own, sizeof(own), hipMemcpyHostToDevice));
    const char* what = "";
    const hipError_t err = make_forcing_record(e, e->bound[0], e->bsets_dev, 0, &e->bound[0].frec, &what);
    if (err != hipSuccess) return fail(e, (int)err, std::string(who) + ": " + what + ": " + hipGetErrorString(err));
  }

  // per-member physics, grid tables (deduplicated by kappa), correction-set mapping
  e->h_phys.resize(nm);
  std::vector<int> tab_index(nm), corr_index(nm);
  std::vector<float> kappas;
  e->shared_corr = true;
  std::vector<float> co2_flux(nm);
  bool own_co2_flux = false;
  std::vector<size_t> phys_sets; // first member of every distinct physics set
  for (size_t m = 0; m < nm; ++m) {
    e->h_phys[m] = make_phys(members[m].p);
    const float kap = members[m].p.kappa;
    co2_flux[m] = members[m].p.co2_flux;
    own_co2_flux = own_co2_flux || !(co2_flux[m] == p->co2_flux);
    size_t ps = 0;
    for (; ps < phys_sets.size(); ++ps) if (!std::memcmp(&e->h_phys[phys_sets[ps]], &e->h_phys[m], sizeof(Phys))) break;
    if (ps == phys_sets.size()) phys_sets.push_back(m);
    size_t ti = 0;
    for (; ti < kappas.size(); ++ti) if (kappas[ti] == kap) break;
    if (ti == kappas.size()) {
      kappas.push_back(kap);
      RowTables t; compute_row_tables(*p, kap, nx, ny, t);
      e->h_tabs.push_back(t);
    }
    tab_index[m] = (int)ti;
    if (ps != 0 || ti != 0 || !(co2_flux[m] == co2_flux[0]) || switches[m] != switches[0]) e->shared_corr = false;
  }
  e->n_phys_sets = (int)phys_sets.size();
  if (own_co2_flux) {
    HIP_TRY(e, dev_alloc(&e->co2_flux_dev, nm));
    HIP_TRY(e, hipMemcpy(e->co2_flux_dev, co2_flux.data(), nm * sizeof(float), hipMemcpyHostToDevice));
  }
  if (!e->xsw_uniform) {
    HIP_TRY(e, dev_alloc(&e->xsw_dev, nm));
    HIP_TRY(e, hipMemcpy(e->xsw_dev, switches.data(), nm * sizeof(unsigned), hipMemcpyHostToDevice));
  }
  for (size_t m = 0; m < nm; ++m) corr_index[m] = e->shared_corr ? 0 : (int)m;
  HIP_TRY(e, dev_alloc(&e->phys, nm));
  HIP_TRY(e, hipMemcpy(e->phys, e->h_phys.data(), nm * sizeof(Phys), hipMemcpyHostToDevice));
  HIP_TRY(e, dev_alloc(&e->tabs, e->h_tabs.size()));
  HIP_TRY(e, hipMemcpy(e->tabs, e->h_tabs.data(), e->h_tabs.size() * sizeof(RowTables), hipMemcpyHostToDevice));
  HIP_TRY(e, dev_alloc(&e->tab_index, nm));
  HIP_TRY(e, hipMemcpy(e->tab_index, tab_index.data(), nm * sizeof(int), hipMemcpyHostToDevice));
  e->h_tab_index = tab_index;
  HIP_TRY(e, dev_alloc(&e->corr_index, nm));
  HIP_TRY(e, hipMemcpy(e->corr_index, corr_index.data(), nm * sizeof(int), hipMemcpyHostToDevice));

  const size_t ncorr = e->shared_corr ? 1 : nm;
  HIP_TRY(e, dev_alloc(&e->corr, ncorr * 3 * n3));
  HIP_TRY(e, hipMemset(e->corr, 0, ncorr * 3 * n3 * sizeof(float))); // time_flux = 0 => zero corrections (A.9-10)
  HIP_TRY(e, dev_alloc(&e->acc, nm * 6 * np));
  HIP_TRY(e, hipMemset(e->acc, 0, nm * 6 * np * sizeof(float)));

  // initial state :194-197 and initial cap_surf :190-191
  std::vector<float> st(5 * np);
  HIP_TRY(e, dev_alloc(&e->state, nm * 5 * np));
  for (size_t m = 0; m < nm; ++m) {
    initial_state(e->bound[0], e->h_phys[m], np, st.data());
    HIP_TRY(e, hipMemcpy(e->state + m * 5 * np, st.data(), 5 * np * sizeof(float), hipMemcpyHostToDevice));
  }
  if (!e->fused) { // the member does not fit one CU (or has another sub-cycling layout): multi-launch engine
    HIP_TRY(e, dev_alloc(&e->Xa, nm * 2 * np));
    HIP_TRY(e, dev_alloc(&e->Xb, nm * 2 * np));
    HIP_TRY(e, dev_alloc(&e->red, nm * np));
    HIP_TRY(e, dev_alloc(&e->W2, 2 * np));
    HIP_TRY(e, hipMemcpy(e->W2, wz_air.data(), np * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(e->W2 + np, wz_vapor.data(), np * sizeof(float), hipMemcpyHostToDevice));
    // 384- and 192-wide grids, FAST: the row strips at every member count -- us per launch of the per-sub-step form
    // against the band kernels it replaces (the scalar sweep_kernel<fused> below 28 members, a (Tair,q)-pair band kernel
    // above, round 2): 1 member 23.2 / 25.1, 8: 27.8 / 28.8, 24: 30.0 / 30.5, 40: 35.6 / 35.2, 48: 39.6 / 40.5, 62: 40.8 /
    // 48.0.  STRICT keeps the band kernel (1 member 64.7 against 74.6 us: its two chains per row run one after the other
    // in one wave here); GREB_F_ROW_STRIPS takes the strips there too.
    static const bool no_step_rows = tuning_int("GREB_NO_STEP_ROWS", 0) != 0; // -DGREB_TUNING builds only (A/B)
    e->strips = !no_step_rows && (!e->strict || (flags & GREB_F_ROW_STRIPS)) &&
                n_members < (1 << (kStepFieldBits - 1)) && // (field and table index share a task word)
                step_rows_supported(e->h_tabs.data(), (int)e->h_tabs.size(), nx, ny);
    if (e->strips && !(flags & GREB_F_NO_PERSISTENT)) {
      e->call = (flags & GREB_F_PERSISTENT) ? greb_engine::kCallAlways : greb_engine::kCallTrial;
      ledger_register(e);
    }
  }
  return 0;
}

// ---------------------------------------------------------------- scenario runs: one driver, one sink per output kind
// What the driver shares with greb_engine_flux_correction.  Before the first year of a call: the yearly scalars
// [member][years][2], cleared on the compute stream.
int clear_yearly(greb_engine* e, int years) {
  const size_t n = (size_t)e->nm * years * 2;
  if (int rc = ensure(e, &e->yearly_dev, &e->yearly_cap, n)) return rc;
  HIP_TRY(e, hipMemsetAsync(e->yearly_dev, 0, n * sizeof(float), e->stream));
  return 0;
}
// after the last year of a call is enqueued: wait for it, then ask the one-launch circulation calls whether one gave up
int finish_years(greb_engine* e) {
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return check_circulation(e);
}
int yearly_to_host(greb_engine* e, int years, float* yearly) {
  if (yearly) HIP_TRY(e, hipMemcpy(yearly, e->yearly_dev, (size_t)e->nm * years * 2 * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// staging slot y & 1 of e->monthly_dev: one model year of every member's records, [member][12][5][np]
size_t year_records(const greb_engine* e) { return (size_t)e->nm * 12 * 5 * (size_t)e->np; }
float* staging_slot(const greb_engine* e, int y) { return e->monthly_dev + (size_t)(y & 1) * year_records(e); }

// every member's record (`rec` floats) of unit u, from `dev` to its place in the caller's [member][n][rec] array
hipError_t unit_to_host(greb_engine* e, float* host, int n, int u, const float* dev, size_t rec) {
  return hipMemcpy2DAsync(host + (size_t)u * rec, (size_t)n * rec * sizeof(float), dev, rec * sizeof(float), rec * sizeof(float),
                          (size_t)e->nm, hipMemcpyDeviceToHost, e->copy_stream);
}

// What run_years offers a sink's year().  A UNIT is what leaves for the host in one piece (a year's records, a period's
// climatology): units complete in ascending order from 0, and unit u is made in output slot u & 1.
struct YearCalls {
  std::function<int(int y, const YearOut& o)> integrate; // enqueue scenario year y of every member, its records going to `o`
  // for a sink that delivers:
  std::function<int(int u)> writing;  // what the sink enqueues next writes output slot u & 1, for unit u
  std::function<int(int u)> complete; // everything that makes unit u is enqueued: it may leave
};

// One output kind.  The driver knows nothing about what is delivered, a sink nothing about streams and events.
struct RunSink {
  std::function<int()> prepare;                     // ensure the sink's own device buffers, bring its plan onto the device
  std::function<int(const YearCalls&, int y)> year; // enqueue year y and whatever consumes it
  std::function<int(int u, int slot)> deliver;      // enqueue unit u's copies on e->copy_stream (unit_to_host); empty: nothing
                                                    // leaves for the host, and the run makes no copy stream and no events
  std::function<int()> finish;                      // optional: what is copied after the final sync
};

// `years` scenario years of every member; `s` says what is made of each year and where it goes.  Host delivery: a unit
// leaves over PCIe on the copy stream while the following year integrates on the compute stream (two output slots, one
// event pair each).  A pinned destination makes the copies true DMA; a pageable one is staged by the runtime and still
// overlaps the kernels.
int run_years(greb_engine* e, int years, const float* co2_ppm, float* yearly, const RunSink& s) {
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t nm = (size_t)e->nm;
  if (int rc = ensure(e, &e->co2_dev, &e->co2_cap, nm * years)) return rc;
  HIP_TRY(e, hipMemcpyAsync(e->co2_dev, co2_ppm, nm * years * sizeof(float), hipMemcpyHostToDevice, e->stream));
  if (int rc = clear_yearly(e, years)) return rc;
  const bool delivers = (bool)s.deliver;
  if (delivers) if (int rc = ensure(e, &e->monthly_dev, &e->monthly_cap, 2 * year_records(e))) return rc; // the staging slots
  if (int rc = s.prepare()) { e->last_error = g_last_error; return rc; } // (a plan reports its failure without an engine)
  if (delivers && !e->copy_stream) HIP_TRY(e, hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  for (int i = 0; delivers && i < 2; ++i) {
    if (!e->ev_done[i]) HIP_TRY(e, hipEventCreateWithFlags(&e->ev_done[i], hipEventDisableTiming));
    if (!e->ev_free[i]) HIP_TRY(e, hipEventCreateWithFlags(&e->ev_free[i], hipEventDisableTiming));
  }
  int completed = 0, delivered = 0; // units
  YearCalls calls;
  calls.integrate = [&](int y, const YearOut& o) -> int { return run_year(e, scenario_args(e, years, y, o), e->nm); };
  // called where the SINK's first write to the slot is enqueued, so that nothing before it waits: a year whose records
  // are reduced on the device does not stall its integration on the copy of unit u - 2's small products
  calls.writing = [&](int u) -> int {
    if (u >= 2) HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_free[u & 1], 0)); // the slot's unit u - 2 has left
    return 0;
  };
  calls.complete = [&](int u) -> int {
    HIP_TRY(e, hipEventRecord(e->ev_done[u & 1], e->stream));
    completed = u + 1;
    return 0;
  };
  auto deliver = [&](int u) -> int {
    HIP_TRY(e, hipStreamWaitEvent(e->copy_stream, e->ev_done[u & 1], 0));
    if (int rc = s.deliver(u, u & 1)) return rc;
    HIP_TRY(e, hipEventRecord(e->ev_free[u & 1], e->copy_stream));
    return 0;
  };
  // an error anywhere below must not return while copies into the CALLER's buffers are still in flight (the caller
  // may free them as soon as it sees the error): the body runs in a lambda and both streams are drained on failure
  const int rc_years = [&]() -> int {
    for (int y = 0; y < years; ++y) {
      // what EARLIER years completed leaves AFTER this year's kernels are enqueued, so that even a copy the runtime
      // performs synchronously (pageable destination) runs beside a kernel
      const int before = completed;
      if (int rc = s.year(calls, y)) return rc;
      for (; delivered < before; ++delivered) if (int rc = deliver(delivered)) return rc;
    }
    for (; delivered < completed; ++delivered) if (int rc = deliver(delivered)) return rc;
    if (delivers) HIP_TRY(e, hipStreamSynchronize(e->copy_stream));
    return 0;
  }();
  if (rc_years && delivers) {
    (void)hipStreamSynchronize(e->copy_stream);
    (void)hipStreamSynchronize(e->stream);
  }
  if (rc_years) return rc_years;
  if (int rc = finish_years(e)) return rc;
  e->it_scnr += (long long)years * kNT;
  if (s.finish) if (int rc = s.finish()) return rc;
  return yearly_to_host(e, years, yearly);
}

// The records sink: greb_engine_run (budget == nullptr) and greb_engine_run_budget (budget != nullptr, monthly may be
// nullptr).  A unit is a year: its five records and, with a budget, its budget records.  With a budget the launches take
// the BUDGET instantiations (MemberArgs::bsum set); what they leave in state, clock, monthly and yearly is what the
// default ones leave.
int run_records(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* budget, float* yearly,
                unsigned run_flags) {
  const size_t np = (size_t)e->np, nm = (size_t)e->nm;
  const size_t rec_year = 12 * 5 * np, bud_year = (size_t)12 * GREB_NBUDGET * np; // floats per member-year
  const bool dev_out = (run_flags & GREB_RUN_DEVICE_OUT) != 0;
  auto budget_slot = [&](int y) { return e->budget_dev + (size_t)(y & 1) * nm * bud_year; }; // as staging_slot
  RunSink s;
  s.prepare = [&]() -> int {
    if (!budget) return 0;
    if (!e->bsum) { // zero from here on: every December ends with the sums cleared
      HIP_TRY(e, dev_alloc(&e->bsum, nm * GREB_NBUDGET * np));
      HIP_TRY(e, hipMemsetAsync(e->bsum, 0, nm * GREB_NBUDGET * np * sizeof(float), e->stream));
    }
    ++e->budget_runs;
    if (!dev_out) return ensure(e, &e->budget_dev, &e->budget_cap, 2 * nm * bud_year);
    // (a budget-only run: the kernels write their five records regardless -- into one staging slot nobody reads)
    return monthly ? 0 : ensure(e, &e->monthly_dev, &e->monthly_cap, year_records(e));
  };
  if (dev_out) { // the kernels write the caller's device arrays, [member][years]
    s.year = [&](const YearCalls& run, int y) -> int {
      return run.integrate(y, monthly ? YearOut{monthly, years, y, budget, years, y} : YearOut{e->monthly_dev, 1, 0, budget, years, y});
    };
    return run_years(e, years, co2_ppm, yearly, s);
  }
  // the staging slot IS the output slot: the year's own kernels write it, so here -- and only here -- the year itself
  // waits until the slot's year y - 2 has left
  s.year = [&](const YearCalls& run, int y) -> int {
    if (int rc = run.writing(y)) return rc;
    if (int rc = run.integrate(y, {staging_slot(e, y), 1, 0, budget ? budget_slot(y) : nullptr, 1, 0})) return rc;
    return run.complete(y);
  };
  s.deliver = [&](int y, int sl) -> int {
    if (monthly) HIP_TRY(e, unit_to_host(e, monthly, years, y, staging_slot(e, sl), rec_year));
    if (budget) HIP_TRY(e, unit_to_host(e, budget, years, y, budget_slot(sl), bud_year));
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, s);
}
} // namespace

extern "C" {

int greb_engine_create_members(const greb_params* p, int nx, int ny, const greb_fields* f, int n_members,
                               const greb_member_config* members, int device, unsigned flags, greb_engine** out) {
  return create_engine("greb_engine_create_members", p, nx, ny, f, n_members, members, device, flags, out);
}

// the four override slots expanded into full member configurations: NaN keeps the engine-wide value, no switches
int greb_engine_create(const greb_params* p, int nx, int ny, const greb_fields* f, int n_members,
                       const greb_member_overrides* overrides, int device, unsigned flags, greb_engine** out) {
  if (!p || n_members < 1) return fail(nullptr, GREB_E_INVALID, "greb_engine_create: bad argument");
  std::vector<greb_member_config> members((size_t)n_members);
  auto pick = [](float base, float ov) { return std::isnan(ov) ? base : ov; };
  for (int m = 0; m < n_members; ++m) {
    greb_member_config& c = members[(size_t)m];
    c.p = *p; c.switches = 0;
    if (!overrides) continue;
    c.p.da_ice = pick(p->da_ice, overrides[m].da_ice);
    c.p.a_no_ice = pick(p->a_no_ice, overrides[m].a_no_ice);
    c.p.a_cloud = pick(p->a_cloud, overrides[m].a_cloud);
    c.p.kappa = pick(p->kappa, overrides[m].kappa);
  }
  return create_engine("greb_engine_create", p, nx, ny, f, n_members, members.data(), device, flags, out);
}

int greb_engine_destroy(greb_engine* e) {
  if (!e) return 0;
  (void)hipSetDevice(e->device); // teardown: nothing useful to do with an error here
  void* ptrs[] = {e->z_topo, e->glacier, e->sw_solar, e->tclim, e->qclim, e->uclim, e->vclim, e->mldclim,
                  e->cldclim, e->swetclim, e->toclim, e->z_ocean, e->wz_air, e->wz_vapor, e->state, e->acc,
                  e->corr, e->corr_index, e->tab_index, e->tabs, e->phys, e->co2_dev, e->monthly_dev, e->yearly_dev,
                  e->Xa, e->Xb, e->red, e->W2, e->xsw_dev, e->co2_flux_dev, e->diag_out, e->diag_reg, e->clim_out, e->ens_out, e->bsum, e->budget_dev,
                  e->f_space, e->f_season, e->f_solar, e->force_dev, e->bsets_dev, e->bset_dev, e->neutral_force_dev};
  for (void* q : ptrs) if (q) (void)hipFree(q);
  for (const auto& b : e->bound) if (b.frec) (void)hipFree(b.frec);
  for (size_t k = 1; k < e->bound.size(); ++k)
    for (int i = 0; i < kBoundaryFields; ++i) if (e->bound[k].own[i]) (void)hipFree(e->bound[k].dev[i]);
  for (auto& kv : e->plans) free_plan(kv.second);
  if (e->call != greb_engine::kCallNever) ledger_release(e);
  for (int i = 0; i < 2; ++i) {
    if (e->ev_done[i]) (void)hipEventDestroy(e->ev_done[i]);
    if (e->ev_free[i]) (void)hipEventDestroy(e->ev_free[i]);
  }
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return 0;
}

int greb_engine_flux_correction(greb_engine* e, int years, float* yearly) {
  if (!e || years < 0) return fail(e, GREB_E_INVALID, "flux_correction: bad argument");
  if (years == 0) return 0;
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t np = (size_t)e->np;
  const int nrun = e->shared_corr ? 1 : e->nm; // identical members: integrate one, broadcast
  if (int rc = clear_yearly(e, years)) return rc;
  for (int y = 0; y < years; ++y) {
    MemberArgs a = base_args(e);
    a.flux_phase = 1;
    a.it0 = e->it_flux + 1 + (long long)y * kNT; a.nsteps = kNT;
    a.monthly = nullptr; a.monthly_years = years; a.year_out0 = y;
    a.yearly = e->yearly_dev; a.yearly_years = years; a.yearly_year0 = y;
    if (int rc = run_year(e, a, nrun)) return rc;
  }
  if (e->shared_corr && e->nm > 1) { // the spun-up state (incl. cap_surf) is every member's start (A.8)
    for (int m = 1; m < e->nm; ++m)
      HIP_TRY(e, hipMemcpyAsync(e->state + (size_t)m * 5 * np, e->state, 5 * np * sizeof(float),
                                hipMemcpyDeviceToDevice, e->stream));
  }
  if (int rc = finish_years(e)) return rc;
  e->it_flux += (long long)years * kNT;
  if (int rc = yearly_to_host(e, years, yearly)) return rc;
  if (yearly && e->shared_corr)
    for (int m = 1; m < e->nm; ++m) std::memcpy(yearly + (size_t)m * years * 2, yearly, (size_t)years * 2 * sizeof(float));
  return 0;
}

int greb_engine_run(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* yearly,
                    unsigned run_flags) {
  if (!e || years < 1 || !co2_ppm || !monthly) return fail(e, GREB_E_INVALID, "run: bad argument");
  return run_records(e, years, co2_ppm, monthly, nullptr, yearly, run_flags);
}

int greb_engine_run_budget(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* budget, float* yearly,
                           unsigned run_flags) {
  if (!e || years < 1 || !co2_ppm) return fail(e, GREB_E_INVALID, "run_budget: bad argument (engine, years or co2_ppm)");
  if (!budget) return fail(e, GREB_E_INVALID, "run_budget: `budget` is NULL (greb_engine_run is the run without budget output)");
  return run_records(e, years, co2_ppm, monthly, budget, yearly, run_flags);
}

const char* greb_budget_name(int i) {
  static const char* const names[GREB_NBUDGET] = {"sw", "LW_surf", "LWair_down", "LW_abs", "Q_sens", "Q_lat", "Q_lat_air",
                                                  "dq_eva", "dq_rain", "dT_ocean", "dTo", "dTa_crcl", "dq_crcl"};
  return i >= 0 && i < GREB_NBUDGET ? names[i] : nullptr;
}

} // extern "C"

// ---------------------------------------------------------------- reduced output (greb_diag.hip)
// A plan is host data only: the combined weights w_r * cos(lat_j) of the globe and the caller's regions and the
// reciprocals of their sums, made once in double.  Their device copies (and the scratch array of the per-band partial
// sums) are made per device the first time the plan reduces something there.
struct greb_diag {
  int nx = 0, ny = 0, nr = 0;  // nr = 1 + n_regions
  std::vector<double> w;       // [nr][ny][nx]
  std::vector<double> inv_sum; // [nr]
  struct Dev { int device; double* w; double* inv_sum; double* partials; size_t partials_cap; };
  std::vector<Dev> devs;
};

namespace {
// the plan's tables on `device` (current), with room for the partial sums of `n_members` when regions are reduced
int diag_on_device(greb_diag* d, int device, int n_members, bool regions, greb_diag::Dev** out) {
  greb_diag::Dev* dv = nullptr;
  for (auto& x : d->devs) if (x.device == device) dv = &x;
  if (!dv) {
    greb_diag::Dev n{device, nullptr, nullptr, nullptr, 0};
    HIP_TRY(nullptr, dev_alloc(&n.w, d->w.size()));
    hipError_t err = dev_alloc(&n.inv_sum, d->inv_sum.size());
    if (err == hipSuccess) err = hipMemcpy(n.w, d->w.data(), d->w.size() * sizeof(double), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(n.inv_sum, d->inv_sum.data(), d->inv_sum.size() * sizeof(double), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
      (void)hipFree(n.w);
      if (n.inv_sum) (void)hipFree(n.inv_sum);
      HIP_TRY(nullptr, err);
    }
    d->devs.push_back(n);
    dv = &d->devs.back();
  }
  const size_t need = regions ? diag_partials(d->nx, d->ny, n_members, d->nr) : 0;
  if (dv->partials_cap < need) { // (a larger batch than before: an earlier reduction may still read the old array)
    if (dv->partials) {
      HIP_TRY(nullptr, hipDeviceSynchronize());
      HIP_TRY(nullptr, hipFree(dv->partials));
      dv->partials = nullptr; dv->partials_cap = 0;
    }
    HIP_TRY(nullptr, dev_alloc(&dv->partials, need));
    dv->partials_cap = need;
  }
  *out = dv;
  return 0;
}

DiagArgs diag_args(const greb_diag* d, const greb_diag::Dev* dv, const float* monthly, float* regions, size_t regions_stride,
                   float* zonal, float* annual) {
  DiagArgs a{};
  a.monthly = monthly; a.nx = d->nx; a.ny = d->ny; a.nr = d->nr;
  a.w = dv->w; a.inv_sum = dv->inv_sum; a.partials = dv->partials;
  a.regions = regions; a.regions_stride = regions_stride; a.zonal = zonal; a.annual = annual;
  return a;
}
} // namespace

extern "C" {

int greb_diag_create(int nx, int ny, const float* region_w, int n_regions, greb_diag** out) {
  if (!out) return fail(nullptr, GREB_E_INVALID, "diag_create: `out` is NULL");
  *out = nullptr;
  if (nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy)
    return fail(nullptr, GREB_E_INVALID, "diag_create: grid " + std::to_string(nx) + " x " + std::to_string(ny) +
                                             " (nx % 4 == 0, nx >= 12, 5 <= ny <= " + std::to_string(kMaxNy) + ")");
  if (n_regions < 0 || n_regions > kDiagMaxRegions)
    return fail(nullptr, GREB_E_INVALID, "diag_create: n_regions = " + std::to_string(n_regions) + " (0 ... " +
                                             std::to_string(kDiagMaxRegions) + "; the globe is region 0 on top of them)");
  if (n_regions > 0 && !region_w) return fail(nullptr, GREB_E_INVALID, "diag_create: region_w is NULL with n_regions > 0");
  const size_t np = (size_t)nx * ny;
  for (int k = 0; k < n_regions; ++k)
    for (size_t i = 0; i < np; ++i) {
      const float v = region_w[(size_t)k * np + i];
      if (!(v >= 0.f && v <= 1.f)) { // (a NaN fails both comparisons)
        char buf[160];
        std::snprintf(buf, sizeof(buf), "diag_create: region %d: weight %g at row %zu, column %zu is not in [0, 1]", k + 1,
                      (double)v, i / (size_t)nx, i % (size_t)nx);
        return fail(nullptr, GREB_E_INVALID, buf);
      }
    }
  greb_diag* d = new (std::nothrow) greb_diag();
  if (!d) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  d->nx = nx; d->ny = ny; d->nr = 1 + n_regions;
  d->w.resize((size_t)d->nr * np);
  d->inv_sum.resize((size_t)d->nr);
  const double pi = 3.14159265358979323846; // the true pi: the area of a grid cell, not the model's constant
  for (int r = 0; r < d->nr; ++r) {
    double sum = 0.0;
    for (int j = 0; j < ny; ++j) {
      const double c = std::cos(((j + 0.5) * 180.0 / ny - 90.0) * pi / 180.0);
      for (int i = 0; i < nx; ++i) {
        const size_t q = (size_t)j * nx + i;
        const double w = r == 0 ? c : (double)region_w[(size_t)(r - 1) * np + q] * c;
        d->w[(size_t)r * np + q] = w;
        sum += w;
      }
    }
    if (!(sum > 0.0)) {
      delete d;
      return fail(nullptr, GREB_E_INVALID, "diag_create: region " + std::to_string(r) + " has zero weight everywhere");
    }
    d->inv_sum[(size_t)r] = 1.0 / sum;
  }
  *out = d;
  return 0;
}

int greb_diag_destroy(greb_diag* d) {
  if (!d) return 0;
  int prev = 0;
  const bool have_prev = !d->devs.empty() && hipGetDevice(&prev) == hipSuccess;
  for (auto& x : d->devs)
    if (hipSetDevice(x.device) == hipSuccess) {
      (void)hipDeviceSynchronize(); // a reduction in flight may still read the tables
      (void)hipFree(x.w); (void)hipFree(x.inv_sum);
      if (x.partials) (void)hipFree(x.partials);
    }
  if (have_prev) (void)hipSetDevice(prev);
  delete d;
  return 0;
}

int greb_diag_reduce_dev(greb_diag* d, int device, const float* monthly_year_dev, int n_members, float* regions_dev,
                         float* zonal_dev, float* annual_dev, void* stream) {
  if (!d) return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: no plan (greb_diag is NULL)");
  if (!monthly_year_dev) return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: monthly_year_dev is NULL");
  if (n_members < 1) return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: n_members = " + std::to_string(n_members));
  if (!regions_dev && !zonal_dev && !annual_dev)
    return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: regions_dev, zonal_dev and annual_dev are all NULL");
  if (reinterpret_cast<uintptr_t>(monthly_year_dev) & 15)
    return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: monthly_year_dev is not 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(annual_dev) & 15)
    return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: annual_dev is not 16-byte aligned");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
    return fail(nullptr, GREB_E_NOGPU, "diag_reduce_dev: no HIP device (no CPU path)");
  HIP_TRY(nullptr, hipSetDevice(device));
  greb_diag::Dev* dv = nullptr;
  if (int rc = diag_on_device(d, device, n_members, regions_dev != nullptr, &dv)) return rc;
  const DiagArgs a = diag_args(d, dv, monthly_year_dev, regions_dev, (size_t)kDiagMonths * kDiagVars * d->nr, zonal_dev, annual_dev);
  HIP_TRY(nullptr, launch_diag_year(a, n_members, (hipStream_t)stream));
  return 0;
}

int greb_engine_run_diag(greb_engine* e, int years, const float* co2_ppm, greb_diag* d, unsigned what, float* regions,
                         float* zonal, float* annual, float* yearly) {
  // argument errors first, before anything touches a device
  if (!d) return fail(e, GREB_E_INVALID, "run_diag: no plan (greb_diag is NULL)");
  if (what == 0 || (what & ~(GREB_D_REGIONS | GREB_D_ZONAL | GREB_D_ANNUAL)))
    return fail(e, GREB_E_INVALID, "run_diag: `what` = " + std::to_string(what) + " selects no product or an unknown one");
  if ((what & GREB_D_REGIONS) && !regions) return fail(e, GREB_E_INVALID, "run_diag: GREB_D_REGIONS selected but `regions` is NULL");
  if ((what & GREB_D_ZONAL) && !zonal) return fail(e, GREB_E_INVALID, "run_diag: GREB_D_ZONAL selected but `zonal` is NULL");
  if ((what & GREB_D_ANNUAL) && !annual) return fail(e, GREB_E_INVALID, "run_diag: GREB_D_ANNUAL selected but `annual` is NULL");
  if (!e || years < 1 || !co2_ppm) return fail(e, GREB_E_INVALID, "run_diag: bad argument (engine, years or co2_ppm)");
  if (d->nx != e->nx || d->ny != e->ny)
    return fail(e, GREB_E_INVALID, "run_diag: the plan's grid " + std::to_string(d->nx) + " x " + std::to_string(d->ny) +
                                       " differs from the engine's " + std::to_string(e->nx) + " x " + std::to_string(e->ny));
  const size_t np = (size_t)e->np, nm = (size_t)e->nm;
  const bool do_r = (what & GREB_D_REGIONS) != 0, do_z = (what & GREB_D_ZONAL) != 0, do_a = (what & GREB_D_ANNUAL) != 0;
  const size_t reg_year = (size_t)12 * 5 * d->nr, zon_year = (size_t)12 * 5 * e->ny, ann_year = 5 * np; // floats per member-year
  const size_t zon_slot = do_z ? nm * zon_year : 0, ann_slot = do_a ? nm * ann_year : 0, out_slot = zon_slot + ann_slot;
  greb_diag::Dev* dv = nullptr;
  // A unit is a year's zonal means and annual maps, made in output slot y & 1 of e->diag_out.  The region series -- the
  // only thing on the device that grows with `years` besides the yearly scalars -- stays there for the whole call.
  RunSink s;
  s.prepare = [&]() -> int {
    if (out_slot) if (int rc = ensure(e, &e->diag_out, &e->diag_out_cap, 2 * out_slot)) return rc;
    if (do_r) if (int rc = ensure(e, &e->diag_reg, &e->diag_reg_cap, nm * years * reg_year)) return rc;
    return diag_on_device(d, e->device, e->nm, do_r, &dv);
  };
  s.year = [&](const YearCalls& run, int y) -> int {
    float* mon = staging_slot(e, y);
    if (int rc = run.integrate(y, {mon, 1, 0})) return rc;
    if (int rc = run.writing(y)) return rc; // (here, not before the year: only the reduction writes the slot)
    float* out = out_slot ? e->diag_out + (size_t)(y & 1) * out_slot : nullptr;
    const DiagArgs g = diag_args(d, dv, mon, do_r ? e->diag_reg + (size_t)y * reg_year : nullptr, (size_t)years * reg_year,
                                 do_z ? out : nullptr, do_a ? out + zon_slot : nullptr);
    HIP_TRY(e, launch_diag_year(g, e->nm, e->stream));
    return run.complete(y);
  };
  s.deliver = [&](int y, int sl) -> int {
    float* out = e->diag_out + (size_t)sl * out_slot;
    if (do_z) HIP_TRY(e, unit_to_host(e, zonal, years, y, out, zon_year));
    if (do_a) HIP_TRY(e, unit_to_host(e, annual, years, y, out + zon_slot, ann_year));
    return 0;
  };
  s.finish = [&]() -> int {
    if (do_r) HIP_TRY(e, hipMemcpy(regions, e->diag_reg, nm * years * reg_year * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, s);
}

} // extern "C"

// ---------------------------------------------------------------- climatology output (greb_clim.hip)
// A plan is host data only: grid, member count, each member's control and the products.  The fp64 sums (and the control
// map's device copy) are made per device the first time the plan adds a year there.  `added` counts the years since the
// last finish: one period is summed at a time, on one device.
struct greb_clim {
  int nx = 0, ny = 0, nm = 0;
  unsigned what = 0;
  std::vector<int32_t> control; // [nm], or empty: no control map
  int added = 0;                // years added since the last finish
  int added_device = -1;        // ... on this device
  struct Dev { int device; double* S; double* T; int* control; };
  std::vector<Dev> devs;
  size_t elems() const { return (size_t)nm * kClimMonths * kClimVars * nx * ny; }
};

namespace {
int clim_on_device(greb_clim* c, int device, greb_clim::Dev** out) {
  for (auto& x : c->devs) if (x.device == device) { *out = &x; return 0; }
  greb_clim::Dev n{device, nullptr, nullptr, nullptr};
  hipError_t err = dev_alloc(&n.S, c->elems());
  if (err == hipSuccess && (c->what & GREB_C_TREND)) err = dev_alloc(&n.T, c->elems());
  if (err == hipSuccess && !c->control.empty()) {
    err = dev_alloc(&n.control, c->control.size());
    if (err == hipSuccess) err = hipMemcpy(n.control, c->control.data(), c->control.size() * sizeof(int), hipMemcpyHostToDevice);
  }
  if (err != hipSuccess) {
    if (n.S) (void)hipFree(n.S);
    if (n.T) (void)hipFree(n.T);
    if (n.control) (void)hipFree(n.control);
    HIP_TRY(nullptr, err);
  }
  c->devs.push_back(n);
  *out = &c->devs.back();
  return 0;
}

// floats of one member's record of each product of one period: MEAN, SEASONS, TREND, the MEAN response, the SEASONS response
void clim_sizes(const greb_clim* c, size_t out[5]) {
  const size_t np = (size_t)c->nx * c->ny, mon = (size_t)kClimMonths * kClimVars * np, sea = (size_t)kClimSeasons * kClimVars * np;
  const bool resp = (c->what & GREB_C_RESPONSE) != 0;
  out[0] = (c->what & GREB_C_MEAN) ? mon : 0;
  out[1] = (c->what & GREB_C_SEASONS) ? sea : 0;
  out[2] = (c->what & GREB_C_TREND) ? mon : 0;
  out[3] = resp && (c->what & GREB_C_MEAN) ? mon : 0;
  out[4] = resp && (c->what & GREB_C_SEASONS) ? sea : 0;
}

ClimFinishArgs clim_finish_args(const greb_clim* c, const greb_clim::Dev* dv, int n_years, float* const out[5]) {
  ClimFinishArgs a{};
  a.S = dv->S; a.T = dv->T; a.control = dv->control;
  a.np = (size_t)c->nx * c->ny; a.n_years = n_years;
  a.mean = out[0]; a.seasons = out[1]; a.trend = out[2]; a.mean_resp = out[3]; a.seasons_resp = out[4];
  return a;
}

const char* const kClimOutNames[5] = {"mean", "seasons", "trend", "mean_resp", "seasons_resp"};
const char* const kClimFlagNames[5] = {"GREB_C_MEAN", "GREB_C_SEASONS", "GREB_C_TREND", "GREB_C_RESPONSE with GREB_C_MEAN",
                                       "GREB_C_RESPONSE with GREB_C_SEASONS"};
} // namespace

extern "C" {

int greb_clim_create(int nx, int ny, int n_members, const int32_t* control, unsigned what, greb_clim** out) {
  if (!out) return fail(nullptr, GREB_E_INVALID, "clim_create: `out` is NULL");
  *out = nullptr;
  if (nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy)
    return fail(nullptr, GREB_E_INVALID, "clim_create: grid " + std::to_string(nx) + " x " + std::to_string(ny) +
                                             " (nx % 4 == 0, nx >= 12, 5 <= ny <= " + std::to_string(kMaxNy) + ")");
  if (n_members < 1) return fail(nullptr, GREB_E_INVALID, "clim_create: n_members = " + std::to_string(n_members));
  const unsigned all = GREB_C_MEAN | GREB_C_SEASONS | GREB_C_TREND | GREB_C_RESPONSE;
  if (what == 0 || (what & ~all))
    return fail(nullptr, GREB_E_INVALID, "clim_create: `what` = " + std::to_string(what) + " selects no product or an unknown one");
  if ((what & GREB_C_RESPONSE) && !(what & (GREB_C_MEAN | GREB_C_SEASONS)))
    return fail(nullptr, GREB_E_INVALID, "clim_create: GREB_C_RESPONSE needs GREB_C_MEAN or GREB_C_SEASONS (it is their difference to "
                                         "the control)");
  if ((what & GREB_C_RESPONSE) && !control)
    return fail(nullptr, GREB_E_INVALID, "clim_create: GREB_C_RESPONSE selected but `control` is NULL");
  if (control)
    for (int m = 0; m < n_members; ++m)
      if (control[m] < -1 || control[m] >= n_members)
        return fail(nullptr, GREB_E_INVALID, "clim_create: member " + std::to_string(m) + ": control = " + std::to_string(control[m]) +
                                                 " (-1 = none, or 0 ... " + std::to_string(n_members - 1) + ")");
  greb_clim* c = new (std::nothrow) greb_clim();
  if (!c) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  c->nx = nx; c->ny = ny; c->nm = n_members; c->what = what;
  if (control) c->control.assign(control, control + n_members);
  *out = c;
  return 0;
}

int greb_clim_destroy(greb_clim* c) {
  if (!c) return 0;
  int prev = 0;
  const bool have_prev = !c->devs.empty() && hipGetDevice(&prev) == hipSuccess;
  for (auto& x : c->devs)
    if (hipSetDevice(x.device) == hipSuccess) {
      (void)hipDeviceSynchronize(); // a pass in flight may still use the sums
      (void)hipFree(x.S);
      if (x.T) (void)hipFree(x.T);
      if (x.control) (void)hipFree(x.control);
    }
  if (have_prev) (void)hipSetDevice(prev);
  delete c;
  return 0;
}

int greb_clim_add_year_dev(greb_clim* c, int device, const float* monthly_year_dev, int k, void* stream) {
  if (!c) return fail(nullptr, GREB_E_INVALID, "clim_add_year_dev: no plan (greb_clim is NULL)");
  if (!monthly_year_dev) return fail(nullptr, GREB_E_INVALID, "clim_add_year_dev: monthly_year_dev is NULL");
  if (reinterpret_cast<uintptr_t>(monthly_year_dev) & 15)
    return fail(nullptr, GREB_E_INVALID, "clim_add_year_dev: monthly_year_dev is not 16-byte aligned");
  if (k != c->added)
    return fail(nullptr, GREB_E_INVALID, "clim_add_year_dev: k = " + std::to_string(k) + ", but " + std::to_string(c->added) +
                                             " years were added since the last finish (years go in ascending order, k = 0 first)");
  if (k > 0 && device != c->added_device)
    return fail(nullptr, GREB_E_INVALID, "clim_add_year_dev: device " + std::to_string(device) + ", but this period's sums are on device " +
                                             std::to_string(c->added_device));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
    return fail(nullptr, GREB_E_NOGPU, "clim_add_year_dev: no HIP device (no CPU path)");
  HIP_TRY(nullptr, hipSetDevice(device));
  greb_clim::Dev* dv = nullptr;
  if (int rc = clim_on_device(c, device, &dv)) return rc;
  HIP_TRY(nullptr, launch_clim_add_year(monthly_year_dev, dv->S, dv->T, c->elems(), k, (hipStream_t)stream));
  c->added = k + 1; c->added_device = device;
  return 0;
}

int greb_clim_finish_dev(greb_clim* c, int device, int n_years, float* mean_dev, float* seasons_dev, float* trend_dev,
                         float* mean_resp_dev, float* seasons_resp_dev, void* stream) {
  if (!c) return fail(nullptr, GREB_E_INVALID, "clim_finish_dev: no plan (greb_clim is NULL)");
  size_t size[5];
  clim_sizes(c, size);
  float* out[5] = {mean_dev, seasons_dev, trend_dev, mean_resp_dev, seasons_resp_dev};
  for (int i = 0; i < 5; ++i) {
    if (!size[i]) { out[i] = nullptr; continue; } // (not selected: the pointer is ignored)
    if (!out[i])
      return fail(nullptr, GREB_E_INVALID, std::string("clim_finish_dev: ") + kClimFlagNames[i] + " selected but `" + kClimOutNames[i] +
                                               "_dev` is NULL");
    if (reinterpret_cast<uintptr_t>(out[i]) & 15)
      return fail(nullptr, GREB_E_INVALID, std::string("clim_finish_dev: ") + kClimOutNames[i] + "_dev is not 16-byte aligned");
  }
  if (n_years != c->added || n_years < 1)
    return fail(nullptr, GREB_E_INVALID, "clim_finish_dev: n_years = " + std::to_string(n_years) + ", but " + std::to_string(c->added) +
                                             " years were added since the last finish");
  if (device != c->added_device)
    return fail(nullptr, GREB_E_INVALID, "clim_finish_dev: device " + std::to_string(device) + ", but this period's sums are on device " +
                                             std::to_string(c->added_device));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
    return fail(nullptr, GREB_E_NOGPU, "clim_finish_dev: no HIP device (no CPU path)");
  HIP_TRY(nullptr, hipSetDevice(device));
  greb_clim::Dev* dv = nullptr;
  if (int rc = clim_on_device(c, device, &dv)) return rc;
  HIP_TRY(nullptr, launch_clim_finish(clim_finish_args(c, dv, n_years, out), c->nm, (hipStream_t)stream));
  c->added = 0; c->added_device = -1;
  return 0;
}

int greb_engine_run_clim(greb_engine* e, int years, const float* co2_ppm, greb_clim* c, int n_periods, const int32_t* first_year,
                         const int32_t* n_years, float* mean, float* seasons, float* trend, float* mean_resp, float* seasons_resp,
                         float* yearly) {
  // argument errors first, before anything touches a device: the plan, the periods, the outputs, then the engine
  if (!c) return fail(e, GREB_E_INVALID, "run_clim: no plan (greb_clim is NULL)");
  if (years < 1) return fail(e, GREB_E_INVALID, "run_clim: years = " + std::to_string(years));
  if (n_periods < 1 || !first_year || !n_years)
    return fail(e, GREB_E_INVALID, "run_clim: n_periods = " + std::to_string(n_periods) + " with first_year / n_years " +
                                       (first_year && n_years ? "given" : "NULL") + " (at least one period is needed)");
  for (int p = 0; p < n_periods; ++p) {
    const std::string who = "run_clim: period " + std::to_string(p) + " (first_year " + std::to_string(first_year[p]) + ", n_years " +
                            std::to_string(n_years[p]) + ")";
    if (n_years[p] < 1) return fail(e, GREB_E_INVALID, who + " has no years");
    if (first_year[p] < 0 || (long long)first_year[p] + n_years[p] > years)
      return fail(e, GREB_E_INVALID, who + " is not inside the run's years 0 ... " + std::to_string(years - 1));
    if (p > 0 && first_year[p] < first_year[p - 1])
      return fail(e, GREB_E_INVALID, who + " starts before period " + std::to_string(p - 1) + ": periods must be ascending");
    if (p > 0 && first_year[p] < first_year[p - 1] + n_years[p - 1])
      return fail(e, GREB_E_INVALID, who + " overlaps period " + std::to_string(p - 1) + ", which ends with year " +
                                         std::to_string(first_year[p - 1] + n_years[p - 1] - 1));
  }
  size_t size[5];
  clim_sizes(c, size);
  float* host[5] = {mean, seasons, trend, mean_resp, seasons_resp};
  for (int i = 0; i < 5; ++i)
    if (size[i] && !host[i])
      return fail(e, GREB_E_INVALID, std::string("run_clim: ") + kClimFlagNames[i] + " selected but `" + kClimOutNames[i] + "` is NULL");
  if (c->added != 0)
    return fail(e, GREB_E_INVALID, "run_clim: the plan holds " + std::to_string(c->added) + " years of an unfinished period");
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, "run_clim: bad argument (engine or co2_ppm)");
  if (c->nx != e->nx || c->ny != e->ny)
    return fail(e, GREB_E_INVALID, "run_clim: the plan's grid " + std::to_string(c->nx) + " x " + std::to_string(c->ny) +
                                       " differs from the engine's " + std::to_string(e->nx) + " x " + std::to_string(e->ny));
  if (c->nm != e->nm)
    return fail(e, GREB_E_INVALID, "run_clim: the plan is for " + std::to_string(c->nm) + " members, the engine has " +
                                       std::to_string(e->nm));
  const size_t nm = (size_t)e->nm;
  size_t at[5], out_slot = 0; // where each product sits in an output slot: [member][its record], 16-byte aligned (np % 4 == 0)
  for (int i = 0; i < 5; ++i) { at[i] = out_slot; out_slot += nm * size[i]; }
  greb_clim::Dev* dv = nullptr;
  int p = 0; // the period the current year is in or before
  // A unit is a period's products, made in output slot p & 1 of e->clim_out.  Nothing on the device grows with `years`
  // or `n_periods` (besides the yearly scalars).
  RunSink s;
  s.prepare = [&]() -> int {
    if (int rc = ensure(e, &e->clim_out, &e->clim_out_cap, 2 * out_slot)) return rc;
    return clim_on_device(c, e->device, &dv);
  };
  s.year = [&](const YearCalls& run, int y) -> int {
    float* mon = staging_slot(e, y);
    if (int rc = run.integrate(y, {mon, 1, 0})) return rc;
    while (p < n_periods && y >= first_year[p] + n_years[p]) ++p;
    if (p >= n_periods || y < first_year[p]) return 0; // (a year outside every period is integrated, not summed)
    const int k = y - first_year[p];
    HIP_TRY(e, launch_clim_add_year(mon, dv->S, dv->T, c->elems(), k, e->stream));
    if (k < n_years[p] - 1) return 0;
    if (int rc = run.writing(p)) return rc; // (here, not before the year: only the finish pass writes the slot)
    float* out[5];
    for (int i = 0; i < 5; ++i) out[i] = size[i] ? e->clim_out + (size_t)(p & 1) * out_slot + at[i] : nullptr;
    HIP_TRY(e, launch_clim_finish(clim_finish_args(c, dv, n_years[p], out), e->nm, e->stream));
    return run.complete(p);
  };
  s.deliver = [&](int u, int sl) -> int {
    for (int i = 0; i < 5; ++i)
      if (size[i]) HIP_TRY(e, unit_to_host(e, host[i], n_periods, u, e->clim_out + (size_t)sl * out_slot + at[i], size[i]));
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, s);
}

} // extern "C"

// ---------------------------------------------------------------- ensemble output (greb_ens.hip)
// A plan is host data only: grid, member count, the products, the probabilities and the member lists -- group g is
// member[offs[g] ... offs[g + 1]) in ascending member index, control[k] the control of member[k].  The lists' device copy
// (one allocation: offs, member, control) is made per device the first time the plan reduces there.
struct greb_ens {
  int nx = 0, ny = 0, nm = 0, ng = 0;
  unsigned what = 0;
  EnsProbs probs{};
  bool has_control = false;
  std::vector<int> offs, member, control;
  struct Dev { int device; int* lists; };
  std::vector<Dev> devs;
};

namespace {
int ens_on_device(greb_ens* s, int device, EnsLists* out) {
  const size_t listed = s->member.size(), n_offs = s->offs.size();
  int* base = nullptr;
  for (auto& x : s->devs) if (x.device == device) base = x.lists;
  if (!base) {
    std::vector<int> all(s->offs);
    all.insert(all.end(), s->member.begin(), s->member.end());
    all.insert(all.end(), s->control.begin(), s->control.end());
    hipError_t err = dev_alloc(&base, all.size());
    if (err == hipSuccess) err = hipMemcpy(base, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
      if (base) (void)hipFree(base);
      HIP_TRY(nullptr, err);
    }
    s->devs.push_back({device, base});
  }
  out->offs = base; out->member = base + n_offs; out->control = s->has_control ? base + n_offs + listed : nullptr;
  return 0;
}

// the five products: MEAN, VAR, the two of RANGE, QUANTILES
const char* const kEnsOutNames[5] = {"mean", "var", "min", "max", "quant"};
const char* const kEnsFlagNames[5] = {"GREB_S_MEAN", "GREB_S_VAR", "GREB_S_RANGE", "GREB_S_RANGE", "GREB_S_QUANTILES"};
// floats of one group's record of each product, for rows of n elements (0: not selected)
void ens_sizes(const greb_ens* s, size_t n, size_t out[5]) {
  out[0] = (s->what & GREB_S_MEAN) ? n : 0;
  out[1] = (s->what & GREB_S_VAR) ? n : 0;
  out[2] = out[3] = (s->what & GREB_S_RANGE) ? n : 0;
  out[4] = (s->what & GREB_S_QUANTILES) ? (size_t)s->probs.n * n : 0;
}

// the moments launch and one quantile launch per group, of x[nm][n] into out[5] (null where not selected)
int ens_launch(greb_engine* e, const greb_ens* s, const EnsLists& l, const float* x, size_t n, float* const out[5],
               hipStream_t stream) {
  if (out[0] || out[1] || out[2]) {
    EnsMomentArgs a{x, n, l, out[0], out[1], out[2], out[3]};
    HIP_TRY(e, launch_ens_moments(a, s->ng, stream));
  }
  for (int g = 0; out[4] && g < s->ng; ++g) {
    const int k0 = s->offs[(size_t)g];
    HIP_TRY(e, launch_ens_quantiles(x, n, l.member + k0, l.control ? l.control + k0 : nullptr, s->offs[(size_t)g + 1] - k0, s->probs,
                                    out[4] + (size_t)g * s->probs.n * n, stream));
  }
  return 0;
}
} // namespace

extern "C" {

int greb_ens_create(int nx, int ny, int n_members, const int32_t* group, int n_groups, const int32_t* control,
                    const float* probs, int n_probs, unsigned what, greb_ens** out) {
  if (!out) return fail(nullptr, GREB_E_INVALID, "ens_create: `out` is NULL");
  *out = nullptr;
  if (nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy)
    return fail(nullptr, GREB_E_INVALID, "ens_create: grid " + std::to_string(nx) + " x " + std::to_string(ny) +
                                             " (nx % 4 == 0, nx >= 12, 5 <= ny <= " + std::to_string(kMaxNy) + ")");
  if (n_members < 1) return fail(nullptr, GREB_E_INVALID, "ens_create: n_members = " + std::to_string(n_members));
  if (n_groups < 1 || n_groups > kEnsMaxGroups)
    return fail(nullptr, GREB_E_INVALID, "ens_create: n_groups = " + std::to_string(n_groups) + " (1 ... " +
                                             std::to_string(kEnsMaxGroups) + ")");
  if (!group) return fail(nullptr, GREB_E_INVALID, "ens_create: `group` is NULL");
  const unsigned all = GREB_S_MEAN | GREB_S_VAR | GREB_S_RANGE | GREB_S_QUANTILES;
  if (what == 0 || (what & ~all))
    return fail(nullptr, GREB_E_INVALID, "ens_create: `what` = " + std::to_string(what) + " selects no product or an unknown one");
  std::vector<int> count((size_t)n_groups, 0);
  for (int m = 0; m < n_members; ++m) {
    if (group[m] < -1 || group[m] >= n_groups)
      return fail(nullptr, GREB_E_INVALID, "ens_create: member " + std::to_string(m) + ": group = " + std::to_string(group[m]) +
                                               " (-1 = none, or 0 ... " + std::to_string(n_groups - 1) + ")");
    if (control && (control[m] < -1 || control[m] >= n_members))
      return fail(nullptr, GREB_E_INVALID, "ens_create: member " + std::to_string(m) + ": control = " + std::to_string(control[m]) +
                                               " (-1 = none, or 0 ... " + std::to_string(n_members - 1) + ")");
    if (group[m] < 0) continue;
    if (control && control[m] < 0)
      return fail(nullptr, GREB_E_INVALID, "ens_create: member " + std::to_string(m) + " is in group " + std::to_string(group[m]) +
                                               " but has no control (control = -1) while a control map is given");
    ++count[(size_t)group[m]];
  }
  for (int g = 0; g < n_groups; ++g)
    if (count[(size_t)g] == 0) return fail(nullptr, GREB_E_INVALID, "ens_create: group " + std::to_string(g) + " is empty");
  EnsProbs pr{};
  if (what & GREB_S_QUANTILES) {
    if (n_probs < 1 || n_probs > kEnsMaxProbs || !probs)
      return fail(nullptr, GREB_E_INVALID, "ens_create: GREB_S_QUANTILES with n_probs = " + std::to_string(n_probs) +
                                               (probs ? "" : " and `probs` NULL") + " (1 ... " + std::to_string(kEnsMaxProbs) + ")");
    pr.n = n_probs;
    for (int i = 0; i < n_probs; ++i) {
      if (!(probs[i] >= 0.f && probs[i] <= 1.f)) { // (a NaN fails both comparisons)
        char buf[128];
        std::snprintf(buf, sizeof(buf), "ens_create: probability %d = %g is not in [0, 1]", i, (double)probs[i]);
        return fail(nullptr, GREB_E_INVALID, buf);
      }
      pr.p[i] = probs[i];
    }
    for (int g = 0; g < n_groups; ++g)
      if (count[(size_t)g] > kEnsMaxSorted)
        return fail(nullptr, GREB_E_UNSUPPORTED, "ens_create: GREB_S_QUANTILES with group " + std::to_string(g) + " of " +
                                                     std::to_string(count[(size_t)g]) + " members (at most " +
                                                     std::to_string(kEnsMaxSorted) + " are sorted in one compute unit's LDS)");
  }
  greb_ens* s = new (std::nothrow) greb_ens();
  if (!s) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  s->nx = nx; s->ny = ny; s->nm = n_members; s->ng = n_groups; s->what = what; s->probs = pr; s->has_control = control != nullptr;
  s->offs.assign((size_t)n_groups + 1, 0);
  for (int g = 0; g < n_groups; ++g) s->offs[(size_t)g + 1] = s->offs[(size_t)g] + count[(size_t)g];
  s->member.resize((size_t)s->offs[(size_t)n_groups]);
  if (control) s->control.resize(s->member.size());
  std::vector<int> at(s->offs.begin(), s->offs.end() - 1);
  for (int m = 0; m < n_members; ++m) { // ascending member index inside every group
    if (group[m] < 0) continue;
    const size_t k = (size_t)at[(size_t)group[m]]++;
    s->member[k] = m;
    if (control) s->control[k] = control[m];
  }
  *out = s;
  return 0;
}

int greb_ens_destroy(greb_ens* s) {
  if (!s) return 0;
  int prev = 0;
  const bool have_prev = !s->devs.empty() && hipGetDevice(&prev) == hipSuccess;
  for (auto& x : s->devs)
    if (hipSetDevice(x.device) == hipSuccess) {
      (void)hipDeviceSynchronize(); // a reduction in flight may still read the lists
      (void)hipFree(x.lists);
    }
  if (have_prev) (void)hipSetDevice(prev);
  delete s;
  return 0;
}

int greb_ens_reduce_dev(greb_ens* s, int device, const float* x_dev, size_t n, float* mean_dev, float* var_dev, float* min_dev,
                        float* max_dev, float* quant_dev, void* stream) {
  if (!s) return fail(nullptr, GREB_E_INVALID, "ens_reduce_dev: no plan (greb_ens is NULL)");
  if (!x_dev) return fail(nullptr, GREB_E_INVALID, "ens_reduce_dev: x_dev is NULL");
  if (reinterpret_cast<uintptr_t>(x_dev) & 15) return fail(nullptr, GREB_E_INVALID, "ens_reduce_dev: x_dev is not 16-byte aligned");
  if (n < 1) return fail(nullptr, GREB_E_INVALID, "ens_reduce_dev: n = 0");
  size_t size[5];
  ens_sizes(s, n, size);
  float* out[5] = {mean_dev, var_dev, min_dev, max_dev, quant_dev};
  for (int i = 0; i < 5; ++i) {
    if (!size[i]) { out[i] = nullptr; continue; } // (not selected: the pointer is ignored)
    if (!out[i])
      return fail(nullptr, GREB_E_INVALID, std::string("ens_reduce_dev: ") + kEnsFlagNames[i] + " selected but `" + kEnsOutNames[i] +
                                               "_dev` is NULL");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
    return fail(nullptr, GREB_E_NOGPU, "ens_reduce_dev: no HIP device (no CPU path)");
  HIP_TRY(nullptr, hipSetDevice(device));
  EnsLists l{};
  if (int rc = ens_on_device(s, device, &l)) return rc;
  return ens_launch(nullptr, s, l, x_dev, n, out, (hipStream_t)stream);
}

int greb_engine_run_ens(greb_engine* e, int years, const float* co2_ppm, greb_ens* s, float* mean, float* var, float* min,
                        float* max, float* quant, float* yearly) {
  // argument errors first, before anything touches a device: the plan, the outputs, then the engine
  if (!s) return fail(e, GREB_E_INVALID, "run_ens: no plan (greb_ens is NULL)");
  if (years < 1) return fail(e, GREB_E_INVALID, "run_ens: years = " + std::to_string(years));
  const size_t n = (size_t)12 * 5 * s->nx * s->ny; // one member's model year
  size_t size[5];
  ens_sizes(s, n, size);
  float* host[5] = {mean, var, min, max, quant};
  for (int i = 0; i < 5; ++i)
    if (size[i] && !host[i])
      return fail(e, GREB_E_INVALID, std::string("run_ens: ") + kEnsFlagNames[i] + " selected but `" + kEnsOutNames[i] + "` is NULL");
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, "run_ens: bad argument (engine or co2_ppm)");
  if (s->nx != e->nx || s->ny != e->ny)
    return fail(e, GREB_E_INVALID, "run_ens: the plan's grid " + std::to_string(s->nx) + " x " + std::to_string(s->ny) +
                                       " differs from the engine's " + std::to_string(e->nx) + " x " + std::to_string(e->ny));
  if (s->nm != e->nm)
    return fail(e, GREB_E_INVALID, "run_ens: the plan is for " + std::to_string(s->nm) + " members, the engine has " +
                                       std::to_string(e->nm));
  const size_t ng = (size_t)s->ng;
  size_t at[5], out_slot = 0; // where each product sits in an output slot: [group][its record], 16-byte aligned (np % 4 == 0)
  for (int i = 0; i < 5; ++i) { at[i] = out_slot; out_slot += ng * size[i]; }
  EnsLists l{};
  // A unit is a year's statistics, made in output slot y & 1 of e->ens_out.  Nothing on the device grows with `years`
  // (besides the yearly scalars).
  RunSink k;
  k.prepare = [&]() -> int {
    if (int rc = ensure(e, &e->ens_out, &e->ens_out_cap, 2 * out_slot)) return rc;
    return ens_on_device(s, e->device, &l);
  };
  k.year = [&](const YearCalls& run, int y) -> int {
    float* mon = staging_slot(e, y);
    if (int rc = run.integrate(y, {mon, 1, 0})) return rc;
    if (int rc = run.writing(y)) return rc; // (here, not before the year: only the reduction writes the slot)
    float* out[5];
    for (int i = 0; i < 5; ++i) out[i] = size[i] ? e->ens_out + (size_t)(y & 1) * out_slot + at[i] : nullptr;
    if (int rc = ens_launch(e, s, l, mon, n, out, e->stream)) return rc;
    return run.complete(y);
  };
  // every group's record of year y to its place in the caller's [group][years][record] array (as unit_to_host, whose rows
  // are the members)
  k.deliver = [&](int y, int sl) -> int {
    for (int i = 0; i < 5; ++i)
      if (size[i])
        HIP_TRY(e, hipMemcpy2DAsync(host[i] + (size_t)y * size[i], (size_t)years * size[i] * sizeof(float),
                                    e->ens_out + (size_t)sl * out_slot + at[i], size[i] * sizeof(float), size[i] * sizeof(float), ng,
                                    hipMemcpyDeviceToHost, e->copy_stream));
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, k);
}

const char* greb_engine_describe(greb_engine* e) {
  static thread_local std::string s;
  if (!e) { s = "{}"; return s.c_str(); }
  char buf[256];
  std::snprintf(buf, sizeof(buf), "{\"grid\": [%d, %d], \"members\": %d, \"arithmetic\": \"%s\", \"engine\": \"%s\"", e->nx, e->ny, e->nm,
                e->strict ? "strict" : "fast", e->fused ? "fused member kernel" : (e->strips ? "row strips" : "latitude bands"));
  s = buf;
  std::snprintf(buf, sizeof(buf), ", \"member_switches\": \"%s\", \"correction_sets\": %d, \"physics_sets\": %d",
                e->xsw_uniform ? "uniform" : "per member", e->shared_corr ? 1 : e->nm, e->n_phys_sets);
  s += buf;
  std::snprintf(buf, sizeof(buf), ", \"budget_runs\": %lld", e->budget_runs);
  s += buf;
  std::snprintf(buf, sizeof(buf), ", \"forcing\": {\"patterns\": %d, \"solar_tables\": %d, \"forced_members\": %d}", e->n_patterns,
                e->n_solar, e->forced_members);
  s += buf;
  std::snprintf(buf, sizeof(buf), ", \"boundary\": {\"sets\": %d, \"members_on_sets\": %d, \"fields\": [", (int)e->bound.size() - 1,
                e->members_on_sets);
  s += buf;
  for (size_t k = 1; k < e->bound.size(); ++k) {
    s += k > 1 ? ", [" : "[";
    bool first = true;
    for (int i = 0; i < kBoundaryInputs; ++i)
      if (e->bound[k].over & (1u << i)) { s += std::string(first ? "\"" : ", \"") + kBoundaryNames[i] + "\""; first = false; }
    s += "]";
  }
  s += "]}";
  { // the packed forcing records of the FAST fused member kernel: one per set that has one
    int n = 0;
    for (const auto& b : e->bound) n += b.frec != nullptr;
    std::snprintf(buf, sizeof(buf), ", \"forcing_records\": {\"sets\": %d, \"bytes\": %zu}", n, (size_t)n * kFrBytes);
    s += buf;
  }
  { // the kernel family the next launch of each phase takes (budget output is chosen per call, on top of it)
    unsigned v;
    auto family = [&v](const MemberArgs& a) { return select_variant(a, &v) == hipSuccess ? variant_family(v) : "none"; };
    MemberArgs flux = base_args(e), scenario = base_args(e);
    flux.flux_phase = 1;
    apply_forcing(e, scenario);
    std::snprintf(buf, sizeof(buf), ", \"kernel_family\": {\"flux_correction\": \"%s\", \"scenario\": \"%s\"}", family(flux),
                  family(scenario));
    s += buf;
  }
  if (e->call != greb_engine::kCallNever) {
    std::snprintf(buf, sizeof(buf), ", \"wavefront_slots_granted\": %d, \"circulation\": [", e->slots_granted);
    s += buf;
    bool first = true;
    for (const auto& kv : e->plans) {
      const StripPlan& p = kv.second;
      std::snprintf(buf, sizeof(buf), "%s{\"members_run\": %d, \"tasks_of_one_launch_per_call\": %d, \"form\": \"%s\", \"trial_ms_per_3_steps\": [%.4f, %.4f]}",
                    first ? "" : ", ", kv.first, p.circ.n,
                    p.circ.n == 0 ? "one launch per sub-step (slots)" : (p.form == 2 ? "one launch per call" : (p.form == 1 ? "one launch per sub-step" : "undecided")),
                    p.ms_substep, p.ms_call);
      s += buf;
      first = false;
    }
    s += "]";
  }
  s += "}";
  return s.c_str();
}

int greb_engine_get_state(greb_engine* e, int member, float* state5) {
  if (!e || member < 0 || member >= e->nm || !state5) return fail(e, GREB_E_INVALID, "get_state: bad argument");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipMemcpy(state5, e->state + (size_t)member * 5 * e->np, (size_t)5 * e->np * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int greb_engine_get_corrections(greb_engine* e, int member, float* corr, float* state5) {
  if (!e || member < 0 || member >= e->nm) return fail(e, GREB_E_INVALID, "get_corrections: bad argument");
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t n = (size_t)3 * kNT * e->np, ci = e->shared_corr ? 0 : (size_t)member;
  if (corr) HIP_TRY(e, hipMemcpy(corr, e->corr + ci * n, n * sizeof(float), hipMemcpyDeviceToHost));
  if (state5) return greb_engine_get_state(e, member, state5);
  return 0;
}

static_assert(GREB_V_FLUX == kVFlux && GREB_V_SWITCHES == kVExp && GREB_V_BUDGET == kVBudget && GREB_V_FORCING == kVForce &&
              GREB_V_BOUNDARY == kVBound, "variant bits mirror the ABI");
static_assert(GREB_X_NO_ICE == kXNoIce && GREB_X_NO_HYDRO == kXNoHydro && GREB_X_NO_DEEP_OCEAN == kXNoDeepOcean &&
              GREB_X_LW_LINEAR_VAPOR == kXLwLinear && GREB_X_NO_CIRCULATION == kXNoCirc &&
              GREB_X_NO_VAPOR_TRANSPORT == kXNoQTransport && GREB_X_VAPOR_DIFFUSION_ONLY == kXQDiffOnly &&
              GREB_X_SST_PLUS1 == kXSstPlus1, "device switch constants mirror the ABI");

// greb.original.model.f90: which process each log_exp value switches off (the conditions are the original's)
unsigned greb_log_exp_switches(int le) {
  unsigned x = 0;
  if (le <= 5) x |= GREB_X_NO_ICE;                                        // :394, :492
  if (le <= 6 || le == 13 || le == 15) x |= GREB_X_NO_HYDRO;              // :453
  if (le <= 9 || le == 11 || (le >= 14 && le <= 16)) x |= GREB_X_NO_DEEP_OCEAN; // :514-515
  if (le == 11) x |= GREB_X_LW_LINEAR_VAPOR;                              // :423, :430
  if (le <= 4) x |= GREB_X_NO_CIRCULATION;                                // :553
  if (le == 7 || le == 16) x |= GREB_X_NO_VAPOR_TRANSPORT;                // :554-555
  if (le == 8) x |= GREB_X_VAPOR_DIFFUSION_ONLY;                          // :560
  if (le >= 14 && le <= 16) x |= GREB_X_SST_PLUS1;                        // :226
  return x;
}

int greb_engine_set_experiment(greb_engine* e, unsigned switches) {
  if (!e || (switches & ~0xffu)) return fail(e, GREB_E_INVALID, "set_experiment: unknown switch bits");
  e->xsw = switches;
  e->h_xsw.assign((size_t)e->nm, switches);
  e->xsw_uniform = true; // (the correction sets stay as they are: shared or one per member)
  return 0;
}

int greb_engine_set_member_experiments(greb_engine* e, const uint32_t* switches) {
  if (!e || !switches) return fail(e, GREB_E_INVALID, "set_member_experiments: bad argument");
  const size_t nm = (size_t)e->nm;
  for (size_t m = 0; m < nm; ++m)
    if (switches[m] & ~0xffu)
      return fail(e, GREB_E_INVALID, "set_member_experiments: member " + std::to_string(m) + ": unknown switch bits");
  std::vector<unsigned> sw(switches, switches + nm);
  if (int rc = check_transport_switches(e, "set_member_experiments", e->fused, sw.data(), e->nm)) return rc;
  const bool uniform = all_equal(sw.data(), e->nm);
  HIP_TRY(e, hipSetDevice(e->device));
  // Everything that can fail is done on NEW buffers; the engine changes only once they are complete (its correction
  // index, one small copy, is the last step that can fail).
  unsigned* xsw_dev = nullptr;
  float* corr = nullptr;
  auto step = [&](hipError_t err, const char* what) -> int {
    if (err == hipSuccess) return 0;
    if (corr) (void)hipFree(corr);
    if (xsw_dev) (void)hipFree(xsw_dev);
    return fail(e, (int)err, std::string("set_member_experiments: ") + what + ": " + hipGetErrorString(err));
  };
  if (!uniform) {
    if (int rc = step(dev_alloc(&xsw_dev, nm), "hipMalloc")) return rc;
    if (int rc = step(hipMemcpy(xsw_dev, sw.data(), nm * sizeof(unsigned), hipMemcpyHostToDevice), "hipMemcpy")) return rc;
    if (e->shared_corr && nm > 1) { // members that now differ need a correction set each: copies of the shared one
      const char* what = "";
      const hipError_t err = copy_shared_corrections(e, &corr, &what);
      if (int rc = step(err, what)) return rc;
      if (int rc = step(adopt_member_corrections(e, corr), "hipMemcpy")) return rc;
    }
  }
  if (xsw_dev) {
    if (e->xsw_dev) (void)hipFree(e->xsw_dev);
    e->xsw_dev = xsw_dev;
  }
  e->h_xsw = sw;
  e->xsw_uniform = uniform;
  e->xsw = uniform ? sw[0] : 0u;
  return 0;
}

static_assert(sizeof(greb_member_forcing) == sizeof(MemberForcing) && sizeof(MemberForcing) == 16,
              "the kernels read greb_member_forcing as it is");

int greb_engine_set_forcing_tables(greb_engine* e, int n_patterns, const float* co2_space, const float* co2_season, int n_solar,
                                   const float* sw_solar) {
  const char* who = "set_forcing_tables: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (n_patterns < 0 || n_patterns > GREB_MAX_FORCING_TABLES)
    return fail(e, GREB_E_INVALID, who + ("n_patterns = " + std::to_string(n_patterns)) + " (0 ... " + std::to_string(GREB_MAX_FORCING_TABLES) + ")");
  if (n_solar < 0 || n_solar > GREB_MAX_FORCING_TABLES)
    return fail(e, GREB_E_INVALID, who + ("n_solar = " + std::to_string(n_solar)) + " (0 ... " + std::to_string(GREB_MAX_FORCING_TABLES) + ")");
  if (n_patterns > 0 && !co2_space) return fail(e, GREB_E_INVALID, std::string(who) + "co2_space is NULL with n_patterns > 0");
  if (n_solar > 0 && !sw_solar) return fail(e, GREB_E_INVALID, std::string(who) + "sw_solar is NULL with n_solar > 0");
  const size_t np = (size_t)e->np, nx = (size_t)e->nx, ny = (size_t)e->ny;
  char buf[200];
  for (int k = 0; k < n_patterns; ++k) {
    for (size_t i = 0; i < np; ++i) {
      const float v = co2_space[(size_t)k * np + i];
      if (!(v >= 0.f && v <= 1.f)) { // (a NaN fails both comparisons)
        std::snprintf(buf, sizeof(buf), "%sco2_space: pattern %d: weight %g at row %zu, column %zu is not in [0, 1]", who, k, (double)v,
                      i / nx, i % nx);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
    for (int t = 0; co2_season && t < kNT; ++t) {
      const float v = co2_season[(size_t)k * kNT + t];
      if (!(v >= 0.f && v <= 1.f)) {
        std::snprintf(buf, sizeof(buf), "%sco2_season: pattern %d: weight %g at step %d is not in [0, 1]", who, k, (double)v, t + 1);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
  }
  for (int t = 0; t < n_solar; ++t)
    for (size_t i = 0; i < (size_t)kNT * ny; ++i) {
      const float v = sw_solar[(size_t)t * kNT * ny + i];
      if (!(v >= 0.f && std::isfinite(v))) {
        std::snprintf(buf, sizeof(buf), "%ssw_solar: table %d: value %g at step %zu, row %zu is negative or not finite", who, t, (double)v,
                      i / ny + 1, i % ny);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
  for (size_t m = 0; m < e->h_force.size(); ++m) { // the members' current indices must stay inside the new tables
    const greb_member_forcing& f = e->h_force[m];
    if (f.co2_pattern >= n_patterns || f.solar_table >= n_solar) {
      std::snprintf(buf, sizeof(buf), "%smember %zu is forced with co2_pattern %d, solar_table %d: outside the new %d patterns, %d tables "
                    "(change or clear the member forcing first)", who, m, f.co2_pattern, f.solar_table, n_patterns, n_solar);
      return fail(e, GREB_E_INVALID, buf);
    }
  }
  HIP_TRY(e, hipSetDevice(e->device));
  // new buffers first; the engine changes only once they are complete
  float *space = nullptr, *season = nullptr, *solar = nullptr;
  auto step = [&](hipError_t err, const char* what) -> int {
    if (err == hipSuccess) return 0;
    if (space) (void)hipFree(space);
    if (season) (void)hipFree(season);
    if (solar) (void)hipFree(solar);
    return fail(e, (int)err, std::string(who) + what + ": " + hipGetErrorString(err));
  };
  if (n_patterns > 0) {
    std::vector<float> ones;
    if (!co2_season) ones.assign((size_t)n_patterns * kNT, 1.f);
    if (int rc = step(dev_alloc(&space, (size_t)n_patterns * np), "hipMalloc")) return rc;
    if (int rc = step(dev_alloc(&season, (size_t)n_patterns * kNT), "hipMalloc")) return rc;
    if (int rc = step(hipMemcpy(space, co2_space, (size_t)n_patterns * np * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy")) return rc;
    if (int rc = step(hipMemcpy(season, co2_season ? co2_season : ones.data(), (size_t)n_patterns * kNT * sizeof(float),
                                hipMemcpyHostToDevice), "hipMemcpy")) return rc;
  }
  if (n_solar > 0) {
    if (int rc = step(dev_alloc(&solar, (size_t)n_solar * kNT * ny), "hipMalloc")) return rc;
    if (int rc = step(hipMemcpy(solar, sw_solar, (size_t)n_solar * kNT * ny * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy")) return rc;
  }
  if (int rc = step(hipStreamSynchronize(e->stream), "hipStreamSynchronize")) return rc; // nothing in flight reads the old ones
  if (e->f_space) (void)hipFree(e->f_space);
  if (e->f_season) (void)hipFree(e->f_season);
  if (e->f_solar) (void)hipFree(e->f_solar);
  e->f_space = space; e->f_season = season; e->f_solar = solar;
  e->n_patterns = n_patterns; e->n_solar = n_solar;
  return 0;
}

int greb_engine_set_member_forcing(greb_engine* e, const greb_member_forcing* f) {
  const char* who = "set_member_forcing: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (!f) { // every member {-1, ., -1, 1}: the default kernels again
    e->h_force.clear();
    e->forced_members = 0;
    return 0;
  }
  const size_t nm = (size_t)e->nm;
  char buf[200];
  int forced = 0;
  for (size_t m = 0; m < nm; ++m) {
    const greb_member_forcing& x = f[m];
    buf[0] = 0;
    if (x.co2_pattern < -1 || x.co2_pattern >= e->n_patterns)
      std::snprintf(buf, sizeof(buf), "%smember %zu: co2_pattern %d is outside -1 ... %d (set_forcing_tables gave %d patterns)", who, m,
                    x.co2_pattern, e->n_patterns - 1, e->n_patterns);
    else if (x.solar_table < -1 || x.solar_table >= e->n_solar)
      std::snprintf(buf, sizeof(buf), "%smember %zu: solar_table %d is outside -1 ... %d (set_forcing_tables gave %d tables)", who, m,
                    x.solar_table, e->n_solar - 1, e->n_solar);
    else if (x.co2_pattern >= 0 && !(std::isfinite(x.co2_ref) && x.co2_ref > 0.f))
      std::snprintf(buf, sizeof(buf), "%smember %zu: co2_ref %g is not finite or not positive", who, m, (double)x.co2_ref);
    else if (!(std::isfinite(x.solar_scale) && x.solar_scale >= 0.f))
      std::snprintf(buf, sizeof(buf), "%smember %zu: solar_scale %g is not finite or negative", who, m, (double)x.solar_scale);
    if (buf[0]) return fail(e, GREB_E_INVALID, buf);
    forced += is_forced(x);
  }
  std::vector<MemberForcing> w(nm);
  for (size_t m = 0; m < nm; ++m) // (co2_ref of a member without a pattern is never read: any bits may stand there)
    w[m] = MemberForcing{f[m].co2_pattern, f[m].co2_pattern >= 0 ? f[m].co2_ref : 1.f, f[m].solar_table, f[m].solar_scale};
  if (forced > 0) {
    HIP_TRY(e, hipSetDevice(e->device));
    MemberForcing* dev = nullptr;
    HIP_TRY(e, dev_alloc(&dev, nm));
    hipError_t err = hipMemcpy(dev, w.data(), nm * sizeof(MemberForcing), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) { (void)hipFree(dev); HIP_TRY(e, err); }
    if (e->force_dev) (void)hipFree(e->force_dev);
    e->force_dev = dev;
  }
  e->h_force.assign(f, f + nm);
  e->forced_members = forced;
  return 0;
}

static_assert(GREB_MAX_BOUNDARY_SETS == kMaxBoundarySets, "the set table's size mirrors the ABI");

int greb_engine_add_boundary_set(greb_engine* e, const greb_fields* over, int* set_id) {
  const char* who = "add_boundary_set: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (!over || !set_id) return fail(e, GREB_E_INVALID, std::string(who) + (over ? "set_id is NULL" : "`over` is NULL"));
  if (over->sw_solar)
    return fail(e, GREB_E_INVALID, std::string(who) + "sw_solar is not part of a boundary set: insolation tables are per-member forcing "
                                   "(greb_engine_set_forcing_tables, greb_engine_set_member_forcing)");
  const float* const src[kBoundaryInputs] = {over->z_topo, over->glacier, over->tclim, over->qclim, over->uclim, over->vclim,
                                             over->mldclim, over->cldclim, over->swetclim};
  unsigned mask = 0;
  for (int i = 0; i < kBoundaryInputs; ++i) if (src[i]) mask |= 1u << i;
  if (!mask) return fail(e, GREB_E_INVALID, std::string(who) + "every field of `over` is NULL: the set would be the engine's own data (set 0)");
  if ((int)e->bound.size() - 1 >= GREB_MAX_BOUNDARY_SETS)
    return fail(e, GREB_E_INVALID, who + ("the engine already has " + std::to_string(GREB_MAX_BOUNDARY_SETS)) + " boundary sets (GREB_MAX_BOUNDARY_SETS)");
  const size_t np = (size_t)e->np;
  for (int i = 0; i < kBoundaryInputs; ++i)
    for (size_t j = 0, n = src[i] ? boundary_floats(i, np) : 0; j < n; ++j)
      if (!std::isfinite(src[i][j])) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "%s%s: value %g at index %zu is not finite", who, kBoundaryNames[i], (double)src[i][j], j);
        return fail(e, GREB_E_INVALID, buf);
      }
  HIP_TRY(e, hipSetDevice(e->device));
  // the set on NEW buffers; the engine changes only once it is complete
  greb_engine::BoundSet b = e->bound[0]; // everything inherited: aliases of the engine's arrays, its host slices
  for (bool& o : b.own) o = false;
  b.over = mask;
  b.frec = nullptr;
  auto step = [&](hipError_t err, const char* what) -> int {
    if (err == hipSuccess) return 0;
    if (b.frec) { (void)hipStreamSynchronize(e->stream); (void)hipFree(b.frec); } // (the pack kernel may still be writing it)
    for (int i = 0; i < kBoundaryFields; ++i) if (b.own[i]) (void)hipFree(b.dev[i]);
    return fail(e, (int)err, std::string(who) + what + ": " + hipGetErrorString(err));
  };
  auto put = [&](int field, const float* host) -> int { // the set's own copy of one field
    float* d = nullptr;
    if (int rc = step(dev_alloc(&d, boundary_floats(field, np)), "hipMalloc")) return rc;
    b.dev[field] = d; b.own[field] = true;
    return step(hipMemcpy(d, host, boundary_floats(field, np) * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  };
  for (int i = 0; i < kBoundaryInputs; ++i)
    if (src[i]) if (int rc = put(i, src[i])) return rc;
  // derived fields whose source the set replaces, exactly as greb_engine_create makes them
  std::vector<float> toclim(over->tclim ? np : 0), z_ocean(over->mldclim ? np : 0), wz_air(over->z_topo ? np : 0), wz_vapor(over->z_topo ? np : 0);
  derive_fields(e->p, np, over->z_topo, over->tclim, over->mldclim, toclim.data(), z_ocean.data(), wz_air.data(), wz_vapor.data());
  if (over->tclim) { if (int rc = put(kBfToclim, toclim.data())) return rc; }
  if (over->mldclim) { if (int rc = put(kBfZocean, z_ocean.data())) return rc; }
  if (over->z_topo) {
    if (int rc = put(kBfWzAir, wz_air.data())) return rc;
    if (int rc = put(kBfWzVapor, wz_vapor.data())) return rc;
  }
  const size_t last = (size_t)(kNT - 1) * np;
  if (over->tclim) { b.t_last.assign(over->tclim + last, over->tclim + last + np); b.toclim = toclim; }
  if (over->qclim) b.q_last.assign(over->qclim + last, over->qclim + last + np);
  if (over->z_topo) b.z_topo.assign(over->z_topo, over->z_topo + np);
  if (over->mldclim) b.mld0.assign(over->mldclim, over->mldclim + np);
  // the table: made with the engine or with the first set (entry 0: the engine's own); a new set fills the next entry,
  // which no launch in flight reads -- and, where the engine keeps forcing records, the next record pointer behind it
  BoundarySet* table = e->bsets_dev;
  if (!table) {
    if (int rc = step(hipMalloc(reinterpret_cast<void**>(&table), kSetTableBytes), "hipMalloc")) return rc;
    const BoundarySet own = set_entry(e->bound[0]);
    if (int rc = step(hipMemcpy(table, &own, sizeof(own), hipMemcpyHostToDevice), "hipMemcpy")) { (void)hipFree(table); return rc; }
  }
  if (uses_forcing_records(e)) {
    const char* what = "";
    const hipError_t err = make_forcing_record(e, b, table, e->bound.size(), &b.frec, &what);
    if (int rc = step(err, what)) return rc;
  }
  const BoundarySet mine = set_entry(b);
  if (int rc = step(hipMemcpy(table + e->bound.size(), &mine, sizeof(mine), hipMemcpyHostToDevice), "hipMemcpy")) {
    if (!e->bsets_dev) (void)hipFree(table);
    return rc;
  }
  e->bsets_dev = table;
  e->bound.push_back(std::move(b));
  *set_id = (int)e->bound.size() - 1;
  return 0;
}

int greb_engine_set_member_boundary(greb_engine* e, const int32_t* set, unsigned flags) {
  const char* who = "set_member_boundary: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (flags & ~GREB_BS_REINIT) return fail(e, GREB_E_INVALID, who + ("unknown flag bits in " + std::to_string(flags)));
  const size_t nm = (size_t)e->nm, np = (size_t)e->np;
  const int made = (int)e->bound.size() - 1;
  std::vector<int> bs(nm, 0);
  int on_sets = 0;
  bool uniform = true;
  for (size_t m = 0; set && m < nm; ++m) {
    if (set[m] < 0 || set[m] > made)
      return fail(e, GREB_E_INVALID, who + ("member " + std::to_string(m)) + ": set " + std::to_string(set[m]) + " is outside 0 ... " +
                                         std::to_string(made) + " (add_boundary_set made " + std::to_string(made) + ")");
    bs[m] = set[m];
    on_sets += bs[m] > 0;
    uniform = uniform && bs[m] == bs[0];
  }
  // the transport kernels of the any-grid engine run all members of a launch with one W2 and one wind slice
  for (size_t m = 0; !e->fused && m < nm; ++m) {
    const unsigned t = e->bound[(size_t)bs[m]].over & ((1u << kBfZtopo) | (1u << kBfUclim) | (1u << kBfVclim));
    if (t)
      return fail(e, GREB_E_UNSUPPORTED,
                  who + ("member " + std::to_string(m)) + ": set " + std::to_string(bs[m]) + " overrides " +
                      kBoundaryNames[(t & (1u << kBfZtopo)) ? kBfZtopo : ((t & (1u << kBfUclim)) ? kBfUclim : kBfVclim)] +
                      ", which the any-grid engine (latitude bands, row strips) transports all members of a launch with -- create an "
                      "engine with those fields or run the groups beside each other (ensemble.run_beside)");
  }
  HIP_TRY(e, hipSetDevice(e->device));
  // Everything that can fail is done on NEW buffers; the engine changes only once they are complete.
  int* bset_dev = nullptr;
  MemberForcing* neutral = nullptr;
  float *corr = nullptr, *state = nullptr;
  auto step = [&](hipError_t err, const char* what) -> int {
    if (err == hipSuccess) return 0;
    if (bset_dev) (void)hipFree(bset_dev);
    if (neutral) (void)hipFree(neutral);
    if (corr) (void)hipFree(corr);
    if (state) (void)hipFree(state);
    return fail(e, (int)err, std::string(who) + what + ": " + hipGetErrorString(err));
  };
  if (on_sets > 0) {
    if (int rc = step(dev_alloc(&bset_dev, nm), "hipMalloc")) return rc;
    if (int rc = step(hipMemcpy(bset_dev, bs.data(), nm * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy")) return rc;
    if (!e->neutral_force_dev) {
      const std::vector<MemberForcing> w(nm, MemberForcing{-1, 1.f, -1, 1.f});
      if (int rc = step(dev_alloc(&neutral, nm), "hipMalloc")) return rc;
      if (int rc = step(hipMemcpy(neutral, w.data(), nm * sizeof(MemberForcing), hipMemcpyHostToDevice), "hipMemcpy")) return rc;
    }
  }
  if (flags & GREB_BS_REINIT) { // every member's state: the initial state of its set (:190-197) under its own physics
    std::vector<float> st(5 * np);
    if (int rc = step(dev_alloc(&state, nm * 5 * np), "hipMalloc of the members' states")) return rc;
    for (size_t m = 0; m < nm; ++m) {
      initial_state(e->bound[(size_t)bs[m]], e->h_phys[m], np, st.data());
      if (int rc = step(hipMemcpy(state + m * 5 * np, st.data(), 5 * np * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy")) return rc;
    }
  }
  if (int rc = step(hipStreamSynchronize(e->stream), "hipStreamSynchronize")) return rc; // nothing in flight reads what is replaced
  if (!uniform && e->shared_corr && nm > 1) { // members whose sets differ need a correction set each
    const char* what = "";
    const hipError_t err = copy_shared_corrections(e, &corr, &what);
    if (int rc = step(err, what)) return rc;
    if (int rc = step(adopt_member_corrections(e, corr), "hipMemcpy")) return rc;
  }
  if (state) { (void)hipFree(e->state); e->state = state; }
  if (neutral) e->neutral_force_dev = neutral;
  if (bset_dev) {
    if (e->bset_dev) (void)hipFree(e->bset_dev);
    e->bset_dev = bset_dev;
  }
  if (set) e->h_bset = bs; else e->h_bset.clear();
  e->members_on_sets = on_sets;
  return 0;
}

int greb_engine_set_corrections(greb_engine* e, int member, const float* corr, const float* state5) {
  if (!e || member < -1 || member >= e->nm) return fail(e, GREB_E_INVALID, "set_corrections: bad argument");
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t n = (size_t)3 * kNT * e->np, s5 = (size_t)5 * e->np;
  const int m0 = member < 0 ? 0 : member, m1 = member < 0 ? e->nm : member + 1; // -1 = every member
  for (int m = m0; m < m1; ++m) {
    const size_t ci = e->shared_corr ? 0 : (size_t)m;
    if (corr && (ci == (size_t)m || m == m0)) HIP_TRY(e, hipMemcpy(e->corr + ci * n, corr, n * sizeof(float), hipMemcpyHostToDevice));
    if (state5) HIP_TRY(e, hipMemcpy(e->state + (size_t)m * s5, state5, s5 * sizeof(float), hipMemcpyHostToDevice));
  }
  return 0;
}

int greb_engine_set_state(greb_engine* e, int member, const float* state5) {
  if (!state5) return fail(e, GREB_E_INVALID, "set_state: bad argument");
  return greb_engine_set_corrections(e, member, nullptr, state5);
}

// ---------------------------------------------------------------- batched single routines
namespace {
struct DevBuf {
  float* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
int batched_common(const greb_params* p, int nx, int ny, int batch, int device) {
  if (!p || nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy || batch < 1) return fail(nullptr, GREB_E_INVALID, "batched: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
    return fail(nullptr, GREB_E_NOGPU, "batched: no HIP device (no CPU path)");
  hipError_t err = hipSetDevice(device);
  if (err != hipSuccess) return fail(nullptr, (int)err, "hipSetDevice");
  return 0;
}
} // namespace

#define HIP_TRY0(expr) HIP_TRY(nullptr, expr)

namespace {
// device copies of row tables for greb_diffusion_batched_dev: one entry per (device, table contents), IMMUTABLE once
// uploaded -- a sweep in flight on any stream never sees its table change under it (the upload of a new table goes to
// a new buffer; the synchronous copy completes before the call that made it launches anything) -- and freed only by
// greb_release_caches(), which waits for the device first.
struct TabCache {
  struct Entry { int device; RowTables* dev; RowTables host; unsigned long long used; };
  std::mutex mu;
  std::vector<Entry> entries;
  unsigned long long clock = 0;
  static constexpr size_t kMax = 32; // a long-lived host that sweeps kappa: the least recently used table is retired
} g_tab_cache;
} // namespace

#ifdef GREB_TUNING
// diagnostic builds only (not part of include/greb_engine.h): where the fused member kernel writes its stamps,
// [n_members][8 waves][8] unsigned long long on the device (tools/stamp_member.py); NULL switches them off
int greb_tuning_set_stamps(greb_engine* e, unsigned long long* stamps_dev) {
  if (!e) return GREB_E_INVALID;
  e->stamps = stamps_dev;
  return 0;
}
#endif

int greb_release_caches(void) {
  rows_release_cache();
  std::lock_guard<std::mutex> lock(g_tab_cache.mu);
  int prev = 0;
  const bool have_prev = hipGetDevice(&prev) == hipSuccess;
  for (auto& e : g_tab_cache.entries)
    if (e.dev && hipSetDevice(e.device) == hipSuccess) { (void)hipDeviceSynchronize(); (void)hipFree(e.dev); }
  g_tab_cache.entries.clear();
  if (have_prev) (void)hipSetDevice(prev);
  return 0;
}

int greb_diffusion_batched_dev(const greb_params* p, int nx, int ny, int batch, const float* T1_dev,
                               const float* wz_dev, float* dX_dev, int strict, int sweeps, void* stream) {
  if (!p || nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy || batch < 1 || sweeps < 1)
    return fail(nullptr, GREB_E_INVALID, "diffusion_batched_dev: bad argument");
  // The row table lives in a small device buffer cached per device and table contents (the launches must not be
  // separated by an allocation or a copy: this entry point is what the HBM-roofline measurement times).  The operands
  // must live on the calling thread's current device.
  int dev = 0;
  HIP_TRY0(hipGetDevice(&dev));
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, T1_dev) != hipSuccess || attr.device != dev) {
    (void)hipGetLastError();
    return fail(nullptr, GREB_E_INVALID, "diffusion_batched_dev: T1_dev is not a device pointer of the current device");
  }
  RowTables t; compute_row_tables(*p, p->kappa, nx, ny, t);
  RowTables* tab_dev = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_tab_cache.mu);
    for (TabCache::Entry& ce : g_tab_cache.entries)
      if (ce.device == dev && std::memcmp(&t, &ce.host, sizeof(t)) == 0) { tab_dev = ce.dev; ce.used = ++g_tab_cache.clock; break; }
    if (!tab_dev && g_tab_cache.entries.size() >= TabCache::kMax) { // (once the device is idle: a sweep in flight may read it)
      size_t lru = g_tab_cache.entries.size();
      for (size_t i = 0; i < g_tab_cache.entries.size(); ++i)
        if (g_tab_cache.entries[i].device == dev && (lru == g_tab_cache.entries.size() || g_tab_cache.entries[i].used < g_tab_cache.entries[lru].used)) lru = i;
      if (lru < g_tab_cache.entries.size()) {
        HIP_TRY0(hipDeviceSynchronize());
        (void)hipFree(g_tab_cache.entries[lru].dev);
        g_tab_cache.entries.erase(g_tab_cache.entries.begin() + (long)lru);
      }
    }
    if (!tab_dev) {
      TabCache::Entry ce{dev, nullptr, t, ++g_tab_cache.clock};
      HIP_TRY0(dev_alloc(&ce.dev, 1));
      hipError_t he = hipMemcpy(ce.dev, &t, sizeof(t), hipMemcpyHostToDevice);
      if (he != hipSuccess) { (void)hipFree(ce.dev); HIP_TRY0(he); }
      g_tab_cache.entries.push_back(ce);
      tab_dev = ce.dev;
    }
  }
  for (int i = 0; i < sweeps; ++i)
    HIP_TRY0(launch_diffusion(T1_dev, wz_dev, dX_dev, tab_dev, t, nx, ny, batch, strict != 0, (hipStream_t)stream));
  return 0;
}

int greb_diffusion_launch_order(const greb_params* p, int nx, int ny, int batch, int* field, int* k0, int* k1, int* up,
                                int capacity) {
  if (!p || nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy || batch < 1 || capacity < 0 ||
      (capacity > 0 && (!field || !k0 || !k1 || !up)))
    return fail(nullptr, GREB_E_INVALID, "diffusion_launch_order: bad argument");
  RowTables t; compute_row_tables(*p, p->kappa, nx, ny, t);
  if (!rows_supported(t, nx, ny)) return 0;
  std::vector<RowsTask> tasks;
  rows_tasks(t, ny, batch, rows_default_tuning(), tasks);
  for (size_t i = 0; i < tasks.size() && (int)i < capacity; ++i) {
    field[i] = tasks[i].field; k0[i] = tasks[i].rows & 0xff; k1[i] = (tasks[i].rows >> 8) & 0x1ff;
    up[i] = (tasks[i].rows & kRowsUp) != 0;
  }
  return (int)tasks.size();
}

int greb_step_variant(int flux_phase, int switches, int budget, int forced, int on_sets, unsigned* variant) {
  if (!variant) return fail(nullptr, GREB_E_INVALID, "step_variant: bad argument");
  static float budget_words[1];
  static const MemberForcing force_words[1] = {};
  static const BoundarySet sets[1] = {};
  static const int set_of_member[1] = {};
  MemberArgs a{}; // non-null pointers for the flags set, as the engine's launches carry them; nothing reads through them
  a.flux_phase = flux_phase != 0;
  a.xsw = switches ? 1u : 0u;
  if (budget) a.bsum = a.brec = budget_words;
  if (on_sets) { a.bsets = sets; a.bset_m = set_of_member; }
  // a forced member, or -- scenario launches with members on sets -- the words that force nothing (apply_forcing)
  if (forced || (on_sets && !flux_phase)) a.force_m = force_words;
  if (select_variant(a, variant) != hipSuccess) return fail(nullptr, GREB_E_INVALID, "step_variant: no launch carries this combination");
  return 0;
}

int greb_step_variants(unsigned* out, int capacity) {
  if (capacity < 0 || (capacity > 0 && !out)) return fail(nullptr, GREB_E_INVALID, "step_variants: bad argument");
  for (int i = 0; i < kNVariants && i < capacity; ++i) out[i] = kVariants[i];
  return kNVariants;
}

int greb_member_deal_cover(int strict, int* counts) {
  if (!counts) return fail(nullptr, GREB_E_INVALID, "member_deal_cover: bad argument");
  member_deal_cover(strict != 0, counts);
  return 0;
}

static_assert(GREB_FORCING_RECORD_FIELDS == kFrFields, "the record's field count mirrors the ABI");

long long greb_forcing_record_offset(int row, int field, int lon) {
  if (row < 0 || row >= kFrNy || field < 0 || field >= kFrFields || lon < 0 || lon >= kFrNx) return -1;
  return (long long)forcing_record_offset(row, field, lon);
}

long long greb_forcing_record_field_bytes(int field) {
  if (field < 0 || field >= kFrFields) return -1;
  return (long long)(forcing_record_offset(0, field, 0) * sizeof(float));
}

int greb_forcing_record_field_static(int field) { return (field < 0 || field >= kFrFields) ? -1 : (field < kFrStaticFields ? 1 : 0); }

long long greb_forcing_record_static_floats(void) { return (long long)kFrStaticFloats; }

long long greb_forcing_record_step_floats(void) { return (long long)kFrStepFloats; }

long long greb_forcing_record_bytes(void) { return (long long)kFrBytes; }

const char* greb_forcing_record_field_name(int field) {
  static const char* const names[kFrFields] = {"z_topo", "glacier", "z_ocean", "wz_air", "tclim", "cldclim", "mldclim", "mldclim_prev",
                                               "swetclim", "wind_speed"};
  return (field < 0 || field >= kFrFields) ? nullptr : names[field];
}

int greb_engine_get_forcing_record(greb_engine* e, int set, int step, float* out) {
  const char* who = "get_forcing_record: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (!out || set < 0 || set >= (int)e->bound.size() || step < 1 || step > kNT)
    return fail(e, GREB_E_INVALID, std::string(who) + "bad argument (set 0 ... sets made, step 1 ... 730)");
  if (!e->bound[(size_t)set].frec)
    return fail(e, GREB_E_UNSUPPORTED, std::string(who) + "this engine keeps no forcing records (they belong to the FAST fused member kernel)");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipStreamSynchronize(e->stream)); // the pack kernel runs on the engine's stream
  const float* rec = e->bound[(size_t)set].frec;
  HIP_TRY(e, hipMemcpy(out, rec, kFrStaticFloats * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(e, hipMemcpy(out + kFrStaticFloats, rec + kFrStaticFloats + (size_t)(step - 1) * kFrStepFloats, kFrStepFloats * sizeof(float),
                       hipMemcpyDeviceToHost));
  return 0;
}

int greb_substep_launch_order(const greb_params* p, int nx, int ny, int n_members, const float* kappa, int* field, int* k0,
                              int* k1, int capacity) {
  if (!p || nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy || n_members < 1 || capacity < 0 || (capacity > 0 && (!field || !k0 || !k1)))
    return fail(nullptr, GREB_E_INVALID, "substep_launch_order: bad argument");
  std::vector<RowTables> tabs((size_t)n_members);
  std::vector<int> idx((size_t)n_members);
  for (int m = 0; m < n_members; ++m) { compute_row_tables(*p, kappa ? kappa[m] : p->kappa, nx, ny, tabs[m]); idx[m] = m; }
  if (n_members >= (1 << (kStepFieldBits - 1)) || !step_rows_supported(tabs.data(), n_members, nx, ny)) return 0;
  std::vector<RowsTask> tasks;
  step_rows_tasks(tabs.data(), idx.data(), n_members, ny, 256 * kStepRowsSlotsPerCu, tasks); // an MI355X: 256 CUs
  for (size_t i = 0; i < tasks.size() && (int)i < capacity; ++i) {
    field[i] = tasks[i].field & ((1 << kStepFieldBits) - 1); k0[i] = tasks[i].rows & 0xff; k1[i] = (tasks[i].rows >> 8) & 0x1ff;
  }
  return (int)tasks.size();
}

int greb_circulation_launch_plan(const greb_params* p, int nx, int ny, int n_members, const float* kappa, int slots,
                                 int* field, int* k0, int* k1, int* chain, int* dep4, int capacity) {
  if (!p || nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy || n_members < 1 || slots < 1 || capacity < 0 ||
      (capacity > 0 && (!field || !k0 || !k1 || !chain || !dep4)))
    return fail(nullptr, GREB_E_INVALID, "circulation_launch_plan: bad argument");
  std::vector<RowTables> tabs((size_t)n_members);
  std::vector<int> idx((size_t)n_members);
  for (int m = 0; m < n_members; ++m) { compute_row_tables(*p, kappa ? kappa[m] : p->kappa, nx, ny, tabs[m]); idx[m] = m; }
  if (n_members >= (1 << (kStepFieldBits - 1)) || !step_rows_supported(tabs.data(), n_members, nx, ny)) return 0;
  std::vector<CircTask> tasks;
  circ_rows_tasks(tabs.data(), idx.data(), n_members, ny, slots, tasks);
  if ((int)tasks.size() > slots) return 0;
  for (size_t i = 0; i < tasks.size() && (int)i < capacity; ++i) {
    field[i] = tasks[i].field & ((1 << kStepFieldBits) - 1); k0[i] = tasks[i].rows & 0xff; k1[i] = (tasks[i].rows >> 8) & 0x1ff;
    chain[i] = (tasks[i].rows & kCircChain) != 0;
    for (int j = 0; j < 4; ++j) dep4[4 * i + j] = tasks[i].dep[j];
  }
  return (int)tasks.size();
}

int greb_diffusion_batched(const greb_params* p, int nx, int ny, int batch, const float* T1, const float* wz,
                           float* dX, int strict, int device) {
  if (int rc = batched_common(p, nx, ny, batch, device)) return rc;
  const size_t n = (size_t)batch * nx * ny;
  DevBuf a, b, c;
  HIP_TRY0(dev_alloc(&a.p, n)); HIP_TRY0(dev_alloc(&b.p, n)); HIP_TRY0(dev_alloc(&c.p, n));
  HIP_TRY0(hipMemcpy(a.p, T1, n * 4, hipMemcpyHostToDevice));
  HIP_TRY0(hipMemcpy(b.p, wz, n * 4, hipMemcpyHostToDevice));
  if (int rc = greb_diffusion_batched_dev(p, nx, ny, batch, a.p, b.p, c.p, strict, 1, nullptr)) return rc;
  HIP_TRY0(hipDeviceSynchronize());
  HIP_TRY0(hipMemcpy(dX, c.p, n * 4, hipMemcpyDeviceToHost));
  return 0;
}

static int adv_or_circ(bool circ, const greb_params* p, int nx, int ny, int batch, const float* X, const float* wz,
                       const float* u, const float* v, float* dX, int strict, int device) {
  if (int rc = batched_common(p, nx, ny, batch, device)) return rc;
  const size_t n = (size_t)batch * nx * ny;
  DevBuf a, b, c, d, o, scr;
  RowTables t; compute_row_tables(*p, p->kappa, nx, ny, t);
  RowTables* tab_dev = nullptr;
  HIP_TRY0(dev_alloc(&tab_dev, 1));
  DevBuf tabhold; tabhold.p = reinterpret_cast<float*>(tab_dev);
  HIP_TRY0(hipMemcpy(tab_dev, &t, sizeof(t), hipMemcpyHostToDevice));
  HIP_TRY0(dev_alloc(&a.p, n)); HIP_TRY0(dev_alloc(&b.p, n)); HIP_TRY0(dev_alloc(&c.p, n));
  HIP_TRY0(dev_alloc(&d.p, n)); HIP_TRY0(dev_alloc(&o.p, n));
  HIP_TRY0(hipMemcpy(a.p, X, n * 4, hipMemcpyHostToDevice));
  HIP_TRY0(hipMemcpy(b.p, wz, n * 4, hipMemcpyHostToDevice));
  HIP_TRY0(hipMemcpy(c.p, u, n * 4, hipMemcpyHostToDevice));
  HIP_TRY0(hipMemcpy(d.p, v, n * 4, hipMemcpyHostToDevice));
  if (circ) {
    HIP_TRY0(dev_alloc(&scr.p, 3 * n));
    HIP_TRY0(launch_circulation(a.p, b.p, c.p, d.p, o.p, scr.p, tab_dev, t, nx, ny, batch, nsub_of(*p), strict != 0, nullptr));
  } else {
    HIP_TRY0(launch_advection(a.p, b.p, c.p, d.p, o.p, tab_dev, nx, ny, batch, strict != 0, nullptr));
  }
  HIP_TRY0(hipDeviceSynchronize());
  HIP_TRY0(hipMemcpy(dX, o.p, n * 4, hipMemcpyDeviceToHost));
  return 0;
}

int greb_advection_batched(const greb_params* p, int nx, int ny, int batch, const float* T1, const float* wz,
                           const float* u, const float* v, float* dX, int strict, int device) {
  return adv_or_circ(false, p, nx, ny, batch, T1, wz, u, v, dX, strict, device);
}

int greb_circulation_batched(const greb_params* p, int nx, int ny, int batch, const float* X, const float* wz,
                             const float* u, const float* v, float* dX, int strict, int device) {
  return adv_or_circ(true, p, nx, ny, batch, X, wz, u, v, dX, strict, device);
}

int greb_engine_point_physics(greb_engine* e, int ityr, float co2, const float* in5, float* out15) {
  if (!e || ityr < 1 || ityr > kNT || !in5 || !out15) return fail(e, GREB_E_INVALID, "point_physics: bad argument");
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t np = (size_t)e->np;
  DevBuf in, out;
  HIP_TRY(e, dev_alloc(&in.p, 5 * np)); HIP_TRY(e, dev_alloc(&out.p, 15 * np));
  HIP_TRY(e, hipMemcpy(in.p, in5, 5 * np * 4, hipMemcpyHostToDevice));
  PointArgs a{};
  a.nx = e->nx; a.ny = e->ny; a.np = e->np; a.ityr = ityr; a.co2 = co2;
  a.z_topo = e->z_topo; a.glacier = e->glacier; a.sw_solar = e->sw_solar; a.tclim = e->tclim;
  a.uclim = e->uclim; a.vclim = e->vclim; a.mldclim = e->mldclim; a.cldclim = e->cldclim; a.swetclim = e->swetclim;
  a.z_ocean = e->z_ocean; a.wz_air = e->wz_air; a.phys = e->h_phys[0]; a.in5 = in.p; a.out15 = out.p;
  a.xsw = e->h_xsw[0]; a.qclim = e->qclim; // (member 0's physics and switches)
  HIP_TRY(e, launch_point_physics(a, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  HIP_TRY(e, hipMemcpy(out15, out.p, 15 * np * 4, hipMemcpyDeviceToHost));
  return 0;
}

} // extern "C"
