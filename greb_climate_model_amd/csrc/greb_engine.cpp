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
#include "greb_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>

using namespace greb;
using namespace greb::host;
using StripPlan = greb_engine::StripPlan;

thread_local std::string greb::host::g_last_error;

static int nint_f(float x) { return (int)lroundf(x); }

// src/greb.f90:578-582, 652-654 (diffusion), 749-753, 838-840 (advection)
void greb::host::compute_row_tables(const greb_params& p, float kappa, int nx, int ny, RowTables& g) {
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
static Phys make_phys(const greb_params& p) {
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

static void free_plan(StripPlan& p) {
  if (p.step_tasks) (void)hipFree(p.step_tasks);
  circ_rows_free_order(&p.circ);
  for (hipEvent_t ev : p.ev) if (ev) (void)hipEventDestroy(ev);
  p = StripPlan{};
}

int greb::host::fail(greb_engine* e, int code, const std::string& msg) {
  if (e) e->last_error = msg;
  g_last_error = msg;
  return code;
}

int greb::host::nsub_of(const greb_params& p) {
  int t = nint_f((float)p.dt / (float)p.dt_crcl); // :543
  return t < 1 ? 1 : t;
}

static MemberArgs base_args(greb_engine* e) {
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
  a.stamps = e->stamps; a.stamp_members = e->nm;
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
static void apply_forcing(const greb_engine* e, MemberArgs& a) {
  // (the boundary-aware scenario kernels are forcing-aware: without a forced member they get words that force nothing)
  // (so are the kernels of a launch with a prescribed-SST member: its words and tables travel beside the forcing's)
  // (and those of a launch with a noisy member)
  if (e->forced_members <= 0 && (e->members_on_sets > 0 || e->sst_members > 0 || e->noisy_members > 0)) a.force_m = e->neutral_force_dev;
  if (e->noisy_members > 0) { a.noise_m = e->noise_dev; a.n_sigma = e->n_sigma; a.n_season = e->n_season; a.n_cells = e->n_cells; }
  if (e->sst_members > 0) { a.sst_m = e->sst_dev; a.s_anom = e->s_anom; a.s_weight = e->s_weight; a.s_season = e->s_season; }
  if (e->forced_members <= 0) return;
  a.force_m = e->force_dev;
  a.f_space = e->f_space; a.f_season = e->f_season; a.f_solar = e->f_solar;
}

// Scenario year y of a run of `years` (run_years), its records going to `o`.
MemberArgs greb::host::scenario_args(greb_engine* e, int years, int y, const YearOut& o) {
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

// vapour diffused but not advected (GREB_X_VAPOR_DIFFUSION_ONLY): on the any-grid engine a property of the launch, so
// every member has it or none (checked where switches are set)
static bool calm_vapor(const greb_engine* e) { return (e->h_xsw[0] & GREB_X_VAPOR_DIFFUSION_ONLY) != 0; }

// the transport kernels of the any-grid engine run all members of a launch alike
int greb::host::check_transport_switches(greb_engine* e, const char* who, bool fused, const unsigned* sw, int n) {
  if (fused) return 0;
  for (int m = 1; m < n; ++m)
    if ((sw[m] ^ sw[0]) & GREB_X_VAPOR_DIFFUSION_ONLY)
      return fail(e, GREB_E_UNSUPPORTED,
                  std::string(who) + ": member " + std::to_string(m) + " differs from member 0 in GREB_X_VAPOR_DIFFUSION_ONLY, "
                  "which the any-grid engine applies to a whole launch -- run the two groups as two engines beside each "
                  "other (ensemble.run_beside)");
  return 0;
}

bool greb::host::all_equal(const unsigned* sw, int n) {
  for (int m = 1; m < n; ++m) if (sw[m] != sw[0]) return false;
  return true;
}

// the greb_params fields that feed data shared by every member (row-table geometry, wz_air / wz_vapor, the clock)
static int check_member_config(const char* who, const greb_params& p, const greb_member_config& c, int m) {
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

int greb::host::use_device(const char* who, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
    return fail(nullptr, GREB_E_NOGPU, std::string(who) + "no HIP device (no CPU path)");
  HIP_TRY(nullptr, hipSetDevice(device));
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
namespace {
struct SlotLedger {
  std::mutex mu;
  struct Entry { greb_engine* e; int device, members, granted; };
  std::vector<Entry> entries;
} g_slots;
} // namespace

static void ledger_register(greb_engine* e) {
  std::lock_guard<std::mutex> lock(g_slots.mu);
  g_slots.entries.push_back({e, e->device, e->nm, 0});
}
static void ledger_release(greb_engine* e) {
  std::lock_guard<std::mutex> lock(g_slots.mu);
  for (size_t i = 0; i < g_slots.entries.size(); ++i)
    if (g_slots.entries[i].e == e) { g_slots.entries.erase(g_slots.entries.begin() + (long)i); break; }
}
static int ledger_grant(greb_engine* e, int device_slots) {
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
static int check_circulation(greb_engine* e) {
  if (e->deal_status) { // the fused engine's dealt launches: did a workgroup give up waiting for an item?
    unsigned d[4] = {0, 0, 0, 0};
    if (hipMemcpy(d, e->deal_status, sizeof(d), hipMemcpyDeviceToHost) != hipSuccess)
      return fail(e, GREB_E_STATE, "dealt member launch: status word unreadable");
    if (d[0]) {
      char buf[256];
      std::snprintf(buf, sizeof(buf),
                    "dealt member launch given up: a workgroup waited more than %.1f s for item %u of its queue; results are "
                    "invalid, recreate the engine (greb_engine_set_dealing(e, -1, 0, 0) runs it without the queue)",
                    kCircSpinTicks / 1e8, d[1]);
      return fail(e, GREB_E_STATE, buf);
    }
  }
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
static int make_strip_plan(greb_engine* e, int nrun, StripPlan& p) {
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

// The fused engine's year for `nrun` members as a dealt launch, where it is one (greb_member.hip: "The deal of member-year
// chunks"): more members than workgroups, or dealing forced.  The queue and its image are made the first time a year of
// that many members and chunks runs; every launch starts from a copy of the image, enqueued in front of it.
static int deal_prepare(greb_engine* e, MemberArgs& a, int nrun, int* workgroups) {
  if (e->deal_workgroups < 0 || a.nsteps < 1 || nrun > kMaxDealtMembers) return 0;
  if (e->cus <= 0) HIP_TRY(e, hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, e->device));
  const int w = e->deal_workgroups > 0 ? e->deal_workgroups : e->cus;
  if (w < 1 || (nrun <= w && !e->deal_force)) return 0;
  const ChunkTable t = chunk_table(e->deal_schedule, a.nsteps);
  const size_t capacity = (size_t)nrun * (size_t)t.n, words = kQItems + capacity;
  if (!e->deal_status) {
    DevBuf<unsigned> st;
    HIP_TRY(e, st.alloc(4));
    HIP_TRY(e, hipMemset(st.get(), 0, 4 * sizeof(unsigned)));
    e->deal_status = st.release();
  }
  if (e->deal_members != nrun || e->deal_chunks != t.n) {
    HIP_TRY(e, hipStreamSynchronize(e->stream)); // (a launch in flight reads the queue this one replaces)
    std::vector<unsigned> image(words, 0u);
    image[kQTail] = (unsigned)nrun;
    for (int m = 0; m < nrun; ++m) image[kQItems + (size_t)m] = ((unsigned)m << 4) + 1u;
    DevBuf<unsigned> q, img;
    HIP_TRY(e, q.alloc(words));
    HIP_TRY(e, img.upload(image.data(), words));
    adopt(e->deal_queue, q);
    adopt(e->deal_image, img);
    e->deal_members = nrun; e->deal_chunks = t.n;
  }
  HIP_TRY(e, hipMemcpyAsync(e->deal_queue, e->deal_image, words * sizeof(unsigned), hipMemcpyDeviceToDevice, e->stream));
  a.queue = e->deal_queue; a.q_status = e->deal_status; a.q_capacity = (unsigned)capacity; a.chunks = t;
  *workgroups = w;
  ++e->deal_launches;
  return 0;
}

// One model year (730 steps) for the first `nrun` members, `a` describing that year.
//   fused layout : one launch of the member kernel
//   other grids  : 24 fused band sub-steps + 1 point-physics launch per model step
//   row strips   : the 24 sub-steps in one launch or one launch each (StripPlan) + 1 point-physics launch per model step
int greb::host::run_year(greb_engine* e, const MemberArgs& a, int nrun) {
  if (e->fused) {
    MemberArgs b = a;
    int workgroups = 0;
    if (int rc = deal_prepare(e, b, nrun, &workgroups)) return rc;
    HIP_TRY(e, launch_member_kernel(b, nrun, e->strict, e->stream, workgroups));
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

// The derived fields of greb_model's preamble (host, once per engine and per boundary set that replaces their source):
// Toclim :1088-1094 from tclim, z_ocean :179-183 from mldclim, wz_air / wz_vapor :201-202 from z_topo.  A null source
// leaves its outputs alone.
void greb::host::derive_fields(const greb_params& p, size_t np, const float* z_topo, const float* tclim, const float* mldclim, float* toclim,
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
void greb::host::initial_state(const greb_engine::BoundSet& b, const Phys& P, size_t np, float* st) {
  for (size_t i = 0; i < np; ++i) {
    st[i] = b.t_last[i]; st[np + i] = st[i]; st[2 * np + i] = b.toclim[i]; st[3 * np + i] = b.q_last[i];
    float c = 0.f;
    if (b.z_topo[i] > 0.f) c = P.cap_land;
    if (b.z_topo[i] <= 0.f) c = P.cap_ocean * b.mld0[i];
    st[4 * np + i] = c;
  }
}

const char* const greb::host::kBoundaryNames[kBoundaryFields] = {"z_topo", "glacier", "tclim", "qclim", "uclim", "vclim", "mldclim",
                                                                 "cldclim", "swetclim", "toclim", "z_ocean", "wz_air", "wz_vapor"};

BoundarySet greb::host::set_entry(const greb_engine::BoundSet& x) {
  return BoundarySet{x.dev[0], x.dev[1], x.dev[2], x.dev[3], x.dev[4], x.dev[5], x.dev[6], x.dev[7], x.dev[8], x.dev[9], x.dev[10],
                     x.dev[11], x.dev[12]};
}
// The FAST fused member kernel reads boundary data from one packed record per set (greb_kernels.h: forcing record).
bool greb::host::uses_forcing_records(const greb_engine* e) { return e->fused && !e->strict; }
// The record of set `b`, whose arrays are on the device: made there, on the engine's stream -- ahead of every launch that
// reads it -- and entered into slot `id` of the record pointers behind the set table.  On failure nothing is left behind
// and *what names the step.
hipError_t greb::host::make_forcing_record(greb_engine* e, const greb_engine::BoundSet& b, BoundarySet* table, size_t id,
                                           DevBuf<float>& rec, const char** what) {
  *what = "hipMalloc of the set's forcing record";
  hipError_t err = rec.alloc(kFrBytes / sizeof(float));
  if (err != hipSuccess) return err;
  float* const r = rec.get();
  *what = "packing the set's forcing record";
  err = launch_pack_forcing(set_entry(b), r, e->stream);
  if (err == hipSuccess) { *what = "hipMemcpy"; err = hipMemcpy(set_table_records(table) + id, &r, sizeof(float*), hipMemcpyHostToDevice); }
  if (err != hipSuccess) { (void)hipStreamSynchronize(e->stream); rec.reset(); } // (the pack kernel may still be writing it)
  return err;
}

// greb_engine_create_members, and greb_engine_create through it (`who` names the entry in messages)
static int create_engine(const char* who, const greb_params* p, int nx, int ny, const greb_fields* f, int n_members,
                  const greb_member_config* members, int device, unsigned flags, greb_engine** out) {
  if (!p || !f || !out || !members || n_members < 1 || !grid_ok(nx, ny))
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

  HIP_TRY(e, dev_upload(&e->z_topo, f->z_topo, np));
  HIP_TRY(e, dev_upload(&e->glacier, f->glacier, np));
  HIP_TRY(e, dev_upload(&e->sw_solar, f->sw_solar, (size_t)kNT * ny));
  HIP_TRY(e, dev_upload(&e->tclim, f->tclim, n3));
  HIP_TRY(e, dev_upload(&e->qclim, f->qclim, n3));
  HIP_TRY(e, dev_upload(&e->uclim, f->uclim, n3));
  HIP_TRY(e, dev_upload(&e->vclim, f->vclim, n3));
  HIP_TRY(e, dev_upload(&e->mldclim, f->mldclim, n3));
  HIP_TRY(e, dev_upload(&e->cldclim, f->cldclim, n3));
  HIP_TRY(e, dev_upload(&e->swetclim, f->swetclim, n3));

  // derived fields (host, once): Toclim :1088-1094, z_ocean :179-183, wz_* :201-202
  std::vector<float> toclim(np), z_ocean(np), wz_air(np), wz_vapor(np);
  derive_fields(*p, np, f->z_topo, f->tclim, f->mldclim, toclim.data(), z_ocean.data(), wz_air.data(), wz_vapor.data());
  HIP_TRY(e, dev_upload(&e->toclim, toclim.data(), np));
  HIP_TRY(e, dev_upload(&e->z_ocean, z_ocean.data(), np));
  HIP_TRY(e, dev_upload(&e->wz_air, wz_air.data(), np));
  HIP_TRY(e, dev_upload(&e->wz_vapor, wz_vapor.data(), np));
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
    DevBuf<float> rec;
    const hipError_t err = make_forcing_record(e, e->bound[0], e->bsets_dev, 0, rec, &what);
    if (err != hipSuccess) return fail(e, (int)err, std::string(who) + ": " + what + ": " + hipGetErrorString(err));
    e->bound[0].frec = rec.release();
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
  if (own_co2_flux) HIP_TRY(e, dev_upload(&e->co2_flux_dev, co2_flux.data(), nm));
  if (!e->xsw_uniform) HIP_TRY(e, dev_upload(&e->xsw_dev, switches.data(), nm));
  for (size_t m = 0; m < nm; ++m) corr_index[m] = e->shared_corr ? 0 : (int)m;
  HIP_TRY(e, dev_upload(&e->phys, e->h_phys.data(), nm));
  HIP_TRY(e, dev_upload(&e->tabs, e->h_tabs.data(), e->h_tabs.size()));
  HIP_TRY(e, dev_upload(&e->tab_index, tab_index.data(), nm));
  e->h_tab_index = tab_index;
  HIP_TRY(e, dev_upload(&e->corr_index, corr_index.data(), nm));

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

// What the driver shares with greb_engine_flux_correction.  Before the first year of a call: the yearly scalars
// [member][years][2], cleared on the compute stream.
int greb::host::clear_yearly(greb_engine* e, int years) {
  const size_t n = (size_t)e->nm * years * 2;
  if (int rc = ensure(e, &e->yearly_dev, &e->yearly_cap, n)) return rc;
  HIP_TRY(e, hipMemsetAsync(e->yearly_dev, 0, n * sizeof(float), e->stream));
  return 0;
}
// after the last year of a call is enqueued: wait for it, then ask the one-launch circulation calls whether one gave up
int greb::host::finish_years(greb_engine* e) {
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return check_circulation(e);
}
int greb::host::yearly_to_host(greb_engine* e, int years, float* yearly) {
  if (yearly) HIP_TRY(e, hipMemcpy(yearly, e->yearly_dev, (size_t)e->nm * years * 2 * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

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
                  e->Xa, e->Xb, e->red, e->W2, e->xsw_dev, e->co2_flux_dev, e->diag_out, e->diag_reg, e->clim_out, e->ens_out, e->lin_out, e->gram_out, e->derive_out, e->bsum, e->budget_dev,
                  e->f_space, e->f_season, e->f_solar, e->force_dev, e->bsets_dev, e->bset_dev, e->neutral_force_dev,
                  e->s_anom, e->s_weight, e->s_season, e->sst_dev, e->n_sigma, e->n_season, e->n_cells, e->noise_dev, e->deal_queue, e->deal_image, e->deal_status};
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
  std::snprintf(buf, sizeof(buf), ", \"sst\": {\"patterns\": %d, \"prescribed_members\": %d}", e->n_sst, e->sst_members);
  s += buf;
  std::snprintf(buf, sizeof(buf), ", \"noise\": {\"patterns\": %d, \"noisy_members\": %d}", e->n_noise, e->noisy_members);
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
  if (e->fused) { // the deal of member-year chunks: the setting, and how many launches so far went through the queue
    std::snprintf(buf, sizeof(buf), ", \"dealing\": {\"workgroups\": %d, \"schedule\": %d, \"forced\": %s, \"dealt_launches\": %lld}",
                  e->deal_workgroups, e->deal_schedule, e->deal_force ? "true" : "false", e->deal_launches);
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

int greb_engine_set_dealing(greb_engine* e, int workgroups, int schedule, int force) {
  if (!e || schedule < 0 || schedule >= kNChunkSchedules) return fail(e, GREB_E_INVALID, "set_dealing: bad argument");
  e->deal_workgroups = workgroups; e->deal_schedule = schedule; e->deal_force = force != 0;
  return 0;
}

int greb_engine_set_state(greb_engine* e, int member, const float* state5) {
  if (!state5) return fail(e, GREB_E_INVALID, "set_state: bad argument");
  return greb_engine_set_corrections(e, member, nullptr, state5);
}

} // extern "C"
