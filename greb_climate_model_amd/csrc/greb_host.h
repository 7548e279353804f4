// greb_host.h -- what the host sources of the C ABI share (private: not installed).  greb_engine.cpp: the engine itself;
// greb_run.cpp: scenario runs; greb_plans.cpp: the output plans; greb_members.cpp: what members are set to;
// greb_batched.cpp: the single routines and the queries.
#pragma once
#include "../../include/greb_engine.h"

#include <hip/hip_runtime.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "greb_kernels.h"

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
  greb::RowTables* tabs = nullptr;
  greb::Phys* phys = nullptr;
  float* co2_dev = nullptr; size_t co2_cap = 0;
  float* monthly_dev = nullptr; size_t monthly_cap = 0;
  float* bsum = nullptr;                               // run_budget: [nm][GREB_NBUDGET][np] running sums, made on the first budget run
  float* budget_dev = nullptr; size_t budget_cap = 0;  // run_budget: two one-year staging slots of budget records
  long long budget_runs = 0;                           // run_budget calls so far (describe)
  // per-member forcing (set_forcing_tables, set_member_forcing): scenario phase only
  int n_patterns = 0, n_solar = 0;
  float *f_space = nullptr, *f_season = nullptr, *f_solar = nullptr; // [n_patterns][np], [n_patterns][730], [n_solar][730][ny]
  std::vector<greb_member_forcing> h_force;            // [nm], or empty: no member forcing set
  greb::MemberForcing* force_dev = nullptr;            // [nm], current whenever forced_members > 0
  int forced_members = 0;                              // members that name a pattern or a table or scale the insolation
  // prescribed SST (set_sst_tables, set_member_sst): scenario phase only
  int n_sst = 0;
  float *s_anom = nullptr, *s_weight = nullptr, *s_season = nullptr; // [n_sst][np], [n_sst][np] or null (1 everywhere), [n_sst][730]
  std::vector<greb_member_sst> h_sst;                  // [nm], or empty: no member SST set
  greb::MemberSst* sst_dev = nullptr;                  // [nm], current whenever sst_members > 0
  int sst_members = 0;                                 // members that name a pattern
  // stochastic heat flux (set_noise_tables, set_member_noise): scenario phase only
  int n_noise = 0;
  float *n_sigma = nullptr, *n_season = nullptr;       // [n_noise][np], [n_noise][730]
  int* n_cells = nullptr;                              // [n_noise][kNoiseRows + ny] (greb_noise.h)
  std::vector<greb_member_noise> h_noise;              // [nm], or empty: no member noise set
  greb::MemberNoise* noise_dev = nullptr;              // [nm], current whenever noisy_members > 0
  int noisy_members = 0;                               // members that name a pattern
  // boundary sets (add_boundary_set, set_member_boundary): both phases
  struct BoundSet {
    float* dev[greb::kBoundaryFields] = {}; // the set's thirteen device arrays in BoundarySet's order: its own or the engine's
    bool own[greb::kBoundaryFields] = {};   // which of them this set allocated
    unsigned over = 0;                   // bit i: input field i (< kBoundaryInputs) is overridden
    float* frec = nullptr;               // the set's forcing record (greb_kernels.h), kFrBytes; FAST fused engine only
    // what the initial state is made of (:190-197), np floats each: tclim[729], qclim[729], toclim, z_topo, mldclim[0]
    std::vector<float> t_last, q_last, toclim, z_topo, mld0;
  };
  std::vector<BoundSet> bound;                         // [1 + sets made]; [0]: the engine's own data
  std::vector<int> h_bset;                             // [nm] each member's set, or empty: every member 0
  int members_on_sets = 0;                             // members that name a set above 0
  greb::BoundarySet* bsets_dev = nullptr;              // the set table (greb_kernels.h: kSetTableBytes), made with the engine where it
                                                       // keeps forcing records, else with the first set
  int* bset_dev = nullptr;                             // [nm], current whenever members_on_sets > 0
  greb::MemberForcing* neutral_force_dev = nullptr;    // [nm] {-1, ., -1, 1}: what a BOUND scenario launch, or one with a
                                                       // prescribed-SST or noisy member, takes when no member is forced
  float* yearly_dev = nullptr; size_t yearly_cap = 0;
  float* diag_out = nullptr; size_t diag_out_cap = 0; // run_diag: zonal means and annual maps of two years (one per staging slot)
  float* diag_reg = nullptr; size_t diag_reg_cap = 0; // run_diag: the region series of the whole call
  float* clim_out = nullptr; size_t clim_out_cap = 0; // run_clim: the products of two periods (one per output slot)
  float* ens_out = nullptr; size_t ens_out_cap = 0;   // run_ens: the group statistics of two years (one per output slot)
  float* lin_out = nullptr; size_t lin_out_cap = 0;   // run_lin: the coefficients and the residual map of two years (likewise)
  double* gram_out = nullptr; size_t gram_out_cap = 0; // run_gram: the matrices of two years (likewise), in doubles
  float* derive_out = nullptr; size_t derive_out_cap = 0; // run_derived_*: one year of derived records [nm][12][n_out][np]
  // host copies needed later
  std::vector<greb::RowTables> h_tabs;
  std::vector<int> h_tab_index;
  bool strips = false;                                      // 384- or 192-wide grid on the row strips (greb_step_strip.h)
  enum { kCallNever, kCallTrial, kCallAlways } call = kCallNever; // the circulation call in ONE launch (greb_circ_rows.hip):
                                                            // never (GREB_F_NO_PERSISTENT), where the trial finds it
                                                            // faster, or wherever it can run (GREB_F_PERSISTENT)
  int cus = 0;                                              // compute units of the device (4 SIMDs each)
  int slots_granted = -1;                                   // wavefront slots of the device this engine may fill (-1: not asked yet)
  // How the row strips run the circulation of the first `nrun` members: the two launch orders and which form runs.
  struct StripPlan {
    greb::RowsTask* step_tasks = nullptr;      // one launch per sub-step (greb_step_rows.hip): the launch order on the device ...
    int n_step = 0;
    greb::RowsTask head[greb::kStepHeadTasks] = {}; // ... and its first tasks, passed by value
    greb::CircOrder circ;                      // one launch per call: tasks, flags, abort word (n == 0: not resident as a whole)
    int form = 0;                              // 0 undecided, 1 one launch per sub-step, 2 one launch per call
    float ms_substep = 0.f, ms_call = 0.f;     // the trial: three model steps of each form
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  };
  std::map<int, StripPlan> plans;                           // how the strips run, per number of members run
  std::vector<greb::Phys> h_phys;
  // model clock
  long long it_flux = 0; // steps done in the flux phase
  long long it_scnr = 0; // steps done in the scenario
  // the deal of member-year chunks (fused engine; greb_member.hip, greb_engine_set_dealing)
  int deal_workgroups = 0;              // > 0: workgroups of a dealt launch; 0: the device's compute units; < 0: no dealing
  int deal_schedule = greb::kChunksHalving;
  bool deal_force = false;              // deal also where the members do not outnumber the workgroups
  unsigned* deal_queue = nullptr;       // kQItems + members x chunks words, re-made from deal_image before every dealt launch
  unsigned* deal_image = nullptr;       // head 0, tail = members, chunk 0 of every member, empty slots
  unsigned* deal_status = nullptr;      // [4], sticky: a workgroup gave up waiting for an item (finish_years)
  int deal_members = 0, deal_chunks = 0; // what queue and image were made for
  long long deal_launches = 0;          // launches that went through the queue so far (describe)
  unsigned long long* stamps = nullptr; // -DGREB_TUNING builds only: device buffer for the member kernel's stamps
  std::string last_error;
};

namespace greb {
namespace host {

extern thread_local std::string g_last_error; // for failures before an engine exists
int fail(greb_engine* e, int code, const std::string& msg);

// a failing step of a call that names itself (`who` ends in ": ") and the step ...
#define HIP_STEP(e, who, what, expr)                                                          \
  do {                                                                                        \
    hipError_t _err = (expr);                                                                 \
    if (_err != hipSuccess)                                                                   \
      return fail((e), (int)_err, std::string(who) + (what) + ": " + hipGetErrorString(_err)); \
  } while (0)
#define HIP_TRY(e, expr) HIP_STEP(e, "", #expr, expr) // ... or is named by its expression

template <typename T>
hipError_t dev_alloc(T** p, size_t n) { return hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)); }
template <typename T>
hipError_t dev_upload(T** p, const T* host, size_t n) { // a new array and a synchronous copy into it
  const hipError_t err = dev_alloc(p, n);
  return err != hipSuccess ? err : hipMemcpy(*p, host, n * sizeof(T), hipMemcpyHostToDevice);
}

// An owned device array: freed when it goes out of scope, so a call that makes NEW buffers first may return at any
// step; what is complete is handed over with release().
template <typename T = float>
class DevBuf {
  T* p_ = nullptr;
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.release()) {}
  DevBuf& operator=(DevBuf&& o) noexcept { reset(o.release()); return *this; }
  ~DevBuf() { reset(); }
  void reset(T* p = nullptr) { if (p_) (void)hipFree(p_); p_ = p; }
  T* release() { T* p = p_; p_ = nullptr; return p; }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  // (what it held is freed first; a failed allocation leaves it empty)
  hipError_t alloc(size_t n) { reset(); const hipError_t err = dev_alloc(&p_, n); if (err != hipSuccess) p_ = nullptr; return err; }
  hipError_t upload(const T* host, size_t n) { reset(); const hipError_t err = dev_upload(&p_, host, n); if (err != hipSuccess) reset(); return err; }
};
// the engine takes a completed buffer in place of its own, which is freed
template <typename T>
void adopt(T*& mine, DevBuf<T>& made) { if (mine) (void)hipFree(mine); mine = made.release(); }

inline bool grid_ok(int nx, int ny) { return !(nx < 12 || (nx & 3) || ny < 5 || ny > kMaxNy); }
// `device` exists and is current from here on; `who` ends in ": "
int use_device(const char* who, int device);
// *buf holds at least n elements: a larger array in place of a smaller one, whose contents go
template <typename T>
int ensure(greb_engine* e, T** buf, size_t* cap, size_t n) {
  if (*cap >= n) return 0;
  if (*buf) HIP_TRY(e, hipFree(*buf));
  *buf = nullptr; *cap = 0;
  HIP_TRY(e, dev_alloc(buf, n));
  *cap = n;
  return 0;
}

// ---- the engine's data and years (greb_engine.cpp)
void compute_row_tables(const greb_params& p, float kappa, int nx, int ny, RowTables& g);
int nsub_of(const greb_params& p);
extern const char* const kBoundaryNames[kBoundaryFields];
enum { kBfZtopo, kBfGlacier, kBfTclim, kBfQclim, kBfUclim, kBfVclim, kBfMld, kBfCld, kBfSwet, kBfToclim, kBfZocean, kBfWzAir, kBfWzVapor };
inline size_t boundary_floats(int field, size_t np) { return (field >= kBfTclim && field <= kBfSwet) ? np * kNT : np; }
void derive_fields(const greb_params& p, size_t np, const float* z_topo, const float* tclim, const float* mldclim, float* toclim,
                   float* z_ocean, float* wz_air, float* wz_vapor);
void initial_state(const greb_engine::BoundSet& b, const Phys& P, size_t np, float* st);
BoundarySet set_entry(const greb_engine::BoundSet& x);
bool uses_forcing_records(const greb_engine* e);
hipError_t make_forcing_record(greb_engine* e, const greb_engine::BoundSet& b, BoundarySet* table, size_t id, DevBuf<float>& rec,
                               const char** what);
int check_transport_switches(greb_engine* e, const char* who, bool fused, const unsigned* sw, int n);
bool all_equal(const unsigned* sw, int n);

// ---- scenario runs (greb_run.cpp): one driver, one sink per output kind
// Where a scenario year's records go: year mon_y of mon_years in `mon` and, where the run has a budget, its budget
// records to year bud_y of bud_years in `bud`.
struct YearOut {
  float* mon; int mon_years, mon_y;
  float* bud = nullptr; int bud_years = 0, bud_y = 0;
};
MemberArgs scenario_args(greb_engine* e, int years, int y, const YearOut& o);
int run_year(greb_engine* e, const MemberArgs& a, int nrun);
// what the driver shares with greb_engine_flux_correction: the yearly scalars cleared before the first year, the wait
// after the last, their copy
int clear_yearly(greb_engine* e, int years);
int finish_years(greb_engine* e);
int yearly_to_host(greb_engine* e, int years, float* yearly);

// staging slot y & 1 of e->monthly_dev: one model year of every member's records, [member][12][5][np]
inline size_t year_records(const greb_engine* e) { return (size_t)e->nm * 12 * 5 * (size_t)e->np; }
inline float* staging_slot(const greb_engine* e, int y) { return e->monthly_dev + (size_t)(y & 1) * year_records(e); }
// every row's record (`rec` floats) of unit u, from `dev` to its place in the caller's [row][n][rec] array; the rows are
// the members unless said otherwise
hipError_t unit_to_host(greb_engine* e, float* host, int n, int u, const float* dev, size_t rec, size_t rows = 0);

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
int run_years(greb_engine* e, int years, const float* co2_ppm, float* yearly, const RunSink& s);

} // namespace host
} // namespace greb
