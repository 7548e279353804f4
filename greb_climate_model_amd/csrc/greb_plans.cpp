// greb_plans.cpp -- the output plans (greb_diag, greb_clim, greb_ens, greb_lin, greb_gram, greb_cross, greb_reg): their _dev entry points and their scenario-run sinks.
// A plan is host data only; what it needs on a device is made the first time it works there (PerDevice).
#include "greb_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>

#include "greb_diag.h"
#include "greb_clim.h"
#include "greb_ens.h"
#include "greb_lin.h"
#include "greb_gram.h"
#include "greb_cross.h"
#include "greb_reg.h"
#include "greb_fluxes.h"
#include "greb_derive.h"

using namespace greb;
using namespace greb::host;

static_assert(kGramMaxUsed == GREB_GRAM_MAX_USED && kGramMaxBlocks == GREB_GRAM_MAX_BLOCKS, "greb_gram.h mirrors include/greb_engine.h");
static_assert(kCrossMaxEvents == GREB_CROSS_MAX_EVENTS && sizeof(greb_cross_event) == 20, "greb_cross.h mirrors include/greb_engine.h");
static_assert(kRegMaxTerms == GREB_REG_MAX_TERMS && kRegMaxIndices == GREB_REG_MAX_INDICES && sizeof(greb_reg_index) == 16 &&
                  sizeof(greb_reg_term) == 16 && season::kSelectors == 17 && kRegMaxMembers == GREB_REG_MAX_MEMBERS,
              "greb_reg.h mirrors include/greb_engine.h");
static_assert(kFluxTerms == GREB_NBUDGET && kFluxMaxOut == GREB_MAX_RECORD_VARS, "greb_fluxes.h mirrors include/greb_engine.h");
static_assert(kDeriveStates == GREB_NVAR_OUT && kDeriveTerms == GREB_NBUDGET && kDeriveMaxOut == GREB_MAX_RECORD_VARS &&
                  kDeriveMaxIns == GREB_DERIVE_MAX_INS && kDeriveMaxTotal == GREB_DERIVE_MAX_TOTAL &&
                  kDeriveMaxStack == GREB_DERIVE_MAX_STACK && kDeriveMaxLocals == GREB_DERIVE_MAX_LOCALS &&
                  kDeriveMaxFields == GREB_DERIVE_MAX_FIELDS && kDeriveOps == GREB_DV_SELECT + 1 && sizeof(greb_derive_ins) == 12,
              "greb_derive.h mirrors include/greb_engine.h");

namespace {
constexpr int kStateVars = GREB_NVAR_OUT; // the variables of a year of state records

// a count `name` of the caller's is 1 ... max
int check_count(greb_engine* e, const std::string& who, const char* name, int n, int max) {
  if (n >= 1 && n <= max) return 0;
  return fail(e, GREB_E_INVALID, who + ": " + name + " = " + std::to_string(n) + " (1 ... " + std::to_string(max) + ")");
}
int check_n_vars(const std::string& who, int n_vars) { return check_count(nullptr, who, "n_vars", n_vars, GREB_MAX_RECORD_VARS); }

// combo[n_out][GREB_NBUDGET] checked and packed for the kernel arguments
int make_combo(greb_engine* e, const std::string& who, const float* combo, int n_out, FluxCombo* out) {
  if (!combo) return fail(e, GREB_E_INVALID, who + ": `combo` is NULL");
  if (int rc = check_count(e, who, "n_out", n_out, GREB_MAX_RECORD_VARS)) return rc;
  FluxCombo c{};
  c.n_out = n_out;
  for (int k = 0; k < n_out; ++k) {
    unsigned row = 0;
    for (int j = 0; j < GREB_NBUDGET; ++j) {
      const float v = combo[(size_t)k * GREB_NBUDGET + j];
      if (!std::isfinite(v)) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), ": combo row %d, term %d (%s) = %g is not finite", k, j, greb_budget_name(j), (double)v);
        return fail(e, GREB_E_INVALID, who + buf);
      }
      c.c[k][j] = v;
      if (v != 0.f) row |= 1u << j;
    }
    if (!row)
      return fail(e, GREB_E_INVALID, who + ": combo row " + std::to_string(k) + " is zero in every term 0 ... " +
                                         std::to_string(GREB_NBUDGET - 1) + " (an output must use at least one term)");
    c.used |= row;
  }
  *out = c;
  return 0;
}

// what Records asks of a derive plan (greb_derive, below)
int derive_n_out(const greb_derive* v);
int derive_check_engine(greb_engine* e, const std::string& who, const greb_derive* v);
int derive_on_engine(greb_engine* e, greb_derive* v);
int derive_year(greb_engine* e, greb_derive* v, const float* state, const float* budget, float* out);

// Where the records a reduced run hands its plan come from: the year's five state records (greb_engine_run_diag, ...), or
// its budget records -- the thirteen terms as the step kernels leave them, or their combinations (greb_engine_run_budget_diag,
// ...) --, or records derived from either (greb_engine_run_derived_diag, ...).  One year at a time in e->budget_dev: the terms
// in front, the combinations behind them; the derived records in e->derive_out; everything that reads a year is enqueued
// on the compute stream before the next year's kernels.
struct Records {
  int nv = kStateVars; // variables per month
  bool budget = false, combine = false;
  FluxCombo combo{};
  greb_derive* derive = nullptr;
  // the outputs of `v`: integrated as a state run where no output names a term, else as a budget run
  int init_derived(greb_engine* e, const std::string& who, greb_derive* v) {
    if (!v) return fail(e, GREB_E_INVALID, who + ": no derive plan (greb_derive is NULL)");
    if (e) if (int rc = derive_check_engine(e, who, v)) return rc;
    derive = v; budget = greb_derive_uses_budget(v) != 0; nv = derive_n_out(v);
    return 0;
  }
  // the state records, the terms (combo == NULL) or the rows of combo; `who` names the entry point
  int init(greb_engine* e, const std::string& who, bool from_budget, const float* c, int n_out) {
    budget = from_budget;
    if (!budget) return 0;
    nv = GREB_NBUDGET;
    if (!c) return 0;
    if (int rc = make_combo(e, who, c, n_out, &combo)) return rc;
    combine = true; nv = n_out;
    return 0;
  }
  // a diag or clim plan is made for a variable count
  int check_plan(greb_engine* e, const std::string& who, int plan_vars) const {
    if (plan_vars == nv) return 0;
    return fail(e, GREB_E_INVALID, who + ": the plan is for n_vars = " + std::to_string(plan_vars) + ", this run reduces records of " +
                                       std::to_string(nv) + " variables");
  }
  size_t year(const greb_engine* e) const { return (size_t)e->nm * 12 * nv * (size_t)e->np; } // floats of every member's year
  static size_t terms_year(const greb_engine* e) { return (size_t)e->nm * 12 * GREB_NBUDGET * (size_t)e->np; }
  // as run_records with a budget: the sums made and zeroed on first use, the call counted
  int prepare(greb_engine* e) const {
    if (derive) {
      if (int rc = ensure(e, &e->derive_out, &e->derive_out_cap, year(e))) return rc;
      if (int rc = derive_on_engine(e, derive)) return rc;
    }
    if (!budget) return 0;
    if (!e->bsum) {
      const size_t n = (size_t)e->nm * GREB_NBUDGET * (size_t)e->np;
      HIP_TRY(e, dev_alloc(&e->bsum, n));
      HIP_TRY(e, hipMemsetAsync(e->bsum, 0, n * sizeof(float), e->stream));
    }
    ++e->budget_runs;
    return ensure(e, &e->budget_dev, &e->budget_cap, terms_year(e) + (combine ? year(e) : 0));
  }
  // enqueue year y; *rec: where its records [member][12][nv][np] are once it is done
  int integrate(greb_engine* e, const YearCalls& run, int y, const float** rec) const {
    if (!budget) {
      float* mon = staging_slot(e, y);
      *rec = mon;
      if (int rc = run.integrate(y, {mon, 1, 0})) return rc;
      if (!derive) return 0;
      *rec = e->derive_out;
      return derive_year(e, derive, mon, nullptr, e->derive_out);
    }
    // (the kernels write their five records regardless -- into a staging slot only a derive stage reads)
    if (int rc = run.integrate(y, {staging_slot(e, 0), 1, 0, e->budget_dev, 1, 0})) return rc;
    *rec = e->budget_dev;
    if (derive) {
      *rec = e->derive_out;
      return derive_year(e, derive, staging_slot(e, 0), e->budget_dev, e->derive_out);
    }
    if (!combine) return 0;
    float* out = e->budget_dev + terms_year(e);
    HIP_TRY(e, launch_budget_combine(combo, e->budget_dev, e->nm, (size_t)e->np, out, e->stream));
    *rec = out;
    return 0;
  }
};

// A plan's device data: one T, which owns its arrays (DevBuf), per device the plan has worked on.
template <typename T>
class PerDevice {
  std::map<int, T> devs_;
 public:
  // the entry of `device` (current); `make` fills a new one, and one it leaves half made frees itself
  template <typename Make>
  int get(int device, Make make, T** out) {
    auto it = devs_.find(device);
    if (it == devs_.end()) {
      T n;
      if (int rc = make(n)) return rc;
      it = devs_.emplace(device, std::move(n)).first;
    }
    *out = &it->second;
    return 0;
  }
  ~PerDevice() { // what is in flight on a device may still use the entry
    int prev = 0;
    const bool have_prev = !devs_.empty() && hipGetDevice(&prev) == hipSuccess;
    for (auto it = devs_.begin(); it != devs_.end(); it = devs_.erase(it))
      if (hipSetDevice(it->first) == hipSuccess) (void)hipDeviceSynchronize();
    if (have_prev) (void)hipSetDevice(prev);
  }
};

// ---- the checks every plan kind makes; `who` names the entry point
int check_grid(const std::string& who, int nx, int ny) {
  if (grid_ok(nx, ny)) return 0;
  return fail(nullptr, GREB_E_INVALID, who + ": grid " + std::to_string(nx) + " x " + std::to_string(ny) +
                                           " (nx % 4 == 0, nx >= 12, 5 <= ny <= " + std::to_string(kMaxNy) + ")");
}
int check_what(greb_engine* e, const std::string& who, unsigned what, unsigned all) {
  if (what != 0 && !(what & ~all)) return 0;
  return fail(e, GREB_E_INVALID, who + ": `what` = " + std::to_string(what) + " selects no product or an unknown one");
}
int check_aligned(const std::string& who, const void* p, const std::string& name) {
  if (!(reinterpret_cast<uintptr_t>(p) & 15)) return 0;
  return fail(nullptr, GREB_E_INVALID, who + ": " + name + " is not 16-byte aligned");
}
// the plan fits the engine: its grid and, where it has one (nm >= 0), its member count
int check_engine(greb_engine* e, const std::string& who, int nx, int ny, int nm) {
  if (nx != e->nx || ny != e->ny)
    return fail(e, GREB_E_INVALID, who + ": the plan's grid " + std::to_string(nx) + " x " + std::to_string(ny) +
                                       " differs from the engine's " + std::to_string(e->nx) + " x " + std::to_string(e->ny));
  if (nm >= 0 && nm != e->nm)
    return fail(e, GREB_E_INVALID, who + ": the plan is for " + std::to_string(nm) + " members, the engine has " + std::to_string(e->nm));
  return 0;
}

const char* const kSelRange = " (0 ... 11: a month; 12 ... 16: DJF, MAM, JJA, SON, ANN)"; // a selector of greb_season.h

// What every create says first: somewhere to put the plan, the grid and, where the kind asks these next, the variable
// count and the member count.
template <typename Plan>
int begin_create(const std::string& who, Plan** out, int nx, int ny, const int* n_vars, const int* n_members) {
  if (!out) return fail(nullptr, GREB_E_INVALID, who + ": `out` is NULL");
  *out = nullptr;
  if (int rc = check_grid(who, nx, ny)) return rc;
  if (n_vars) if (int rc = check_n_vars(who, *n_vars)) return rc;
  if (n_members && *n_members < 1) return fail(nullptr, GREB_E_INVALID, who + ": n_members = " + std::to_string(*n_members));
  return 0;
}
// member m's control is none or a member (no control map: nothing to check) ...
int check_control_of(const std::string& who, const int32_t* control, int m, int n_members) {
  if (!control || (control[m] >= -1 && control[m] < n_members)) return 0;
  return fail(nullptr, GREB_E_INVALID, who + ": member " + std::to_string(m) + ": control = " + std::to_string(control[m]) +
                                           " (-1 = none, or 0 ... " + std::to_string(n_members - 1) + ")");
}
// ... and every member's
int check_control(const std::string& who, const int32_t* control, int n_members) {
  for (int m = 0; m < n_members; ++m)
    if (int rc = check_control_of(who, control, m, n_members)) return rc;
  return 0;
}
// The members a lin or gram plan uses (`use` NULL: all) in ascending member index, and their controls where there is a
// map: each member's control is checked, a used one needs one, and one member at least is used.
int used_members(const std::string& who, const int32_t* use, const int32_t* control, int n_members, std::vector<int>* member,
                 std::vector<int>* control_of_used) {
  for (int m = 0; m < n_members; ++m) {
    if (int rc = check_control_of(who, control, m, n_members)) return rc;
    if (use && !use[m]) continue;
    if (control && control[m] < 0)
      return fail(nullptr, GREB_E_INVALID, who + ": member " + std::to_string(m) +
                                               " is used but has no control (control = -1) while a control map is given");
    member->push_back(m);
    if (control) control_of_used->push_back(control[m]);
  }
  if (member->empty()) return fail(nullptr, GREB_E_INVALID, who + ": no used member (`use` is zero everywhere)");
  return 0;
}
// The lists of the members by group (ens, cross; `what` = "member", `of` = "group") or of the records by block (gram): group
// g is member[offs[g] ... offs[g + 1]) in ascending index, of the members with group[m] = g (-1: in none).  `also(m)` is
// what else the kind asks of member m, once its group is in range.
int group_lists(const std::string& who, const char* what, const char* of, const int32_t* group, int n_groups, int n_members,
                std::vector<int>* offs, std::vector<int>* member, const std::function<int(int)>& also = nullptr) {
  offs->assign((size_t)n_groups + 1, 0);
  for (int m = 0; m < n_members; ++m) {
    if (group[m] < -1 || group[m] >= n_groups)
      return fail(nullptr, GREB_E_INVALID, who + ": " + what + " " + std::to_string(m) + ": " + of + " = " + std::to_string(group[m]) +
                                               " (-1 = none, or 0 ... " + std::to_string(n_groups - 1) + ")");
    if (also) if (int rc = also(m)) return rc;
    if (group[m] >= 0) ++(*offs)[(size_t)group[m] + 1];
  }
  for (int g = 0; g < n_groups; ++g) {
    if ((*offs)[(size_t)g + 1] == 0) return fail(nullptr, GREB_E_INVALID, who + ": " + of + " " + std::to_string(g) + " is empty");
    (*offs)[(size_t)g + 1] += (*offs)[(size_t)g];
  }
  member->resize((size_t)offs->back());
  std::vector<int> at(offs->begin(), offs->end() - 1);
  for (int m = 0; m < n_members; ++m)
    if (group[m] >= 0) (*member)[(size_t)at[(size_t)group[m]]++] = m;
  return 0;
}

// The years a clim, cross or reg plan has taken since the last finish: one period is followed at a time, on one device.
// `holds` says what of it lies there ("sums are", "state is").
struct Period {
  const char* holds;
  int added = 0, added_device = -1;
  int check_add(const std::string& who, int k, int device) const {
    if (k != added)
      return fail(nullptr, GREB_E_INVALID, who + ": k = " + std::to_string(k) + ", but " + std::to_string(added) +
                                               " years were added since the last finish (years go in ascending order, k = 0 first)");
    return k > 0 ? check_device(who, device) : 0;
  }
  int check_finish(const std::string& who, int n_years, int device) const {
    if (n_years != added || n_years < 1)
      return fail(nullptr, GREB_E_INVALID, who + ": n_years = " + std::to_string(n_years) + ", but " + std::to_string(added) +
                                               " years were added since the last finish");
    return check_device(who, device);
  }
  int check_idle(greb_engine* e, const std::string& who) const { // a scenario run follows a period of its own
    if (added == 0) return 0;
    return fail(e, GREB_E_INVALID, who + ": the plan holds " + std::to_string(added) + " years of an unfinished period");
  }
  void advance(int k, int device) { added = k + 1; added_device = device; }
  void reset() { added = 0; added_device = -1; }
 private:
  int check_device(const std::string& who, int device) const {
    if (device == added_device) return 0;
    return fail(nullptr, GREB_E_INVALID, who + ": device " + std::to_string(device) + ", but this period's " + holds + " on device " +
                                             std::to_string(added_device));
  }
};

// The products of a plan: per product the entry points' parameter (without "_dev"), what selects it, the elements of
// one row's record (0: not selected) and its rows where they are its own (lin).  An output slot holds [row][record] of each
// selected product in turn, 16-byte aligned (np % 4 == 0); the rows are the members (clim) or the groups (ens).
struct Products {
  struct One { const char* name; const char* flag; size_t size, rows = 0; };
  static constexpr int kMax = 6;
  One p[kMax] = {};
  int n = 0;
  size_t at[kMax] = {}, out_slot = 0;
  Products(std::initializer_list<One> l) { for (const One& o : l) p[n++] = o; }
  void layout(size_t n_rows = 0) {
    out_slot = 0;
    for (int i = 0; i < n; ++i) {
      if (n_rows) p[i].rows = n_rows;
      at[i] = out_slot; out_slot += p[i].rows * p[i].size;
    }
  }
  // every selected product has somewhere to go (suffix "_dev": on the device); what is not selected is ignored
  template <typename T>
  int check(greb_engine* e, const std::string& who, T* ptr[], const char* suffix, bool aligned) const {
    for (int i = 0; i < n; ++i) {
      if (!p[i].size) { ptr[i] = nullptr; continue; }
      if (!ptr[i]) return fail(e, GREB_E_INVALID, who + ": " + p[i].flag + " selected but `" + p[i].name + suffix + "` is NULL");
      if (aligned) if (int rc = check_aligned(who, ptr[i], std::string(p[i].name) + suffix)) return rc;
    }
    return 0;
  }
  void pointers(float* slot, float* out[]) const { for (int i = 0; i < n; ++i) out[i] = p[i].size ? slot + at[i] : nullptr; }
};

// The year of a run of which every year is a unit: its records, then what `launch(mon, y)` enqueues -- the only thing that
// writes output slot y & 1, hence `writing` here and not before the year.  delivers = false: nothing leaves before the end.
template <typename Launch>
std::function<int(const YearCalls&, int)> year_hook(greb_engine* e, const Records* src, Launch launch, bool delivers = true) {
  return [e, src, launch, delivers](const YearCalls& run, int y) -> int {
    const float* mon = nullptr;
    if (int rc = src->integrate(e, run, y, &mon)) return rc;
    if (delivers) if (int rc = run.writing(y)) return rc;
    if (int rc = launch(mon, y)) return rc;
    return delivers ? run.complete(y) : 0;
  };
}

// What run_clim, run_ens and run_lin share.  Unit u of n_units is made in output slot u & 1 of *buf (slot()), and every row's
// record of it leaves from there to its place in the caller's [row][n_units][record] arrays.
struct ProductSink {
  greb_engine* e; const Products& pr; float** buf; size_t* cap; float* const* host; int n_units;
  float* slot(int u) const { return *buf + (size_t)(u & 1) * pr.out_slot; }
  void install(RunSink& s, std::function<int()> plan_on_device) const {
    const ProductSink k = *this;
    s.prepare = [k, plan_on_device]() -> int {
      if (int rc = ensure(k.e, k.buf, k.cap, 2 * k.pr.out_slot)) return rc;
      return plan_on_device();
    };
    s.deliver = [k](int u, int sl) -> int {
      for (int i = 0; i < k.pr.n; ++i)
        if (k.pr.p[i].size) HIP_TRY(k.e, unit_to_host(k.e, k.host[i], k.n_units, u, k.slot(sl) + k.pr.at[i], k.pr.p[i].size, k.pr.p[i].rows));
      return 0;
    };
  }
};
} // namespace

// ---------------------------------------------------------------- reduced output (greb_diag.hip)
// The combined weights w_r * cos(lat_j) of the globe and the caller's regions and the reciprocals of their sums, made
// once in double.  Per device: their copies and the scratch array of the per-band partial sums.
struct greb_diag {
  int nx = 0, ny = 0, nr = 0;  // nr = 1 + n_regions
  int nv = kStateVars;         // variables per month of the records it reduces
  std::vector<double> w;       // [nr][ny][nx]
  std::vector<double> inv_sum; // [nr]
  struct Dev { DevBuf<double> w, inv_sum, partials; size_t partials_cap = 0; };
  PerDevice<Dev> devs;
};

namespace {
// the plan's tables on `device` (current), with room for the partial sums of `n_members` when regions are reduced
int diag_on_device(greb_diag* d, int device, int n_members, bool regions, greb_diag::Dev** out) {
  greb_diag::Dev* dv = nullptr;
  auto make = [d](greb_diag::Dev& n) -> int {
    HIP_TRY(nullptr, n.w.upload(d->w.data(), d->w.size()));
    HIP_TRY(nullptr, n.inv_sum.upload(d->inv_sum.data(), d->inv_sum.size()));
    return 0;
  };
  if (int rc = d->devs.get(device, make, &dv)) return rc;
  const size_t need = regions ? diag_partials(d->nx, d->ny, n_members, d->nr, d->nv) : 0;
  if (dv->partials_cap < need) { // (a larger batch than before: an earlier reduction may still read the old array)
    if (dv->partials) HIP_TRY(nullptr, hipDeviceSynchronize());
    dv->partials_cap = 0;
    HIP_TRY(nullptr, dv->partials.alloc(need));
    dv->partials_cap = need;
  }
  *out = dv;
  return 0;
}

DiagArgs diag_args(const greb_diag* d, const greb_diag::Dev* dv, const float* monthly, float* regions, size_t regions_stride,
                   float* zonal, float* annual) {
  DiagArgs a{};
  a.monthly = monthly; a.nx = d->nx; a.ny = d->ny; a.nr = d->nr; a.nv = d->nv;
  a.w = dv->w.get(); a.inv_sum = dv->inv_sum.get(); a.partials = dv->partials.get();
  a.regions = regions; a.regions_stride = regions_stride; a.zonal = zonal; a.annual = annual;
  return a;
}

// The plan of greb_diag_create_vars for whoever makes one (`who`: "diag_create", or "reg_create" for the regional means a
// regression plan takes its indices from): the checks, the combined weights and the reciprocals of their sums.
int make_diag(const std::string& who, int nx, int ny, const float* region_w, int n_regions, int n_vars, greb_diag** out) {
  if (int rc = begin_create(who, out, nx, ny, &n_vars, nullptr)) return rc;
  if (n_regions < 0 || n_regions > kDiagMaxRegions)
    return fail(nullptr, GREB_E_INVALID, who + ": n_regions = " + std::to_string(n_regions) + " (0 ... " +
                                             std::to_string(kDiagMaxRegions) + "; the globe is region 0 on top of them)");
  if (n_regions > 0 && !region_w) return fail(nullptr, GREB_E_INVALID, who + ": region_w is NULL with n_regions > 0");
  const size_t np = (size_t)nx * ny;
  for (int k = 0; k < n_regions; ++k)
    for (size_t i = 0; i < np; ++i) {
      const float v = region_w[(size_t)k * np + i];
      if (!(v >= 0.f && v <= 1.f)) { // (a NaN fails both comparisons)
        char buf[160];
        std::snprintf(buf, sizeof(buf), ": region %d: weight %g at row %zu, column %zu is not in [0, 1]", k + 1, (double)v,
                      i / (size_t)nx, i % (size_t)nx);
        return fail(nullptr, GREB_E_INVALID, who + buf);
      }
    }
  greb_diag* d = new (std::nothrow) greb_diag();
  if (!d) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  d->nx = nx; d->ny = ny; d->nr = 1 + n_regions; d->nv = n_vars;
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
      return fail(nullptr, GREB_E_INVALID, who + ": region " + std::to_string(r) + " has zero weight everywhere");
    }
    d->inv_sum[(size_t)r] = 1.0 / sum;
  }
  *out = d;
  return 0;
}
} // namespace

extern "C" {

int greb_diag_create(int nx, int ny, const float* region_w, int n_regions, greb_diag** out) {
  return make_diag("diag_create", nx, ny, region_w, n_regions, kStateVars, out);
}

int greb_diag_create_vars(int nx, int ny, const float* region_w, int n_regions, int n_vars, greb_diag** out) {
  return make_diag("diag_create", nx, ny, region_w, n_regions, n_vars, out);
}

int greb_diag_destroy(greb_diag* d) {
  delete d; // (PerDevice waits for each device before its tables go)
  return 0;
}

int greb_diag_reduce_dev(greb_diag* d, int device, const float* monthly_year_dev, int n_members, float* regions_dev,
                         float* zonal_dev, float* annual_dev, void* stream) {
  if (!d) return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: no plan (greb_diag is NULL)");
  if (!monthly_year_dev) return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: monthly_year_dev is NULL");
  if (n_members < 1) return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: n_members = " + std::to_string(n_members));
  if (!regions_dev && !zonal_dev && !annual_dev)
    return fail(nullptr, GREB_E_INVALID, "diag_reduce_dev: regions_dev, zonal_dev and annual_dev are all NULL");
  if (int rc = check_aligned("diag_reduce_dev", monthly_year_dev, "monthly_year_dev")) return rc;
  if (int rc = check_aligned("diag_reduce_dev", annual_dev, "annual_dev")) return rc;
  if (int rc = use_device("diag_reduce_dev: ", device)) return rc;
  greb_diag::Dev* dv = nullptr;
  if (int rc = diag_on_device(d, device, n_members, regions_dev != nullptr, &dv)) return rc;
  const DiagArgs a = diag_args(d, dv, monthly_year_dev, regions_dev, (size_t)kDiagMonths * d->nv * d->nr, zonal_dev, annual_dev);
  HIP_TRY(nullptr, launch_diag_year(a, n_members, (hipStream_t)stream));
  return 0;
}

} // extern "C"

namespace {
// The four reduced runs, of the state records (greb_engine_run_diag, ...: `who` "run_diag") or of the budget records
// (greb_engine_run_budget_diag, ...: "run_budget_diag").  Everything but where a year's records come from (Records) and how
// many variables they have is the same.
int run_diag(const std::string& who, Records src, greb_engine* e, int years, const float* co2_ppm, greb_diag* d, unsigned what,
             float* regions, float* zonal, float* annual, float* yearly) {
  // argument errors first, before anything touches a device
  if (!d) return fail(e, GREB_E_INVALID, who + ": no plan (greb_diag is NULL)");
  if (int rc = src.check_plan(e, who, d->nv)) return rc;
  if (int rc = check_what(e, who, what, GREB_D_REGIONS | GREB_D_ZONAL | GREB_D_ANNUAL)) return rc;
  float* host[3] = {regions, zonal, annual};
  const Products pr{{"regions", "GREB_D_REGIONS", what & GREB_D_REGIONS}, {"zonal", "GREB_D_ZONAL", what & GREB_D_ZONAL},
                    {"annual", "GREB_D_ANNUAL", what & GREB_D_ANNUAL}};
  if (int rc = pr.check(e, who, host, "", false)) return rc;
  if (!e || years < 1 || !co2_ppm) return fail(e, GREB_E_INVALID, who + ": bad argument (engine, years or co2_ppm)");
  if (int rc = check_engine(e, who, d->nx, d->ny, -1)) return rc;
  const size_t np = (size_t)e->np, nm = (size_t)e->nm, nv = (size_t)src.nv;
  const bool do_r = (what & GREB_D_REGIONS) != 0, do_z = (what & GREB_D_ZONAL) != 0, do_a = (what & GREB_D_ANNUAL) != 0;
  const size_t reg_year = (size_t)12 * nv * d->nr, zon_year = (size_t)12 * nv * e->ny, ann_year = nv * np; // floats per member-year
  const size_t zon_slot = do_z ? nm * zon_year : 0, ann_slot = do_a ? nm * ann_year : 0, out_slot = zon_slot + ann_slot;
  greb_diag::Dev* dv = nullptr;
  // A unit is a year's zonal means and annual maps, made in output slot y & 1 of e->diag_out.  The region series -- the
  // only thing on the device that grows with `years` besides the yearly scalars -- stays there for the whole call.
  RunSink s;
  s.prepare = [&]() -> int {
    if (out_slot) if (int rc = ensure(e, &e->diag_out, &e->diag_out_cap, 2 * out_slot)) return rc;
    if (do_r) if (int rc = ensure(e, &e->diag_reg, &e->diag_reg_cap, nm * years * reg_year)) return rc;
    if (int rc = src.prepare(e)) return rc;
    return diag_on_device(d, e->device, e->nm, do_r, &dv);
  };
  s.year = year_hook(e, &src, [&](const float* mon, int y) -> int {
    float* out = out_slot ? e->diag_out + (size_t)(y & 1) * out_slot : nullptr;
    const DiagArgs g = diag_args(d, dv, mon, do_r ? e->diag_reg + (size_t)y * reg_year : nullptr, (size_t)years * reg_year,
                                 do_z ? out : nullptr, do_a ? out + zon_slot : nullptr);
    HIP_TRY(e, launch_diag_year(g, e->nm, e->stream));
    return 0;
  });
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
} // namespace

extern "C" {

int greb_engine_run_diag(greb_engine* e, int years, const float* co2_ppm, greb_diag* d, unsigned what, float* regions,
                         float* zonal, float* annual, float* yearly) {
  return run_diag("run_diag", Records{}, e, years, co2_ppm, d, what, regions, zonal, annual, yearly);
}

int greb_engine_run_budget_diag(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_diag* d,
                                unsigned what, float* regions, float* zonal, float* annual, float* yearly) {
  Records src;
  if (int rc = src.init(e, "run_budget_diag", true, combo, n_out)) return rc;
  return run_diag("run_budget_diag", src, e, years, co2_ppm, d, what, regions, zonal, annual, yearly);
}

int greb_budget_combine_dev(const float* combo, int n_out, const float* budget_year_dev, int n_members, size_t np, float* out_dev,
                            void* stream) {
  FluxCombo c{};
  if (int rc = make_combo(nullptr, "budget_combine_dev", combo, n_out, &c)) return rc;
  if (!budget_year_dev || !out_dev) return fail(nullptr, GREB_E_INVALID, "budget_combine_dev: budget_year_dev or out_dev is NULL");
  if (n_members < 1) return fail(nullptr, GREB_E_INVALID, "budget_combine_dev: n_members = " + std::to_string(n_members));
  if (np < 4 || (np & 3)) return fail(nullptr, GREB_E_INVALID, "budget_combine_dev: np = " + std::to_string(np) + " (a multiple of four)");
  if (int rc = check_aligned("budget_combine_dev", budget_year_dev, "budget_year_dev")) return rc;
  if (int rc = check_aligned("budget_combine_dev", out_dev, "out_dev")) return rc;
  int ndev = 0, device = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || hipGetDevice(&device) != hipSuccess)
    return fail(nullptr, GREB_E_NOGPU, "budget_combine_dev: no HIP device (no CPU path)");
  HIP_TRY(nullptr, launch_budget_combine(c, budget_year_dev, n_members, np, out_dev, (hipStream_t)stream));
  return 0;
}

} // extern "C"

// ---------------------------------------------------------------- climatology output (greb_clim.hip)
// Grid, member count, each member's control and the products.  Per device: the fp64 sums and the control map's copy.
struct greb_clim {
  int nx = 0, ny = 0, nm = 0;
  int nv = kStateVars;          // variables per month of the records it sums
  unsigned what = 0;
  std::vector<int32_t> control; // [nm], or empty: no control map
  Period period{"sums are"};
  struct Dev { DevBuf<double> S, T; DevBuf<int> control; };
  PerDevice<Dev> devs;
  size_t elems() const { return (size_t)nm * kClimMonths * nv * nx * ny; }
};

namespace {
int clim_on_device(greb_clim* c, int device, greb_clim::Dev** out) {
  return c->devs.get(device, [c](greb_clim::Dev& n) -> int {
    HIP_TRY(nullptr, n.S.alloc(c->elems()));
    if (c->what & GREB_C_TREND) HIP_TRY(nullptr, n.T.alloc(c->elems()));
    if (!c->control.empty()) HIP_TRY(nullptr, n.control.upload(c->control.data(), c->control.size()));
    return 0;
  }, out);
}

// floats of one member's record of each product of one period: MEAN, SEASONS, TREND, the MEAN response, the SEASONS response
Products clim_products(const greb_clim* c) {
  const size_t np = (size_t)c->nx * c->ny;
  const size_t mon = (c->what & GREB_C_MEAN) ? (size_t)kClimMonths * c->nv * np : 0, sea = (c->what & GREB_C_SEASONS) ? (size_t)kClimSeasons * c->nv * np : 0;
  const bool resp = (c->what & GREB_C_RESPONSE) != 0;
  return {{"mean", "GREB_C_MEAN", mon}, {"seasons", "GREB_C_SEASONS", sea},
          {"trend", "GREB_C_TREND", (c->what & GREB_C_TREND) ? (size_t)kClimMonths * c->nv * np : 0},
          {"mean_resp", "GREB_C_RESPONSE with GREB_C_MEAN", resp ? mon : 0}, {"seasons_resp", "GREB_C_RESPONSE with GREB_C_SEASONS", resp ? sea : 0}};
}

ClimFinishArgs clim_finish_args(const greb_clim* c, const greb_clim::Dev* dv, int n_years, float* const out[5]) {
  ClimFinishArgs a{};
  a.S = dv->S.get(); a.T = dv->T.get(); a.control = dv->control.get();
  a.np = (size_t)c->nx * c->ny; a.nv = c->nv; a.n_years = n_years;
  a.mean = out[0]; a.seasons = out[1]; a.trend = out[2]; a.mean_resp = out[3]; a.seasons_resp = out[4];
  return a;
}
} // namespace

extern "C" {

int greb_clim_create(int nx, int ny, int n_members, const int32_t* control, unsigned what, greb_clim** out) {
  return greb_clim_create_vars(nx, ny, n_members, control, what, kStateVars, out);
}

int greb_clim_create_vars(int nx, int ny, int n_members, const int32_t* control, unsigned what, int n_vars, greb_clim** out) {
  if (int rc = begin_create("clim_create", out, nx, ny, &n_vars, &n_members)) return rc;
  if (int rc = check_what(nullptr, "clim_create", what, GREB_C_MEAN | GREB_C_SEASONS | GREB_C_TREND | GREB_C_RESPONSE)) return rc;
  if ((what & GREB_C_RESPONSE) && !(what & (GREB_C_MEAN | GREB_C_SEASONS)))
    return fail(nullptr, GREB_E_INVALID, "clim_create: GREB_C_RESPONSE needs GREB_C_MEAN or GREB_C_SEASONS (it is their difference to "
                                         "the control)");
  if ((what & GREB_C_RESPONSE) && !control)
    return fail(nullptr, GREB_E_INVALID, "clim_create: GREB_C_RESPONSE selected but `control` is NULL");
  if (int rc = check_control("clim_create", control, n_members)) return rc;
  greb_clim* c = new (std::nothrow) greb_clim();
  if (!c) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  c->nx = nx; c->ny = ny; c->nm = n_members; c->what = what; c->nv = n_vars;
  if (control) c->control.assign(control, control + n_members);
  *out = c;
  return 0;
}

int greb_clim_destroy(greb_clim* c) {
  delete c; // (PerDevice waits for each device before its sums go)
  return 0;
}

int greb_clim_add_year_dev(greb_clim* c, int device, const float* monthly_year_dev, int k, void* stream) {
  if (!c) return fail(nullptr, GREB_E_INVALID, "clim_add_year_dev: no plan (greb_clim is NULL)");
  if (!monthly_year_dev) return fail(nullptr, GREB_E_INVALID, "clim_add_year_dev: monthly_year_dev is NULL");
  if (int rc = check_aligned("clim_add_year_dev", monthly_year_dev, "monthly_year_dev")) return rc;
  if (int rc = c->period.check_add("clim_add_year_dev", k, device)) return rc;
  if (int rc = use_device("clim_add_year_dev: ", device)) return rc;
  greb_clim::Dev* dv = nullptr;
  if (int rc = clim_on_device(c, device, &dv)) return rc;
  HIP_TRY(nullptr, launch_clim_add_year(monthly_year_dev, dv->S.get(), dv->T.get(), c->elems(), k, (hipStream_t)stream));
  c->period.advance(k, device);
  return 0;
}

int greb_clim_finish_dev(greb_clim* c, int device, int n_years, float* mean_dev, float* seasons_dev, float* trend_dev,
                         float* mean_resp_dev, float* seasons_resp_dev, void* stream) {
  if (!c) return fail(nullptr, GREB_E_INVALID, "clim_finish_dev: no plan (greb_clim is NULL)");
  const Products pr = clim_products(c);
  float* out[5] = {mean_dev, seasons_dev, trend_dev, mean_resp_dev, seasons_resp_dev};
  if (int rc = pr.check(nullptr, "clim_finish_dev", out, "_dev", true)) return rc;
  if (int rc = c->period.check_finish("clim_finish_dev", n_years, device)) return rc;
  if (int rc = use_device("clim_finish_dev: ", device)) return rc;
  greb_clim::Dev* dv = nullptr;
  if (int rc = clim_on_device(c, device, &dv)) return rc;
  HIP_TRY(nullptr, launch_clim_finish(clim_finish_args(c, dv, n_years, out), c->nm, (hipStream_t)stream));
  c->period.reset();
  return 0;
}

} // extern "C"

namespace {
int run_clim(const std::string& name, Records src, greb_engine* e, int years, const float* co2_ppm, greb_clim* c, int n_periods,
             const int32_t* first_year, const int32_t* n_years, float* mean, float* seasons, float* trend, float* mean_resp,
             float* seasons_resp, float* yearly) {
  // argument errors first, before anything touches a device: the plan, the periods, the outputs, then the engine
  if (!c) return fail(e, GREB_E_INVALID, name + ": no plan (greb_clim is NULL)");
  if (int rc = src.check_plan(e, name, c->nv)) return rc;
  if (years < 1) return fail(e, GREB_E_INVALID, name + ": years = " + std::to_string(years));
  if (n_periods < 1 || !first_year || !n_years)
    return fail(e, GREB_E_INVALID, name + ": n_periods = " + std::to_string(n_periods) + " with first_year / n_years " +
                                       (first_year && n_years ? "given" : "NULL") + " (at least one period is needed)");
  for (int p = 0; p < n_periods; ++p) {
    const std::string who = name + ": period " + std::to_string(p) + " (first_year " + std::to_string(first_year[p]) + ", n_years " +
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
  Products pr = clim_products(c);
  float* host[5] = {mean, seasons, trend, mean_resp, seasons_resp};
  if (int rc = pr.check(e, name, host, "", false)) return rc;
  if (int rc = c->period.check_idle(e, name)) return rc;
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, name + ": bad argument (engine or co2_ppm)");
  if (int rc = check_engine(e, name, c->nx, c->ny, c->nm)) return rc;
  pr.layout((size_t)e->nm);
  greb_clim::Dev* dv = nullptr;
  int p = 0; // the period the current year is in or before
  // A unit is a period's products, made in output slot p & 1 of e->clim_out.  Nothing on the device grows with `years`
  // or `n_periods` (besides the yearly scalars).
  const ProductSink k{e, pr, &e->clim_out, &e->clim_out_cap, host, n_periods};
  RunSink s;
  k.install(s, [&]() -> int {
    if (int rc = src.prepare(e)) return rc;
    return clim_on_device(c, e->device, &dv);
  });
  s.year = [&](const YearCalls& run, int y) -> int {
    const float* mon = nullptr;
    if (int rc = src.integrate(e, run, y, &mon)) return rc;
    while (p < n_periods && y >= first_year[p] + n_years[p]) ++p;
    if (p >= n_periods || y < first_year[p]) return 0; // (a year outside every period is integrated, not summed)
    const int yk = y - first_year[p];
    HIP_TRY(e, launch_clim_add_year(mon, dv->S.get(), dv->T.get(), c->elems(), yk, e->stream));
    if (yk < n_years[p] - 1) return 0;
    if (int rc = run.writing(p)) return rc; // (here, not before the year: only the finish pass writes the slot)
    float* out[5];
    pr.pointers(k.slot(p), out);
    HIP_TRY(e, launch_clim_finish(clim_finish_args(c, dv, n_years[p], out), e->nm, e->stream));
    return run.complete(p);
  };
  return run_years(e, years, co2_ppm, yearly, s);
}
} // namespace

extern "C" {

int greb_engine_run_clim(greb_engine* e, int years, const float* co2_ppm, greb_clim* c, int n_periods, const int32_t* first_year,
                         const int32_t* n_years, float* mean, float* seasons, float* trend, float* mean_resp, float* seasons_resp,
                         float* yearly) {
  return run_clim("run_clim", Records{}, e, years, co2_ppm, c, n_periods, first_year, n_years, mean, seasons, trend, mean_resp,
                  seasons_resp, yearly);
}

int greb_engine_run_budget_clim(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_clim* c,
                                int n_periods, const int32_t* first_year, const int32_t* n_years, float* mean, float* seasons,
                                float* trend, float* mean_resp, float* seasons_resp, float* yearly) {
  Records src;
  if (int rc = src.init(e, "run_budget_clim", true, combo, n_out)) return rc;
  return run_clim("run_budget_clim", src, e, years, co2_ppm, c, n_periods, first_year, n_years, mean, seasons, trend, mean_resp,
                  seasons_resp, yearly);
}

} // extern "C"

// ---------------------------------------------------------------- ensemble output (greb_ens.hip)
// Grid, member count, the products, the probabilities and the member lists -- group g is member[offs[g] ... offs[g + 1])
// in ascending member index, control[k] the control of member[k].  Per device: the lists' copy (one allocation: offs,
// member, control).
struct greb_ens {
  int nx = 0, ny = 0, nm = 0, ng = 0;
  unsigned what = 0;
  EnsProbs probs{};
  bool has_control = false;
  std::vector<int> offs, member, control;
  struct Dev { DevBuf<int> lists; };
  PerDevice<Dev> devs;
};

namespace {
int ens_on_device(greb_ens* s, int device, EnsLists* out) {
  const size_t listed = s->member.size(), n_offs = s->offs.size();
  greb_ens::Dev* dv = nullptr;
  auto make = [s](greb_ens::Dev& n) -> int {
    std::vector<int> all(s->offs);
    all.insert(all.end(), s->member.begin(), s->member.end());
    all.insert(all.end(), s->control.begin(), s->control.end());
    HIP_TRY(nullptr, n.lists.upload(all.data(), all.size()));
    return 0;
  };
  if (int rc = s->devs.get(device, make, &dv)) return rc;
  int* const base = dv->lists.get();
  out->offs = base; out->member = base + n_offs; out->control = s->has_control ? base + n_offs + listed : nullptr;
  return 0;
}

// floats of one group's record of each product, for rows of n elements: MEAN, VAR, the two of RANGE, QUANTILES
Products ens_products(const greb_ens* s, size_t n) {
  const size_t range = (s->what & GREB_S_RANGE) ? n : 0;
  return {{"mean", "GREB_S_MEAN", (s->what & GREB_S_MEAN) ? n : 0}, {"var", "GREB_S_VAR", (s->what & GREB_S_VAR) ? n : 0},
          {"min", "GREB_S_RANGE", range}, {"max", "GREB_S_RANGE", range},
          {"quant", "GREB_S_QUANTILES", (s->what & GREB_S_QUANTILES) ? (size_t)s->probs.n * n : 0}};
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
  if (int rc = begin_create("ens_create", out, nx, ny, nullptr, &n_members)) return rc;
  if (int rc = check_count(nullptr, "ens_create", "n_groups", n_groups, kEnsMaxGroups)) return rc;
  if (!group) return fail(nullptr, GREB_E_INVALID, "ens_create: `group` is NULL");
  if (int rc = check_what(nullptr, "ens_create", what, GREB_S_MEAN | GREB_S_VAR | GREB_S_RANGE | GREB_S_QUANTILES)) return rc;
  std::vector<int> offs, member;
  auto grouped_has_control = [=](int m) -> int {
    if (int rc = check_control_of("ens_create", control, m, n_members)) return rc;
    if (group[m] < 0 || !control || control[m] >= 0) return 0;
    return fail(nullptr, GREB_E_INVALID, "ens_create: member " + std::to_string(m) + " is in group " + std::to_string(group[m]) +
                                             " but has no control (control = -1) while a control map is given");
  };
  if (int rc = group_lists("ens_create", "member", "group", group, n_groups, n_members, &offs, &member, grouped_has_control)) return rc;
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
      if (const int count = offs[(size_t)g + 1] - offs[(size_t)g]; count > kEnsMaxSorted)
        return fail(nullptr, GREB_E_UNSUPPORTED, "ens_create: GREB_S_QUANTILES with group " + std::to_string(g) + " of " +
                                                     std::to_string(count) + " members (at most " +
                                                     std::to_string(kEnsMaxSorted) + " are sorted in one compute unit's LDS)");
  }
  greb_ens* s = new (std::nothrow) greb_ens();
  if (!s) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  s->nx = nx; s->ny = ny; s->nm = n_members; s->ng = n_groups; s->what = what; s->probs = pr; s->has_control = control != nullptr;
  s->offs = offs; s->member = member;
  for (size_t k = 0; control && k < member.size(); ++k) s->control.push_back(control[member[k]]);
  *out = s;
  return 0;
}

int greb_ens_destroy(greb_ens* s) {
  delete s; // (PerDevice waits for each device before its lists go)
  return 0;
}

int greb_ens_reduce_dev(greb_ens* s, int device, const float* x_dev, size_t n, float* mean_dev, float* var_dev, float* min_dev,
                        float* max_dev, float* quant_dev, void* stream) {
  if (!s) return fail(nullptr, GREB_E_INVALID, "ens_reduce_dev: no plan (greb_ens is NULL)");
  if (!x_dev) return fail(nullptr, GREB_E_INVALID, "ens_reduce_dev: x_dev is NULL");
  if (int rc = check_aligned("ens_reduce_dev", x_dev, "x_dev")) return rc;
  if (n < 1) return fail(nullptr, GREB_E_INVALID, "ens_reduce_dev: n = 0");
  float* out[5] = {mean_dev, var_dev, min_dev, max_dev, quant_dev};
  if (int rc = ens_products(s, n).check(nullptr, "ens_reduce_dev", out, "_dev", false)) return rc;
  if (int rc = use_device("ens_reduce_dev: ", device)) return rc;
  EnsLists l{};
  if (int rc = ens_on_device(s, device, &l)) return rc;
  return ens_launch(nullptr, s, l, x_dev, n, out, (hipStream_t)stream);
}

} // extern "C"

namespace {
int run_ens(const std::string& who, Records src, greb_engine* e, int years, const float* co2_ppm, greb_ens* s, float* mean,
            float* var, float* min, float* max, float* quant, float* yearly) {
  // argument errors first, before anything touches a device: the plan, the outputs, then the engine
  if (!s) return fail(e, GREB_E_INVALID, who + ": no plan (greb_ens is NULL)");
  if (years < 1) return fail(e, GREB_E_INVALID, who + ": years = " + std::to_string(years));
  const size_t n = (size_t)12 * src.nv * s->nx * s->ny; // one member's model year
  Products pr = ens_products(s, n);
  float* host[5] = {mean, var, min, max, quant};
  if (int rc = pr.check(e, who, host, "", false)) return rc;
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, who + ": bad argument (engine or co2_ppm)");
  if (int rc = check_engine(e, who, s->nx, s->ny, s->nm)) return rc;
  pr.layout((size_t)s->ng);
  EnsLists l{};
  // A unit is a year's statistics, made in output slot y & 1 of e->ens_out.  Nothing on the device grows with `years`
  // (besides the yearly scalars).
  const ProductSink k{e, pr, &e->ens_out, &e->ens_out_cap, host, years};
  RunSink sink;
  k.install(sink, [&]() -> int {
    if (int rc = src.prepare(e)) return rc;
    return ens_on_device(s, e->device, &l);
  });
  sink.year = year_hook(e, &src, [&](const float* mon, int y) -> int {
    float* out[5];
    pr.pointers(k.slot(y), out);
    return ens_launch(e, s, l, mon, n, out, e->stream);
  });
  return run_years(e, years, co2_ppm, yearly, sink);
}
} // namespace

extern "C" {

int greb_engine_run_ens(greb_engine* e, int years, const float* co2_ppm, greb_ens* s, float* mean, float* var, float* min,
                        float* max, float* quant, float* yearly) {
  return run_ens("run_ens", Records{}, e, years, co2_ppm, s, mean, var, min, max, quant, yearly);
}

int greb_engine_run_budget_ens(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_ens* s,
                               float* mean, float* var, float* min, float* max, float* quant, float* yearly) {
  Records src;
  if (int rc = src.init(e, "run_budget_ens", true, combo, n_out)) return rc;
  return run_ens("run_budget_ens", src, e, years, co2_ppm, s, mean, var, min, max, quant, yearly);
}

} // extern "C"

// ---------------------------------------------------------------- linear-model output (greb_lin.hip)
// Grid, member count, the products and the tables of the USED members in ascending member index: member[k], control[k],
// and per used member a row of `stride` = 16 * ceil(K / 16) doubles of weights (and of the design), zero behind term
// K - 1.  Per device: the tables' copies (one allocation of ints, one of doubles).
struct greb_lin {
  int nx = 0, ny = 0, nm = 0, nk = 0, stride = 0;
  unsigned what = 0;
  bool has_control = false;
  std::vector<int> member, control;   // [n_used]
  std::vector<double> weight, design; // [n_used][stride]; design empty without one
  struct Dev { DevBuf<int> lists; DevBuf<double> tables; };
  PerDevice<Dev> devs;
};

namespace {
int lin_on_device(greb_lin* l, int device, LinTables* out) {
  greb_lin::Dev* dv = nullptr;
  auto make = [l](greb_lin::Dev& n) -> int {
    std::vector<int> lists(l->member);
    lists.insert(lists.end(), l->control.begin(), l->control.end());
    std::vector<double> tables(l->weight);
    tables.insert(tables.end(), l->design.begin(), l->design.end());
    HIP_TRY(nullptr, n.lists.upload(lists.data(), lists.size()));
    HIP_TRY(nullptr, n.tables.upload(tables.data(), tables.size()));
    return 0;
  };
  if (int rc = l->devs.get(device, make, &dv)) return rc;
  const size_t used = l->member.size();
  out->member = dv->lists.get();
  out->control = l->has_control ? dv->lists.get() + used : nullptr;
  out->weight = dv->tables.get();
  out->design = l->design.empty() ? nullptr : dv->tables.get() + l->weight.size();
  out->n_used = (int)used; out->n_terms = l->nk; out->stride = l->stride;
  return 0;
}

// The two products for records of `rec` floats: `coef` has K rows of a record, `rss` one.  An output slot holds coef
// [K][rec], then rss [rec].
Products lin_products(const greb_lin* l, size_t rec) {
  return {{"coef", "GREB_L_COEF", (l->what & GREB_L_COEF) ? rec : 0, (size_t)l->nk}, {"rss", "GREB_L_RSS", (l->what & GREB_L_RSS) ? rec : 0, 1}};
}

int lin_launch(greb_engine* e, const LinTables& t, const float* x, size_t n, float* const out[2], hipStream_t stream) {
  if (out[0]) HIP_TRY(e, launch_lin_coef(x, n, t, out[0], stream));
  if (out[1]) HIP_TRY(e, launch_lin_rss(x, n, t, out[1], stream));
  return 0;
}
} // namespace

extern "C" {

int greb_lin_create(int nx, int ny, int n_members, const double* weight, int n_terms, const int32_t* use, const int32_t* control,
                    const double* design, unsigned what, greb_lin** out) {
  if (int rc = begin_create("lin_create", out, nx, ny, nullptr, &n_members)) return rc;
  if (int rc = check_count(nullptr, "lin_create", "n_terms", n_terms, kLinMaxTerms)) return rc;
  if (int rc = check_what(nullptr, "lin_create", what, GREB_L_COEF | GREB_L_RSS)) return rc;
  if (!weight) return fail(nullptr, GREB_E_INVALID, "lin_create: `weight` is NULL");
  if ((what & GREB_L_RSS) && !design)
    return fail(nullptr, GREB_E_INVALID, "lin_create: GREB_L_RSS selected but `design` is NULL (the residual is that of the fit design * coef)");
  std::vector<int> member, control_of_used;
  if (int rc = used_members("lin_create", use, control, n_members, &member, &control_of_used)) return rc;
  for (const int m : member) {
    for (int k = 0; k < n_terms; ++k) {
      const bool w_ok = std::isfinite(weight[(size_t)k * n_members + m]);
      if (w_ok && (!design || std::isfinite(design[(size_t)m * n_terms + k]))) continue;
      char buf[160];
      std::snprintf(buf, sizeof(buf), "lin_create: %s of term %d, member %d = %g is not finite", w_ok ? "design" : "weight", k, m,
                    w_ok ? design[(size_t)m * n_terms + k] : weight[(size_t)k * n_members + m]);
      return fail(nullptr, GREB_E_INVALID, buf);
    }
  }
  greb_lin* l = new (std::nothrow) greb_lin();
  if (!l) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  l->nx = nx; l->ny = ny; l->nm = n_members; l->nk = n_terms; l->what = what; l->has_control = control != nullptr;
  l->stride = kLinChunk * ((n_terms + kLinChunk - 1) / kLinChunk);
  l->member = member; l->control = control_of_used;
  l->weight.assign(member.size() * l->stride, 0.0);
  if (design) l->design.assign(member.size() * l->stride, 0.0);
  for (size_t u = 0; u < member.size(); ++u) {
    const size_t at = u * (size_t)l->stride;
    const int m = member[u];
    for (int k = 0; k < n_terms; ++k) {
      l->weight[at + k] = weight[(size_t)k * n_members + m];
      if (design) l->design[at + k] = design[(size_t)m * n_terms + k];
    }
  }
  *out = l;
  return 0;
}

int greb_lin_destroy(greb_lin* l) {
  delete l; // (PerDevice waits for each device before its tables go)
  return 0;
}

int greb_lin_reduce_dev(greb_lin* l, int device, const float* x_dev, size_t n, float* coef_dev, float* rss_dev, void* stream) {
  if (!l) return fail(nullptr, GREB_E_INVALID, "lin_reduce_dev: no plan (greb_lin is NULL)");
  if (!x_dev) return fail(nullptr, GREB_E_INVALID, "lin_reduce_dev: x_dev is NULL");
  if (int rc = check_aligned("lin_reduce_dev", x_dev, "x_dev")) return rc;
  if (n < 1) return fail(nullptr, GREB_E_INVALID, "lin_reduce_dev: n = 0");
  float* out[2] = {coef_dev, rss_dev};
  if (int rc = lin_products(l, n).check(nullptr, "lin_reduce_dev", out, "_dev", false)) return rc;
  if (int rc = use_device("lin_reduce_dev: ", device)) return rc;
  LinTables t{};
  if (int rc = lin_on_device(l, device, &t)) return rc;
  return lin_launch(nullptr, t, x_dev, n, out, (hipStream_t)stream);
}

} // extern "C"

namespace {
int run_lin(const std::string& who, Records src, greb_engine* e, int years, const float* co2_ppm, greb_lin* l, float* coef,
            float* rss, float* yearly) {
  // argument errors first, before anything touches a device: the plan, the outputs, then the engine
  if (!l) return fail(e, GREB_E_INVALID, who + ": no plan (greb_lin is NULL)");
  if (years < 1) return fail(e, GREB_E_INVALID, who + ": years = " + std::to_string(years));
  const size_t n = (size_t)12 * src.nv * l->nx * l->ny; // one member's model year
  Products pr = lin_products(l, n);
  float* host[2] = {coef, rss};
  if (int rc = pr.check(e, who, host, "", false)) return rc;
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, who + ": bad argument (engine or co2_ppm)");
  if (int rc = check_engine(e, who, l->nx, l->ny, l->nm)) return rc;
  pr.layout();
  LinTables t{};
  // A unit is a year's coefficients and residual map, made in output slot y & 1 of e->lin_out.  Nothing on the device
  // grows with `years` (besides the yearly scalars).
  const ProductSink k{e, pr, &e->lin_out, &e->lin_out_cap, host, years};
  RunSink sink;
  k.install(sink, [&]() -> int {
    if (int rc = src.prepare(e)) return rc;
    return lin_on_device(l, e->device, &t);
  });
  sink.year = year_hook(e, &src, [&](const float* mon, int y) -> int {
    float* out[2];
    pr.pointers(k.slot(y), out);
    return lin_launch(e, t, mon, n, out, e->stream);
  });
  return run_years(e, years, co2_ppm, yearly, sink);
}
} // namespace

extern "C" {

int greb_engine_run_lin(greb_engine* e, int years, const float* co2_ppm, greb_lin* l, float* coef, float* rss, float* yearly) {
  return run_lin("run_lin", Records{}, e, years, co2_ppm, l, coef, rss, yearly);
}

int greb_engine_run_budget_lin(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_lin* l,
                               float* coef, float* rss, float* yearly) {
  Records src;
  if (int rc = src.init(e, "run_budget_lin", true, combo, n_out)) return rc;
  return run_lin("run_budget_lin", src, e, years, co2_ppm, l, coef, rss, yearly);
}

} // extern "C"

// ---------------------------------------------------------------- covariance output (greb_gram.hip)
// Grid, member count, record count and: the USED members in ascending member index (member[k], control[k]); the records
// that enter a matrix, sorted by block and ascending inside each (record[q], offs[b] ... offs[b + 1] - 1 those of block
// b); the scale map.  Per device: the lists' copy (one allocation: member, control, record, offs), the scale's, and the
// scratch array of the per-record matrices.
struct greb_gram {
  int nx = 0, ny = 0, nm = 0, nrec = 0, nb = 0;
  bool has_control = false;
  std::vector<int> member, control, record, offs;
  std::vector<float> scale; // [ny][nx], or empty: none
  struct Dev { DevBuf<int> lists; DevBuf<float> scale; DevBuf<double> partial; };
  PerDevice<Dev> devs;
  size_t used() const { return member.size(); }
  size_t matrix() const { return (size_t)nb * used() * used(); } // doubles of one call's output
};

namespace {
int gram_on_device(greb_gram* g, int device, GramTables* out) {
  greb_gram::Dev* dv = nullptr;
  auto make = [g](greb_gram::Dev& n) -> int {
    std::vector<int> lists(g->member);
    lists.insert(lists.end(), g->control.begin(), g->control.end());
    lists.insert(lists.end(), g->record.begin(), g->record.end());
    lists.insert(lists.end(), g->offs.begin(), g->offs.end());
    HIP_TRY(nullptr, n.lists.upload(lists.data(), lists.size()));
    if (!g->scale.empty()) HIP_TRY(nullptr, n.scale.upload(g->scale.data(), g->scale.size()));
    HIP_TRY(nullptr, n.partial.alloc(g->record.size() * g->used() * g->used()));
    return 0;
  };
  if (int rc = g->devs.get(device, make, &dv)) return rc;
  const size_t used = g->used(), ctl = g->control.size();
  int* const base = dv->lists.get();
  out->member = base;
  out->control = g->has_control ? base + used : nullptr;
  out->record = base + used + ctl;
  out->offs = base + used + ctl + g->record.size();
  out->scale = dv->scale.get();
  out->partial = dv->partial.get();
  out->n_used = (int)used; out->n_listed = (int)g->record.size(); out->n_blocks = g->nb; out->n_records = g->nrec;
  return 0;
}

int check_gram_len(greb_engine* e, const std::string& who, const greb_gram* g, size_t len) {
  if (len < 1) return fail(e, GREB_E_INVALID, who + ": len = 0");
  if (!g->scale.empty() && len != (size_t)g->nx * g->ny)
    return fail(e, GREB_E_INVALID, who + ": len = " + std::to_string(len) + ", but the plan has a scale map of ny * nx = " +
                                       std::to_string((size_t)g->nx * g->ny) + " elements");
  return 0;
}
} // namespace

extern "C" {

int greb_gram_create(int nx, int ny, int n_members, int n_records, const int32_t* block, int n_blocks, const int32_t* use,
                     const int32_t* control, const float* scale, greb_gram** out) {
  if (int rc = begin_create("gram_create", out, nx, ny, nullptr, &n_members)) return rc;
  if (n_records < 1) return fail(nullptr, GREB_E_INVALID, "gram_create: n_records = " + std::to_string(n_records));
  if (int rc = check_count(nullptr, "gram_create", "n_blocks", n_blocks, kGramMaxBlocks)) return rc;
  if (!block) return fail(nullptr, GREB_E_INVALID, "gram_create: `block` is NULL");
  std::vector<int> offs, record, member, control_of_used;
  if (int rc = group_lists("gram_create", "record", "block", block, n_blocks, n_records, &offs, &record)) return rc;
  if (int rc = used_members("gram_create", use, control, n_members, &member, &control_of_used)) return rc;
  if (member.size() > (size_t)kGramMaxUsed)
    return fail(nullptr, GREB_E_UNSUPPORTED, "gram_create: " + std::to_string(member.size()) + " used members (at most " +
                                                 std::to_string(kGramMaxUsed) + ")");
  const size_t np = (size_t)nx * ny;
  for (size_t i = 0; scale && i < np; ++i)
    if (!(scale[i] >= 0.f && std::isfinite(scale[i]))) { // (a NaN fails the comparison)
      char buf[160];
      std::snprintf(buf, sizeof(buf), "gram_create: scale %g at row %zu, column %zu is negative or not finite", (double)scale[i],
                    i / (size_t)nx, i % (size_t)nx);
      return fail(nullptr, GREB_E_INVALID, buf);
    }
  greb_gram* g = new (std::nothrow) greb_gram();
  if (!g) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  g->nx = nx; g->ny = ny; g->nm = n_members; g->nrec = n_records; g->nb = n_blocks; g->has_control = control != nullptr;
  g->member = member; g->control = control_of_used; g->record = record; g->offs = offs;
  if (scale) g->scale.assign(scale, scale + np);
  *out = g;
  return 0;
}

int greb_gram_destroy(greb_gram* g) {
  delete g; // (PerDevice waits for each device before its tables go)
  return 0;
}

int greb_gram_reduce_dev(greb_gram* g, int device, const float* x_dev, size_t len, double* G_dev, void* stream) {
  if (!g) return fail(nullptr, GREB_E_INVALID, "gram_reduce_dev: no plan (greb_gram is NULL)");
  if (!x_dev) return fail(nullptr, GREB_E_INVALID, "gram_reduce_dev: x_dev is NULL");
  if (int rc = check_aligned("gram_reduce_dev", x_dev, "x_dev")) return rc;
  if (!G_dev) return fail(nullptr, GREB_E_INVALID, "gram_reduce_dev: G_dev is NULL");
  if (reinterpret_cast<uintptr_t>(G_dev) & 7) return fail(nullptr, GREB_E_INVALID, "gram_reduce_dev: G_dev is not 8-byte aligned");
  if (int rc = check_gram_len(nullptr, "gram_reduce_dev", g, len)) return rc;
  if (int rc = use_device("gram_reduce_dev: ", device)) return rc;
  GramTables t{};
  if (int rc = gram_on_device(g, device, &t)) return rc;
  HIP_TRY(nullptr, launch_gram(x_dev, len, t, G_dev, (hipStream_t)stream));
  return 0;
}

} // extern "C"

namespace {
int run_gram(const std::string& who, Records src, greb_engine* e, int years, const float* co2_ppm, greb_gram* g, double* G,
             float* yearly) {
  // argument errors first, before anything touches a device: the plan, the output, then the engine
  if (!g) return fail(e, GREB_E_INVALID, who + ": no plan (greb_gram is NULL)");
  if (years < 1) return fail(e, GREB_E_INVALID, who + ": years = " + std::to_string(years));
  if (g->nrec != 12 * src.nv)
    return fail(e, GREB_E_INVALID, who + ": the plan is for n_records = " + std::to_string(g->nrec) + ", a model year of this run has 12 * " +
                                       std::to_string(src.nv) + " = " + std::to_string(12 * src.nv));
  if (!G) return fail(e, GREB_E_INVALID, who + ": `G` is NULL");
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, who + ": bad argument (engine or co2_ppm)");
  if (int rc = check_engine(e, who, g->nx, g->ny, g->nm)) return rc;
  const size_t len = (size_t)e->np, out = g->matrix(); // doubles of a year's matrices
  GramTables t{};
  // A unit is a year's matrices, made in output slot y & 1 of e->gram_out.  Nothing on the device grows with `years`
  // (besides the yearly scalars).
  auto slot = [&](int u) { return e->gram_out + (size_t)(u & 1) * out; };
  RunSink sink;
  sink.prepare = [&]() -> int {
    if (int rc = ensure(e, &e->gram_out, &e->gram_out_cap, 2 * out)) return rc;
    if (int rc = src.prepare(e)) return rc;
    return gram_on_device(g, e->device, &t);
  };
  sink.year = year_hook(e, &src, [&](const float* mon, int y) -> int {
    HIP_TRY(e, launch_gram(mon, len, t, slot(y), e->stream));
    return 0;
  });
  sink.deliver = [&](int y, int sl) -> int {
    HIP_TRY(e, hipMemcpyAsync(G + (size_t)y * out, slot(sl), out * sizeof(double), hipMemcpyDeviceToHost, e->copy_stream));
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, sink);
}
} // namespace

extern "C" {

int greb_engine_run_gram(greb_engine* e, int years, const float* co2_ppm, greb_gram* g, double* G, float* yearly) {
  return run_gram("run_gram", Records{}, e, years, co2_ppm, g, G, yearly);
}

int greb_engine_run_budget_gram(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_gram* g,
                                double* G, float* yearly) {
  Records src;
  if (int rc = src.init(e, "run_budget_gram", true, combo, n_out)) return rc;
  return run_gram("run_budget_gram", src, e, years, co2_ppm, g, G, yearly);
}

} // extern "C"

// ---------------------------------------------------------------- crossing output (greb_cross.hip)
// Grid, member count, variable count, the events in the caller's order and as the update kernel walks them (CrossTable:
// sorted by variable, then selector), each member's control, the group lists (group g is member[offs[g] ... offs[g + 1]) in
// ascending member index) and the products.  Per device: the state words the products need, the hit bytes and the two
// output slots of FRACTION, and the lists' copy (one allocation: control, offs, member).
struct greb_cross {
  int nx = 0, ny = 0, nm = 0, nv = 0, ne = 0, ng = 0;
  unsigned what = 0;
  CrossTable table{};
  std::vector<int> control, offs, member;
  Period period{"state is"};
  struct Dev { DevBuf<int> first, last, last_miss, count, peak_year, lists; DevBuf<float> peak, frac_out; DevBuf<unsigned char> hit; };
  PerDevice<Dev> devs;
  size_t np() const { return (size_t)nx * ny; }
  size_t elems() const { return (size_t)nm * ne * np(); }    // one state word, one map
  size_t fraction() const { return (size_t)ng * ne * np(); } // floats of a year's FRACTION
};

namespace {
constexpr unsigned kCrossAll = GREB_T_FIRST | GREB_T_LAST | GREB_T_STAY | GREB_T_COUNT | GREB_T_PEAK | GREB_T_FRACTION;

int cross_on_device(greb_cross* c, int device, greb_cross::Dev** out) {
  return c->devs.get(device, [c](greb_cross::Dev& n) -> int {
    const size_t el = c->elems();
    if (c->what & GREB_T_FIRST) HIP_TRY(nullptr, n.first.alloc(el));
    if (c->what & GREB_T_LAST) HIP_TRY(nullptr, n.last.alloc(el));
    if (c->what & GREB_T_STAY) HIP_TRY(nullptr, n.last_miss.alloc(el));
    if (c->what & GREB_T_COUNT) HIP_TRY(nullptr, n.count.alloc(el));
    if (c->what & GREB_T_PEAK) { HIP_TRY(nullptr, n.peak.alloc(el)); HIP_TRY(nullptr, n.peak_year.alloc(el)); }
    if (c->what & GREB_T_FRACTION) { HIP_TRY(nullptr, n.hit.alloc(el)); HIP_TRY(nullptr, n.frac_out.alloc(2 * c->fraction())); }
    std::vector<int> lists(c->control);
    lists.insert(lists.end(), c->offs.begin(), c->offs.end());
    lists.insert(lists.end(), c->member.begin(), c->member.end());
    if (!lists.empty()) HIP_TRY(nullptr, n.lists.upload(lists.data(), lists.size()));
    return 0;
  }, out);
}
const int* cross_control(const greb_cross* c, const greb_cross::Dev* dv) { return c->control.empty() ? nullptr : dv->lists.get(); }
const int* cross_offs(const greb_cross* c, const greb_cross::Dev* dv) { return dv->lists.get() + c->control.size(); }

CrossState cross_state(const greb_cross::Dev* dv) {
  return CrossState{dv->first.get(), dv->last.get(), dv->last_miss.get(), dv->count.get(), dv->peak_year.get(), dv->peak.get(), dv->hit.get()};
}

// year k of x into the state and, with FRACTION, the year's exceedance probabilities into `fraction`
int cross_launch_year(greb_engine* e, const greb_cross* c, const greb_cross::Dev* dv, const float* x, int k, float* fraction,
                      hipStream_t stream) {
  CrossUpdateArgs a{};
  a.x = x; a.control = cross_control(c, dv); a.st = cross_state(dv); a.np = c->np();
  a.n_members = c->nm; a.n_vars = c->nv; a.n_events = c->ne; a.k = k; a.t = c->table;
  HIP_TRY(e, launch_cross_update(a, stream));
  if (c->what & GREB_T_FRACTION)
    HIP_TRY(e, launch_cross_fraction(dv->hit.get(), cross_offs(c, dv), cross_offs(c, dv) + c->offs.size(), c->ng, c->nm, c->ne, c->np(),
                                     fraction, stream));
  return 0;
}

// the six maps, of one word per (member, event, point), and the year's FRACTION
Products cross_maps(const greb_cross* c) {
  auto size = [c](unsigned flag) { return (c->what & flag) ? c->elems() : 0; };
  return {{"first", "GREB_T_FIRST", size(GREB_T_FIRST)}, {"last", "GREB_T_LAST", size(GREB_T_LAST)}, {"stay", "GREB_T_STAY", size(GREB_T_STAY)},
          {"count", "GREB_T_COUNT", size(GREB_T_COUNT)}, {"peak", "GREB_T_PEAK", size(GREB_T_PEAK)}, {"peak_year", "GREB_T_PEAK", size(GREB_T_PEAK)}};
}
Products cross_fraction(const greb_cross* c) { return {{"fraction", "GREB_T_FRACTION", (c->what & GREB_T_FRACTION) ? c->fraction() : 0}}; }
} // namespace

extern "C" {

int greb_cross_create(int nx, int ny, int n_members, int n_vars, const greb_cross_event* events, int n_events, const int32_t* control,
                      const int32_t* group, int n_groups, unsigned what, greb_cross** out) {
  if (int rc = begin_create("cross_create", out, nx, ny, &n_vars, &n_members)) return rc;
  if (int rc = check_what(nullptr, "cross_create", what, kCrossAll)) return rc;
  if (n_events < 1 || n_events > GREB_CROSS_MAX_EVENTS || !events)
    return fail(nullptr, GREB_E_INVALID, "cross_create: n_events = " + std::to_string(n_events) + (events ? "" : " and `events` NULL") +
                                             " (1 ... " + std::to_string(GREB_CROSS_MAX_EVENTS) + ")");
  for (int i = 0; i < n_events; ++i) {
    const greb_cross_event& ev = events[i];
    const std::string who = "cross_create: event " + std::to_string(i) + ": ";
    if (ev.var < 0 || ev.var >= n_vars)
      return fail(nullptr, GREB_E_INVALID, who + "var = " + std::to_string(ev.var) + " (0 ... " + std::to_string(n_vars - 1) + ")");
    if (ev.sel < 0 || ev.sel >= season::kSelectors) return fail(nullptr, GREB_E_INVALID, who + "sel = " + std::to_string(ev.sel) + kSelRange);
    if (ev.rel != 0 && ev.rel != 1) return fail(nullptr, GREB_E_INVALID, who + "rel = " + std::to_string(ev.rel) + " (0 or 1)");
    if (ev.rel && !control) return fail(nullptr, GREB_E_INVALID, who + "rel = 1 (member minus its control) but `control` is NULL");
    if (ev.dir != 1 && ev.dir != -1) return fail(nullptr, GREB_E_INVALID, who + "dir = " + std::to_string(ev.dir) + " (+1: q >= thr, -1: q <= thr)");
    if (!std::isfinite(ev.thr)) {
      char buf[64];
      std::snprintf(buf, sizeof(buf), "thr = %g is not finite", (double)ev.thr);
      return fail(nullptr, GREB_E_INVALID, who + buf);
    }
  }
  if (int rc = check_control("cross_create", control, n_members)) return rc;
  if ((what & GREB_T_FRACTION) && !group)
    return fail(nullptr, GREB_E_INVALID, "cross_create: GREB_T_FRACTION selected but `group` is NULL (it is the share of a group's members)");
  std::vector<int> offs, member;
  if (group) {
    if (int rc = check_count(nullptr, "cross_create", "n_groups", n_groups, GREB_ENS_MAX_GROUPS)) return rc;
    if (int rc = group_lists("cross_create", "member", "group", group, n_groups, n_members, &offs, &member)) return rc;
  }
  greb_cross* c = new (std::nothrow) greb_cross();
  if (!c) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  c->nx = nx; c->ny = ny; c->nm = n_members; c->nv = n_vars; c->ne = n_events; c->what = what;
  if (control) c->control.assign(control, control + n_members);
  if (group) { c->ng = n_groups; c->offs = offs; c->member = member; }
  build_year_table(c->table, events, n_events, [](CrossEv& to, const greb_cross_event& ev) { to.dir = ev.dir; to.thr = ev.thr; });
  *out = c;
  return 0;
}

int greb_cross_destroy(greb_cross* c) {
  delete c; // (PerDevice waits for each device before its state goes)
  return 0;
}

int greb_cross_add_year_dev(greb_cross* c, int device, const float* x_dev, int k, float* fraction_dev, void* stream) {
  if (!c) return fail(nullptr, GREB_E_INVALID, "cross_add_year_dev: no plan (greb_cross is NULL)");
  if (!x_dev) return fail(nullptr, GREB_E_INVALID, "cross_add_year_dev: x_dev is NULL");
  if (int rc = check_aligned("cross_add_year_dev", x_dev, "x_dev")) return rc;
  if (int rc = cross_fraction(c).check(nullptr, "cross_add_year_dev", &fraction_dev, "_dev", true)) return rc;
  if (int rc = c->period.check_add("cross_add_year_dev", k, device)) return rc;
  if (int rc = use_device("cross_add_year_dev: ", device)) return rc;
  greb_cross::Dev* dv = nullptr;
  if (int rc = cross_on_device(c, device, &dv)) return rc;
  if (int rc = cross_launch_year(nullptr, c, dv, x_dev, k, fraction_dev, (hipStream_t)stream)) return rc;
  c->period.advance(k, device);
  return 0;
}

int greb_cross_finish_dev(greb_cross* c, int device, int n_years, int32_t* first_dev, int32_t* last_dev, int32_t* stay_dev,
                          int32_t* count_dev, float* peak_dev, int32_t* peak_year_dev, void* stream) {
  if (!c) return fail(nullptr, GREB_E_INVALID, "cross_finish_dev: no plan (greb_cross is NULL)");
  void* out[6] = {first_dev, last_dev, stay_dev, count_dev, peak_dev, peak_year_dev};
  if (int rc = cross_maps(c).check(nullptr, "cross_finish_dev", out, "_dev", true)) return rc;
  if (int rc = c->period.check_finish("cross_finish_dev", n_years, device)) return rc;
  if (int rc = use_device("cross_finish_dev: ", device)) return rc;
  greb_cross::Dev* dv = nullptr;
  if (int rc = cross_on_device(c, device, &dv)) return rc;
  CrossFinishArgs a{};
  a.st = cross_state(dv); a.n = c->elems(); a.n_years = n_years;
  a.first = (int32_t*)out[0]; a.last = (int32_t*)out[1]; a.stay = (int32_t*)out[2]; a.count = (int32_t*)out[3];
  a.peak = (float*)out[4]; a.peak_year = (int32_t*)out[5];
  if (c->what & ~GREB_T_FRACTION) HIP_TRY(nullptr, launch_cross_finish(a, (hipStream_t)stream));
  c->period.reset();
  return 0;
}

} // extern "C"

namespace {
int run_cross(const std::string& who, Records src, greb_engine* e, int years, const float* co2_ppm, greb_cross* c, int32_t* first,
              int32_t* last, int32_t* stay, int32_t* count, float* peak, int32_t* peak_year, float* fraction, float* yearly) {
  // argument errors first, before anything touches a device: the plan, the outputs, then the engine
  if (!c) return fail(e, GREB_E_INVALID, who + ": no plan (greb_cross is NULL)");
  if (int rc = src.check_plan(e, who, c->nv)) return rc;
  if (years < 1) return fail(e, GREB_E_INVALID, who + ": years = " + std::to_string(years));
  void* host[6] = {first, last, stay, count, peak, peak_year};
  if (int rc = cross_maps(c).check(e, who, host, "", false)) return rc;
  const bool frac = (c->what & GREB_T_FRACTION) != 0;
  if (int rc = cross_fraction(c).check(e, who, &fraction, "", false)) return rc;
  if (int rc = c->period.check_idle(e, who)) return rc;
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, who + ": bad argument (engine or co2_ppm)");
  if (int rc = check_engine(e, who, c->nx, c->ny, c->nm)) return rc;
  const size_t el = c->elems(), fr = c->fraction();
  greb_cross::Dev* dv = nullptr;
  // The state follows every year where the year was integrated.  A unit is a year's FRACTION, made in output slot y & 1 of
  // the plan's frac_out; without FRACTION nothing leaves before the end, and the run makes no copy stream and no events.
  // Nothing on the device grows with `years` (besides the yearly scalars).
  auto slot = [&](int u) { return dv->frac_out.get() + (size_t)(u & 1) * fr; };
  RunSink sink;
  sink.prepare = [&]() -> int {
    if (int rc = ensure(e, &e->monthly_dev, &e->monthly_cap, 2 * year_records(e))) return rc; // the staging slots
    if (int rc = src.prepare(e)) return rc;
    return cross_on_device(c, e->device, &dv);
  };
  sink.year = year_hook(e, &src, [&](const float* mon, int y) -> int {
    return cross_launch_year(e, c, dv, mon, y, frac ? slot(y) : nullptr, e->stream);
  }, frac);
  if (frac)
    sink.deliver = [&](int y, int sl) -> int {
      HIP_TRY(e, hipMemcpyAsync(fraction + (size_t)y * fr, slot(sl), fr * sizeof(float), hipMemcpyDeviceToHost, e->copy_stream));
      return 0;
    };
  // The maps, once, after the last year.  All but STAY are the state words themselves and leave from where they lie; STAY
  // is made IN PLACE over last_miss (element by element; the period is over, and the next year 0 stores the state anew).
  sink.finish = [&]() -> int {
    const CrossState st = cross_state(dv);
    if (host[2]) {
      CrossFinishArgs a{};
      a.st = st; a.n = el; a.n_years = years; a.stay = st.last_miss;
      HIP_TRY(e, launch_cross_finish(a, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
    }
    const void* from[6] = {st.first, st.last, st.last_miss, st.count, st.peak, st.peak_year};
    for (int i = 0; i < 6; ++i)
      if (host[i]) HIP_TRY(e, hipMemcpy(host[i], from[i], el * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, sink);
}
} // namespace

extern "C" {

int greb_engine_run_cross(greb_engine* e, int years, const float* co2_ppm, greb_cross* c, int32_t* first, int32_t* last, int32_t* stay,
                          int32_t* count, float* peak, int32_t* peak_year, float* fraction, float* yearly) {
  return run_cross("run_cross", Records{}, e, years, co2_ppm, c, first, last, stay, count, peak, peak_year, fraction, yearly);
}

int greb_engine_run_budget_cross(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_cross* c,
                                 int32_t* first, int32_t* last, int32_t* stay, int32_t* count, float* peak, int32_t* peak_year,
                                 float* fraction, float* yearly) {
  Records src;
  if (int rc = src.init(e, "run_budget_cross", true, combo, n_out)) return rc;
  return run_cross("run_budget_cross", src, e, years, co2_ppm, c, first, last, stay, count, peak, peak_year, fraction, yearly);
}

} // extern "C"

// ---------------------------------------------------------------- regression output (greb_reg.hip)
// Grid, member count, variable count, a diag plan over the caller's region weights (made by make_diag: the regional means
// the indices are taken from have the bits a greb_diag plan over the same weights returns), the indices in the caller's
// order, the terms in the caller's order (index_of) and as the update kernel walks them (RegTable: sorted by variable, then
// selector), each member's control and the products.  Per device: the term state, the index state, one year's regional
// means, the control's copy; for greb_engine_run_reg the map the products leave through and the INDEX series.
struct greb_reg {
  int nx = 0, ny = 0, nm = 0, nv = 0, nt = 0, ni = 0;
  unsigned what = 0;
  greb_diag* diag = nullptr;
  RegTable table{};
  RegIndexTable itable{};
  int index_of[kRegMaxTerms] = {};
  std::vector<int> control;
  Period period{"state is"};
  struct Dev {
    DevBuf<float> y0, g0, regions, out, series;
    DevBuf<double> sy, sgy, syy, G, sg, sgg;
    DevBuf<int> control;
    size_t series_cap = 0;
  };
  PerDevice<Dev> devs;
  size_t np() const { return (size_t)nx * ny; }
  size_t elems() const { return (size_t)nm * nt * np(); } // one state word, one map
  size_t regions() const { return (size_t)nm * kDiagMonths * nv * diag->nr; }
  ~greb_reg() { delete diag; }
};

namespace {
constexpr unsigned kRegMaps = GREB_R_SLOPE | GREB_R_INTERCEPT | GREB_R_R2;
constexpr unsigned kRegAll = kRegMaps | GREB_R_INDEX;

int reg_on_device(greb_reg* r, int device, greb_reg::Dev** out) {
  return r->devs.get(device, [r](greb_reg::Dev& n) -> int {
    const size_t el = r->elems(), ix = (size_t)r->nm * r->ni;
    HIP_TRY(nullptr, n.y0.alloc(el)); HIP_TRY(nullptr, n.sy.alloc(el)); HIP_TRY(nullptr, n.sgy.alloc(el));
    if (r->what & GREB_R_R2) HIP_TRY(nullptr, n.syy.alloc(el));
    HIP_TRY(nullptr, n.g0.alloc(ix)); HIP_TRY(nullptr, n.G.alloc(ix)); HIP_TRY(nullptr, n.sg.alloc(ix)); HIP_TRY(nullptr, n.sgg.alloc(ix));
    HIP_TRY(nullptr, n.regions.alloc(r->regions()));
    if (!r->control.empty()) HIP_TRY(nullptr, n.control.upload(r->control.data(), r->control.size()));
    return 0;
  }, out);
}

RegState reg_state(const greb_reg::Dev* dv) { return RegState{dv->y0.get(), dv->sy.get(), dv->sgy.get(), dv->syy.get()}; }
RegIndexState reg_index_state(const greb_reg::Dev* dv) { return RegIndexState{dv->g0.get(), dv->G.get(), dv->sg.get(), dv->sgg.get()}; }

// year k of x: its regional means, the indices from them (member m's g to index + m * index_stride where `index` is
// given), then the terms' sums
int reg_launch_year(greb_engine* e, greb_reg* r, int device, const greb_reg::Dev* dv, const float* x, int k, float* index,
                    size_t index_stride, hipStream_t stream) {
  greb_diag::Dev* ddv = nullptr;
  if (int rc = diag_on_device(r->diag, device, r->nm, true, &ddv)) return rc;
  const DiagArgs d = diag_args(r->diag, ddv, x, dv->regions.get(), (size_t)kDiagMonths * r->nv * r->diag->nr, nullptr, nullptr);
  HIP_TRY(e, launch_diag_year(d, r->nm, stream));
  RegIndexArgs ia{};
  ia.regions = dv->regions.get(); ia.control = dv->control.get(); ia.ix = reg_index_state(dv);
  ia.n_members = r->nm; ia.n_vars = r->nv; ia.nr = r->diag->nr; ia.n_indices = r->ni; ia.k = k;
  ia.index = index; ia.index_stride = index_stride; ia.t = r->itable;
  HIP_TRY(e, launch_reg_index(ia, stream));
  RegUpdateArgs a{};
  a.x = x; a.control = dv->control.get(); a.st = reg_state(dv); a.G = dv->G.get(); a.np = r->np();
  a.n_members = r->nm; a.n_vars = r->nv; a.n_terms = r->nt; a.n_indices = r->ni; a.k = k; a.t = r->table;
  HIP_TRY(e, launch_reg_update(a, stream));
  return 0;
}

RegFinishArgs reg_finish_args(const greb_reg* r, const greb_reg::Dev* dv, int n_years, float* slope, float* intercept, float* r2) {
  RegFinishArgs a{};
  a.st = reg_state(dv); a.ix = reg_index_state(dv); a.np = r->np();
  a.n_members = r->nm; a.n_terms = r->nt; a.n_indices = r->ni; a.n_years = n_years;
  for (int t = 0; t < r->nt; ++t) a.index_of[t] = r->index_of[t];
  a.slope = slope; a.intercept = intercept; a.r2 = r2;
  return a;
}

// the three maps, of one float per (member, term, point), and a year's INDEX values
Products reg_maps(const greb_reg* r) {
  auto size = [r](unsigned flag) { return (r->what & flag) ? r->elems() : 0; };
  return {{"slope", "GREB_R_SLOPE", size(GREB_R_SLOPE)}, {"intercept", "GREB_R_INTERCEPT", size(GREB_R_INTERCEPT)}, {"r2", "GREB_R_R2", size(GREB_R_R2)}};
}
Products reg_index(const greb_reg* r) { return {{"index", "GREB_R_INDEX", (r->what & GREB_R_INDEX) ? (size_t)r->nm * r->ni : 0}}; }
} // namespace

extern "C" {

int greb_reg_create(int nx, int ny, int n_members, int n_vars, const float* region_w, int n_regions, const int32_t* control,
                    const greb_reg_index* indices, int n_indices, const greb_reg_term* terms, int n_terms, unsigned what,
                    greb_reg** out) {
  if (int rc = begin_create("reg_create", out, nx, ny, &n_vars, nullptr)) return rc;
  if (n_members < 1 || n_members > GREB_REG_MAX_MEMBERS) // (the member is a grid dimension of the update and finish kernels)
    return fail(nullptr, GREB_E_INVALID, "reg_create: n_members = " + std::to_string(n_members) + " (1 ... " +
                                             std::to_string(GREB_REG_MAX_MEMBERS) + ")");
  if (int rc = check_what(nullptr, "reg_create", what, kRegAll)) return rc;
  if (n_indices < 1 || n_indices > GREB_REG_MAX_INDICES || !indices)
    return fail(nullptr, GREB_E_INVALID, "reg_create: n_indices = " + std::to_string(n_indices) + (indices ? "" : " and `indices` NULL") +
                                             " (1 ... " + std::to_string(GREB_REG_MAX_INDICES) + ")");
  if (n_terms < 1 || n_terms > GREB_REG_MAX_TERMS || !terms)
    return fail(nullptr, GREB_E_INVALID, "reg_create: n_terms = " + std::to_string(n_terms) + (terms ? "" : " and `terms` NULL") +
                                             " (1 ... " + std::to_string(GREB_REG_MAX_TERMS) + ")");
  if (n_regions < 0 || n_regions > kDiagMaxRegions) // (make_diag says the same; here before an index's region is held against it)
    return fail(nullptr, GREB_E_INVALID, "reg_create: n_regions = " + std::to_string(n_regions) + " (0 ... " +
                                             std::to_string(kDiagMaxRegions) + "; the globe is region 0 on top of them)");
  for (int j = 0; j < n_indices; ++j) {
    const greb_reg_index& ix = indices[j];
    const std::string who = "reg_create: index " + std::to_string(j) + ": ";
    if (ix.var < 0 || ix.var >= n_vars)
      return fail(nullptr, GREB_E_INVALID, who + "var = " + std::to_string(ix.var) + " (0 ... " + std::to_string(n_vars - 1) + ")");
    if (ix.sel < 0 || ix.sel >= season::kSelectors) return fail(nullptr, GREB_E_INVALID, who + "sel = " + std::to_string(ix.sel) + kSelRange);
    if (ix.rel != 0 && ix.rel != 1) return fail(nullptr, GREB_E_INVALID, who + "rel = " + std::to_string(ix.rel) + " (0 or 1)");
    if (ix.region < 0 || ix.region > n_regions)
      return fail(nullptr, GREB_E_INVALID, who + "region = " + std::to_string(ix.region) + " (0: the globe, ... " + std::to_string(n_regions) + ")");
  }
  for (int t = 0; t < n_terms; ++t) {
    const greb_reg_term& tm = terms[t];
    const std::string who = "reg_create: term " + std::to_string(t) + ": ";
    if (tm.var < 0 || tm.var >= n_vars)
      return fail(nullptr, GREB_E_INVALID, who + "var = " + std::to_string(tm.var) + " (0 ... " + std::to_string(n_vars - 1) + ")");
    if (tm.sel < 0 || tm.sel >= season::kSelectors) return fail(nullptr, GREB_E_INVALID, who + "sel = " + std::to_string(tm.sel) + kSelRange);
    if (tm.rel != 0 && tm.rel != 1) return fail(nullptr, GREB_E_INVALID, who + "rel = " + std::to_string(tm.rel) + " (0 or 1)");
    if (tm.index < 0 || tm.index >= n_indices)
      return fail(nullptr, GREB_E_INVALID, who + "index = " + std::to_string(tm.index) + " (0 ... " + std::to_string(n_indices - 1) + ")");
    if (tm.rel && !control) return fail(nullptr, GREB_E_INVALID, who + "rel = 1 (member minus its control) but `control` is NULL");
    if (indices[tm.index].rel && !control)
      return fail(nullptr, GREB_E_INVALID, who + "its index " + std::to_string(tm.index) + " has rel = 1 (member minus its control) but `control` is NULL");
  }
  for (int j = 0; j < n_indices; ++j) // (one that no term names)
    if (indices[j].rel && !control)
      return fail(nullptr, GREB_E_INVALID, "reg_create: index " + std::to_string(j) + ": rel = 1 (member minus its control) but `control` is NULL");
  if (int rc = check_control("reg_create", control, n_members)) return rc;
  greb_diag* diag = nullptr;
  if (int rc = make_diag("reg_create", nx, ny, region_w, n_regions, n_vars, &diag)) return rc; // the weights
  greb_reg* r = new (std::nothrow) greb_reg();
  if (!r) { delete diag; return fail(nullptr, GREB_E_INVALID, "out of host memory"); }
  r->nx = nx; r->ny = ny; r->nm = n_members; r->nv = n_vars; r->nt = n_terms; r->ni = n_indices; r->what = what; r->diag = diag;
  if (control) r->control.assign(control, control + n_members);
  for (int j = 0; j < n_indices; ++j) r->itable.ix[j] = RegIndexTable::Ix{indices[j].var, indices[j].sel, indices[j].rel, indices[j].region};
  for (int i = 0; i < n_terms; ++i) r->index_of[i] = terms[i].index;
  build_year_table(r->table, terms, n_terms, [](RegTerm& to, const greb_reg_term& tm) { to.index = tm.index; });
  *out = r;
  return 0;
}

int greb_reg_destroy(greb_reg* r) {
  delete r; // (PerDevice waits for each device before its state goes)
  return 0;
}

int greb_reg_add_year_dev(greb_reg* r, int device, const float* x_dev, int k, float* index_dev, void* stream) {
  if (!r) return fail(nullptr, GREB_E_INVALID, "reg_add_year_dev: no plan (greb_reg is NULL)");
  if (!x_dev) return fail(nullptr, GREB_E_INVALID, "reg_add_year_dev: x_dev is NULL");
  if (int rc = check_aligned("reg_add_year_dev", x_dev, "x_dev")) return rc;
  if (int rc = reg_index(r).check(nullptr, "reg_add_year_dev", &index_dev, "_dev", false)) return rc;
  if (int rc = r->period.check_add("reg_add_year_dev", k, device)) return rc;
  if (int rc = use_device("reg_add_year_dev: ", device)) return rc;
  greb_reg::Dev* dv = nullptr;
  if (int rc = reg_on_device(r, device, &dv)) return rc;
  if (int rc = reg_launch_year(nullptr, r, device, dv, x_dev, k, index_dev, (size_t)r->ni, (hipStream_t)stream)) return rc;
  r->period.advance(k, device);
  return 0;
}

int greb_reg_finish_dev(greb_reg* r, int device, int n_years, float* slope_dev, float* intercept_dev, float* r2_dev, void* stream) {
  if (!r) return fail(nullptr, GREB_E_INVALID, "reg_finish_dev: no plan (greb_reg is NULL)");
  float* out[3] = {slope_dev, intercept_dev, r2_dev};
  if (int rc = reg_maps(r).check(nullptr, "reg_finish_dev", out, "_dev", true)) return rc;
  if (int rc = r->period.check_finish("reg_finish_dev", n_years, device)) return rc;
  if (int rc = use_device("reg_finish_dev: ", device)) return rc;
  greb_reg::Dev* dv = nullptr;
  if (int rc = reg_on_device(r, device, &dv)) return rc;
  HIP_TRY(nullptr, launch_reg_finish(reg_finish_args(r, dv, n_years, out[0], out[1], out[2]), (hipStream_t)stream));
  r->period.reset();
  return 0;
}

} // extern "C"

namespace {
int run_reg(const std::string& who, Records src, greb_engine* e, int years, const float* co2_ppm, greb_reg* r, float* slope,
            float* intercept, float* r2, float* index, float* yearly) {
  // argument errors first, before anything touches a device: the plan, the outputs, then the engine
  if (!r) return fail(e, GREB_E_INVALID, who + ": no plan (greb_reg is NULL)");
  if (int rc = src.check_plan(e, who, r->nv)) return rc;
  if (years < 1) return fail(e, GREB_E_INVALID, who + ": years = " + std::to_string(years));
  float* host[3] = {slope, intercept, r2};
  if (int rc = reg_maps(r).check(e, who, host, "", false)) return rc;
  const bool series = (r->what & GREB_R_INDEX) != 0;
  if (int rc = reg_index(r).check(e, who, &index, "", false)) return rc;
  if (int rc = r->period.check_idle(e, who)) return rc;
  if (!e || !co2_ppm) return fail(e, GREB_E_INVALID, who + ": bad argument (engine or co2_ppm)");
  if (int rc = check_engine(e, who, r->nx, r->ny, r->nm)) return rc;
  const size_t el = r->elems(), ser = (size_t)r->nm * years * r->ni;
  greb_reg::Dev* dv = nullptr;
  // The state follows every year where the year was integrated; nothing leaves before the end, so the run makes no copy
  // stream and no events.  The INDEX series [member][years][index] is the only thing that grows with `years`.
  RunSink sink;
  sink.prepare = [&]() -> int {
    if (int rc = ensure(e, &e->monthly_dev, &e->monthly_cap, 2 * year_records(e))) return rc; // the staging slots
    if (int rc = src.prepare(e)) return rc;
    if (int rc = reg_on_device(r, e->device, &dv)) return rc;
    if ((r->what & kRegMaps) && !dv->out) HIP_TRY(e, dv->out.alloc(el));
    if (series && dv->series_cap < ser) {
      if (dv->series) HIP_TRY(e, hipDeviceSynchronize());
      dv->series_cap = 0;
      HIP_TRY(e, dv->series.alloc(ser));
      dv->series_cap = ser;
    }
    return 0;
  };
  sink.year = year_hook(e, &src, [&](const float* mon, int y) -> int {
    return reg_launch_year(e, r, e->device, dv, mon, y, series ? dv->series.get() + (size_t)y * r->ni : nullptr, (size_t)years * r->ni,
                           e->stream);
  }, false);
  // The maps, once, after the last year: each selected one is made in the plan's output map and leaves from there.
  sink.finish = [&]() -> int {
    for (int i = 0; i < 3; ++i) {
      if (!host[i]) continue;
      float* o = dv->out.get();
      HIP_TRY(e, launch_reg_finish(reg_finish_args(r, dv, years, i == 0 ? o : nullptr, i == 1 ? o : nullptr, i == 2 ? o : nullptr), e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
      HIP_TRY(e, hipMemcpy(host[i], o, el * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (series) {
      HIP_TRY(e, hipStreamSynchronize(e->stream)); // (the index kernels of the last year)
      HIP_TRY(e, hipMemcpy(index, dv->series.get(), ser * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, sink);
}
} // namespace

extern "C" {

int greb_engine_run_reg(greb_engine* e, int years, const float* co2_ppm, greb_reg* r, float* slope, float* intercept, float* r2,
                        float* index, float* yearly) {
  return run_reg("run_reg", Records{}, e, years, co2_ppm, r, slope, intercept, r2, index, yearly);
}

int greb_engine_run_budget_reg(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_reg* r,
                               float* slope, float* intercept, float* r2, float* index, float* yearly) {
  Records src;
  if (int rc = src.init(e, "run_budget_reg", true, combo, n_out)) return rc;
  return run_reg("run_budget_reg", src, e, years, co2_ppm, r, slope, intercept, r2, index, yearly);
}

} // extern "C"

// ---------------------------------------------------------------- derived records (greb_derive.hip)
// Grid, the outputs' programs as the kernel walks them (DeriveWord: the stack slot of every instruction decided here), the
// records they name in ascending order and the caller's fields.  Per device: the program's and the fields' copies.
struct greb_derive {
  int nx = 0, ny = 0, n_out = 0, n_fields = 0;
  std::vector<DeriveWord> words;
  std::vector<unsigned char> src; // the inputs named: j < 5 state j, j < 18 term j - 5, else field j - 18
  bool uses_budget = false;
  int stack_cols = 1, local_cols = 0; // what the kernel keeps in LDS: the deepest stack less its top (at least 1), the locals set
  std::vector<float> fields;      // [n_fields][ny][nx]
  struct Dev { DevBuf<DeriveWord> words; DevBuf<float> fields; };
  PerDevice<Dev> devs;
};

namespace {
int derive_n_out(const greb_derive* v) { return v->n_out; }
int derive_check_engine(greb_engine* e, const std::string& who, const greb_derive* v) { return check_engine(e, who, v->nx, v->ny, -1); }

int derive_on_device(greb_derive* v, int device, greb_derive::Dev** out) {
  return v->devs.get(device, [v](greb_derive::Dev& n) -> int {
    HIP_TRY(nullptr, n.words.upload(v->words.data(), v->words.size()));
    if (v->n_fields) HIP_TRY(nullptr, n.fields.upload(v->fields.data(), v->fields.size()));
    return 0;
  }, out);
}
int derive_on_engine(greb_engine* e, greb_derive* v) {
  greb_derive::Dev* dv = nullptr;
  return derive_on_device(v, e->device, &dv);
}

int derive_launch(greb_engine* e, greb_derive* v, int device, const float* state, const float* budget, int n_members, float* out,
                  hipStream_t stream) {
  greb_derive::Dev* dv = nullptr;
  if (int rc = derive_on_device(v, device, &dv)) return rc;
  DeriveArgs a{};
  a.prog = dv->words.get(); a.fields = dv->fields.get(); a.state = state; a.budget = budget; a.out = out;
  a.np = (size_t)v->nx * v->ny; a.n_words = (int)v->words.size(); a.n_out = v->n_out; a.n_in = (int)v->src.size();
  a.stack_cols = v->stack_cols; a.local_cols = v->local_cols;
  for (size_t s = 0; s < v->src.size(); ++s) a.src[s] = v->src[s];
  HIP_TRY(e, launch_derive(a, n_members, stream));
  return 0;
}
int derive_year(greb_engine* e, greb_derive* v, const float* state, const float* budget, float* out) {
  return derive_launch(e, v, e->device, state, budget, e->nm, out, e->stream);
}
} // namespace

extern "C" {

int greb_derive_create(int nx, int ny, const greb_derive_ins* ins, const int32_t* n_ins, int n_out, const float* fields,
                       int n_fields, greb_derive** out) {
  const std::string who = "derive_create";
  if (int rc = begin_create(who, out, nx, ny, nullptr, nullptr)) return rc;
  if (int rc = check_count(nullptr, who, "n_out", n_out, GREB_MAX_RECORD_VARS)) return rc;
  if (!ins || !n_ins) return fail(nullptr, GREB_E_INVALID, who + ": `ins` or `n_ins` is NULL");
  if (n_fields < 0 || n_fields > GREB_DERIVE_MAX_FIELDS)
    return fail(nullptr, GREB_E_INVALID, who + ": n_fields = " + std::to_string(n_fields) + " (0 ... " +
                                             std::to_string(GREB_DERIVE_MAX_FIELDS) + ")");
  if (n_fields > 0 && !fields) return fail(nullptr, GREB_E_INVALID, who + ": `fields` is NULL with n_fields > 0");
  long long total = 0;
  for (int k = 0; k < n_out; ++k) {
    if (n_ins[k] < 1 || n_ins[k] > GREB_DERIVE_MAX_INS)
      return fail(nullptr, GREB_E_INVALID, who + ": output " + std::to_string(k) + " has " + std::to_string(n_ins[k]) +
                                               " instructions (1 ... " + std::to_string(GREB_DERIVE_MAX_INS) + ")");
    total += n_ins[k];
  }
  if (total > GREB_DERIVE_MAX_TOTAL)
    return fail(nullptr, GREB_E_INVALID, who + ": " + std::to_string(total) + " instructions in all (at most " +
                                             std::to_string(GREB_DERIVE_MAX_TOTAL) + ")");
  const size_t np = (size_t)nx * ny;
  for (int f = 0; f < n_fields; ++f)
    for (size_t i = 0; i < np; ++i)
      if (!std::isfinite(fields[(size_t)f * np + i])) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), ": field %d: value %g at row %zu, column %zu is not finite", f, (double)fields[(size_t)f * np + i],
                      i / (size_t)nx, i % (size_t)nx);
        return fail(nullptr, GREB_E_INVALID, who + buf);
      }
  // First pass: the inputs named, so that an input's slot among the loaded ones is known.  (Indices are checked below.)
  unsigned named = 0;
  for (long long i = 0; i < total; ++i) {
    if (ins[i].op == GREB_DV_STATE && ins[i].arg >= 0 && ins[i].arg < kDeriveStates) named |= 1u << ins[i].arg;
    if (ins[i].op == GREB_DV_TERM && ins[i].arg >= 0 && ins[i].arg < kDeriveTerms) named |= 1u << (kDeriveStates + ins[i].arg);
    if (ins[i].op == GREB_DV_FIELD && ins[i].arg >= 0 && ins[i].arg < n_fields) named |= 1u << (kDeriveRecords + ins[i].arg);
  }
  int slot_of[kDeriveInputs] = {};
  std::vector<unsigned char> src;
  for (int j = 0; j < kDeriveInputs; ++j)
    if ((named >> j) & 1u) { slot_of[j] = (int)src.size(); src.push_back((unsigned char)j); }
  std::vector<DeriveWord> words;
  int deepest = 1, locals = 0;
  const greb_derive_ins* in = ins;
  for (int k = 0; k < n_out; in += n_ins[k], ++k) {
    int depth = 0;
    unsigned set = 0; // locals set so far in this output
    for (int i = 0; i < n_ins[k]; ++i) {
      const int op = in[i].op, arg = in[i].arg;
      const std::string at = who + ": output " + std::to_string(k) + ", instruction " + std::to_string(i);
      auto index_in = [&](const char* what, int n) -> int {
        if (arg >= 0 && arg < n) return 0;
        return fail(nullptr, GREB_E_INVALID, at + ": " + what + " " + std::to_string(arg) + " (0 ... " + std::to_string(n - 1) + ")");
      };
      if (op < 0 || op >= kDeriveOps) return fail(nullptr, GREB_E_INVALID, at + ": unknown op " + std::to_string(op));
      int pops = 0, word_arg = 0;
      bool pushes = true;
      switch (op) {
        case GREB_DV_STATE:
          if (int rc = index_in("state record", kDeriveStates)) return rc;
          word_arg = slot_of[arg];
          break;
        case GREB_DV_TERM:
          if (int rc = index_in("budget term", kDeriveTerms)) return rc;
          word_arg = slot_of[kDeriveStates + arg];
          break;
        case GREB_DV_FIELD:
          if (n_fields == 0) return fail(nullptr, GREB_E_INVALID, at + ": FIELD " + std::to_string(arg) + ", but the plan has no fields (n_fields = 0)");
          if (int rc = index_in("field", n_fields)) return rc;
          word_arg = slot_of[kDeriveRecords + arg];
          break;
        case GREB_DV_CONST: {
          if (!std::isfinite(in[i].value)) {
            char buf[64];
            std::snprintf(buf, sizeof(buf), ": CONST %g is not finite", (double)in[i].value);
            return fail(nullptr, GREB_E_INVALID, at + buf);
          }
          static_assert(sizeof(float) == sizeof(int32_t), "the value's bits travel in a word");
          std::memcpy(&word_arg, &in[i].value, sizeof(float));
        } break;
        case GREB_DV_TEE:
          if (int rc = index_in("local", GREB_DERIVE_MAX_LOCALS)) return rc;
          pops = 1; word_arg = arg; // (the top stays where it is)
          break;
        case GREB_DV_GET:
          if (int rc = index_in("local", GREB_DERIVE_MAX_LOCALS)) return rc;
          if (!((set >> arg) & 1u))
            return fail(nullptr, GREB_E_INVALID, at + ": GET of local " + std::to_string(arg) + ", which no earlier TEE of this output set");
          word_arg = arg;
          break;
        case GREB_DV_SELECT: pops = 3; break;
        default: pops = op >= GREB_DV_NEG ? 1 : 2; break;
      }
      if (depth < pops)
        return fail(nullptr, GREB_E_INVALID, at + ": stack underflow (the op takes " + std::to_string(pops) + " values, the stack holds " +
                                                 std::to_string(depth) + ")");
      if (op == GREB_DV_TEE) { set |= 1u << arg; pushes = false; pops = 0; locals = std::max(locals, arg + 1); }
      depth -= pops;
      // the slot the result goes to; TEE: the slot it copies
      const int slot = op == GREB_DV_TEE ? depth - 1 : depth;
      if (pushes) ++depth;
      if (depth > GREB_DERIVE_MAX_STACK)
        return fail(nullptr, GREB_E_INVALID, at + ": the stack would hold " + std::to_string(depth) + " values (at most " +
                                                 std::to_string(GREB_DERIVE_MAX_STACK) + ")");
      deepest = std::max(deepest, depth);
      words.push_back({op * 8 + slot, word_arg});
    }
    if (depth != 1)
      return fail(nullptr, GREB_E_INVALID, who + ": output " + std::to_string(k) + ", instruction " + std::to_string(n_ins[k] - 1) +
                                               ": the program leaves " + std::to_string(depth) + " values on the stack (exactly one is the output)");
    words.push_back({kDeriveStore * 8, k});
  }
  greb_derive* v = new (std::nothrow) greb_derive();
  if (!v) return fail(nullptr, GREB_E_INVALID, "out of host memory");
  v->nx = nx; v->ny = ny; v->n_out = n_out; v->n_fields = n_fields;
  v->words = std::move(words); v->src = std::move(src);
  v->stack_cols = std::max(1, deepest - 1); v->local_cols = locals;
  v->uses_budget = ((named >> kDeriveStates) & ((1u << kDeriveTerms) - 1u)) != 0;
  if (n_fields) v->fields.assign(fields, fields + (size_t)n_fields * np);
  *out = v;
  return 0;
}

int greb_derive_destroy(greb_derive* v) {
  delete v; // (PerDevice waits for each device before the program's copy goes)
  return 0;
}

int greb_derive_uses_budget(const greb_derive* v) { return v && v->uses_budget ? 1 : 0; }

int greb_derive_apply_dev(greb_derive* v, int device, const float* state_year_dev, const float* budget_year_dev, int n_members,
                          float* out_dev, void* stream) {
  const std::string who = "derive_apply_dev";
  if (!v) return fail(nullptr, GREB_E_INVALID, who + ": no plan (greb_derive is NULL)");
  if (!state_year_dev || !out_dev) return fail(nullptr, GREB_E_INVALID, who + ": state_year_dev or out_dev is NULL");
  if (v->uses_budget && !budget_year_dev)
    return fail(nullptr, GREB_E_INVALID, who + ": budget_year_dev is NULL, but the program names a budget term (GREB_DV_TERM)");
  if (n_members < 1) return fail(nullptr, GREB_E_INVALID, who + ": n_members = " + std::to_string(n_members));
  if (int rc = check_aligned(who, state_year_dev, "state_year_dev")) return rc;
  if (int rc = check_aligned(who, budget_year_dev, "budget_year_dev")) return rc;
  if (int rc = check_aligned(who, out_dev, "out_dev")) return rc;
  if (int rc = use_device("derive_apply_dev: ", device)) return rc;
  return derive_launch(nullptr, v, device, state_year_dev, v->uses_budget ? budget_year_dev : nullptr, n_members, out_dev,
                       (hipStream_t)stream);
}

int greb_engine_run_derived_diag(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_diag* d, unsigned what,
                                 float* regions, float* zonal, float* annual, float* yearly) {
  Records src;
  if (int rc = src.init_derived(e, "run_derived_diag", v)) return rc;
  return run_diag("run_derived_diag", src, e, years, co2_ppm, d, what, regions, zonal, annual, yearly);
}

int greb_engine_run_derived_clim(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_clim* c, int n_periods,
                                 const int32_t* first_year, const int32_t* n_years, float* mean, float* seasons, float* trend,
                                 float* mean_resp, float* seasons_resp, float* yearly) {
  Records src;
  if (int rc = src.init_derived(e, "run_derived_clim", v)) return rc;
  return run_clim("run_derived_clim", src, e, years, co2_ppm, c, n_periods, first_year, n_years, mean, seasons, trend, mean_resp,
                  seasons_resp, yearly);
}

int greb_engine_run_derived_ens(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_ens* s, float* mean,
                                float* var, float* min, float* max, float* quant, float* yearly) {
  Records src;
  if (int rc = src.init_derived(e, "run_derived_ens", v)) return rc;
  return run_ens("run_derived_ens", src, e, years, co2_ppm, s, mean, var, min, max, quant, yearly);
}

int greb_engine_run_derived_lin(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_lin* l, float* coef,
                                float* rss, float* yearly) {
  Records src;
  if (int rc = src.init_derived(e, "run_derived_lin", v)) return rc;
  return run_lin("run_derived_lin", src, e, years, co2_ppm, l, coef, rss, yearly);
}

int greb_engine_run_derived_gram(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_gram* g, double* G,
                                 float* yearly) {
  Records src;
  if (int rc = src.init_derived(e, "run_derived_gram", v)) return rc;
  return run_gram("run_derived_gram", src, e, years, co2_ppm, g, G, yearly);
}

int greb_engine_run_derived_cross(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_cross* c, int32_t* first,
                                  int32_t* last, int32_t* stay, int32_t* count, float* peak, int32_t* peak_year, float* fraction,
                                  float* yearly) {
  Records src;
  if (int rc = src.init_derived(e, "run_derived_cross", v)) return rc;
  return run_cross("run_derived_cross", src, e, years, co2_ppm, c, first, last, stay, count, peak, peak_year, fraction, yearly);
}

int greb_engine_run_derived_reg(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_reg* r, float* slope,
                                float* intercept, float* r2, float* index, float* yearly) {
  Records src;
  if (int rc = src.init_derived(e, "run_derived_reg", v)) return rc;
  return run_reg("run_derived_reg", src, e, years, co2_ppm, r, slope, intercept, r2, index, yearly);
}

} // extern "C"
