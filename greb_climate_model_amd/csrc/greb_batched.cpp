// greb_batched.cpp -- the batched single routines and their table cache, point physics, the launch-order, variant and deal
// queries, the tuning hooks.
#include "greb_host.h"

#include <cstring>
#include <mutex>

using namespace greb;
using namespace greb::host;

#define HIP_TRY0(expr) HIP_TRY(nullptr, expr)

namespace {
int batched_common(const greb_params* p, int nx, int ny, int batch, int device) {
  if (!p || !grid_ok(nx, ny) || batch < 1) return fail(nullptr, GREB_E_INVALID, "batched: bad argument");
  return use_device("batched: ", device);
}

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

extern "C" {

#ifdef GREB_TUNING
// diagnostic builds only (not part of include/greb_engine.h): where the fused member kernel writes its stamps,
// [n_members][8 waves][8] unsigned long long on the device, then the item records [n_members][kMaxChunks][8]
// (tools/stamp_member.py); NULL switches them off
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
  if (!p || !grid_ok(nx, ny) || batch < 1 || sweeps < 1)
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
      DevBuf<RowTables> made;
      HIP_TRY0(made.upload(&t, 1));
      tab_dev = made.release();
      g_tab_cache.entries.push_back({dev, tab_dev, t, ++g_tab_cache.clock});
    }
  }
  for (int i = 0; i < sweeps; ++i)
    HIP_TRY0(launch_diffusion(T1_dev, wz_dev, dX_dev, tab_dev, t, nx, ny, batch, strict != 0, (hipStream_t)stream));
  return 0;
}

int greb_diffusion_launch_order(const greb_params* p, int nx, int ny, int batch, int* field, int* k0, int* k1, int* up,
                                int capacity) {
  if (!p || !grid_ok(nx, ny) || batch < 1 || capacity < 0 ||
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

static_assert(GREB_V_FLUX == kVFlux && GREB_V_SWITCHES == kVExp && GREB_V_BUDGET == kVBudget && GREB_V_FORCING == kVForce &&
              GREB_V_BOUNDARY == kVBound, "variant bits mirror the ABI");

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

int greb_member_chunk_table(int schedule, int nsteps, int* end, int capacity) {
  if (schedule < 0 || schedule >= kNChunkSchedules || nsteps < 1 || capacity < 0 || (capacity > 0 && !end))
    return fail(nullptr, GREB_E_INVALID, "member_chunk_table: bad argument");
  const ChunkTable t = chunk_table(schedule, nsteps);
  for (int c = 0; c < t.n && c < capacity; ++c) end[c] = t.end[c];
  return t.n;
}

long long greb_member_queue_capacity(int members, int schedule, int nsteps) {
  if (schedule < 0 || schedule >= kNChunkSchedules || nsteps < 1 || members < 1 || members > kMaxDealtMembers)
    return fail(nullptr, GREB_E_INVALID, "member_queue_capacity: bad argument");
  return (long long)members * chunk_table(schedule, nsteps).n;
}

int greb_member_deal_cover(int strict, int* counts) {
  if (!counts) return fail(nullptr, GREB_E_INVALID, "member_deal_cover: bad argument");
  member_deal_cover(strict != 0, counts);
  return 0;
}

int greb_member_lds_table(int strict, int* records, int capacity) {
  if (capacity < 0 || (capacity > 0 && !records)) return fail(nullptr, GREB_E_INVALID, "member_lds_table: bad argument");
  return member_lds_table(strict != 0, records, capacity);
}

int greb_member_lds_map(int* words8) {
  if (!words8) return fail(nullptr, GREB_E_INVALID, "member_lds_map: bad argument");
  member_lds_map(words8);
  return 0;
}

int greb_substep_launch_order(const greb_params* p, int nx, int ny, int n_members, const float* kappa, int* field, int* k0,
                              int* k1, int capacity) {
  if (!p || !grid_ok(nx, ny) || n_members < 1 || capacity < 0 || (capacity > 0 && (!field || !k0 || !k1)))
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
  if (!p || !grid_ok(nx, ny) || n_members < 1 || slots < 1 || capacity < 0 ||
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
  DevBuf<float> a, b, c;
  HIP_TRY0(a.upload(T1, n)); HIP_TRY0(b.upload(wz, n)); HIP_TRY0(c.alloc(n));
  if (int rc = greb_diffusion_batched_dev(p, nx, ny, batch, a.get(), b.get(), c.get(), strict, 1, nullptr)) return rc;
  HIP_TRY0(hipDeviceSynchronize());
  HIP_TRY0(hipMemcpy(dX, c.get(), n * 4, hipMemcpyDeviceToHost));
  return 0;
}

static int adv_or_circ(bool circ, const greb_params* p, int nx, int ny, int batch, const float* X, const float* wz,
                       const float* u, const float* v, float* dX, int strict, int device) {
  if (int rc = batched_common(p, nx, ny, batch, device)) return rc;
  const size_t n = (size_t)batch * nx * ny;
  DevBuf<float> a, b, c, d, o, scr;
  RowTables t; compute_row_tables(*p, p->kappa, nx, ny, t);
  DevBuf<RowTables> tab;
  HIP_TRY0(tab.upload(&t, 1));
  RowTables* const tab_dev = tab.get();
  HIP_TRY0(a.upload(X, n)); HIP_TRY0(b.upload(wz, n)); HIP_TRY0(c.upload(u, n));
  HIP_TRY0(d.upload(v, n)); HIP_TRY0(o.alloc(n));
  if (circ) {
    HIP_TRY0(scr.alloc(3 * n));
    HIP_TRY0(launch_circulation(a.get(), b.get(), c.get(), d.get(), o.get(), scr.get(), tab_dev, t, nx, ny, batch, nsub_of(*p), strict != 0, nullptr));
  } else {
    HIP_TRY0(launch_advection(a.get(), b.get(), c.get(), d.get(), o.get(), tab_dev, nx, ny, batch, strict != 0, nullptr));
  }
  HIP_TRY0(hipDeviceSynchronize());
  HIP_TRY0(hipMemcpy(dX, o.get(), n * 4, hipMemcpyDeviceToHost));
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
  DevBuf<float> in, out;
  HIP_TRY(e, in.upload(in5, 5 * np)); HIP_TRY(e, out.alloc(15 * np));
  PointArgs a{};
  a.nx = e->nx; a.ny = e->ny; a.np = e->np; a.ityr = ityr; a.co2 = co2;
  a.z_topo = e->z_topo; a.glacier = e->glacier; a.sw_solar = e->sw_solar; a.tclim = e->tclim;
  a.uclim = e->uclim; a.vclim = e->vclim; a.mldclim = e->mldclim; a.cldclim = e->cldclim; a.swetclim = e->swetclim;
  a.z_ocean = e->z_ocean; a.wz_air = e->wz_air; a.phys = e->h_phys[0]; a.in5 = in.get(); a.out15 = out.get();
  a.xsw = e->h_xsw[0]; a.qclim = e->qclim; // (member 0's physics and switches)
  HIP_TRY(e, launch_point_physics(a, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  HIP_TRY(e, hipMemcpy(out15, out.get(), 15 * np * 4, hipMemcpyDeviceToHost));
  return 0;
}

} // extern "C"
