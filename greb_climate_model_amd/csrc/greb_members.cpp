// greb_members.cpp -- what the members of an engine are set to after it is made: experiments, forcing tables and member
// forcing, boundary sets; and the forcing-record queries.
#include "greb_host.h"

#include <cmath>
#include <cstdio>

using namespace greb;
using namespace greb::host;

namespace {
bool is_forced(const greb_member_forcing& f) { return f.co2_pattern >= 0 || f.solar_table >= 0 || !(f.solar_scale == 1.f); }

// An engine whose members share one flux-correction set gives every member a copy of it.  The copies are made on a NEW
// buffer; the engine takes it after its correction index -- one small copy, the LAST step of a call that can fail.
int own_corrections(greb_engine* e, const char* who) {
  const size_t nm = (size_t)e->nm, set = (size_t)3 * kNT * e->np;
  HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream));
  DevBuf<float> corr;
  HIP_STEP(e, who, "hipMalloc of the members' correction sets", corr.alloc(nm * set));
  for (size_t m = 0; m < nm; ++m)
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(corr.get() + m * set, e->corr, set * sizeof(float), hipMemcpyDeviceToDevice));
  std::vector<int> corr_index(nm);
  for (size_t m = 0; m < nm; ++m) corr_index[m] = (int)m;
  HIP_STEP(e, who, "hipMemcpy", hipMemcpy(e->corr_index, corr_index.data(), nm * sizeof(int), hipMemcpyHostToDevice));
  adopt(e->corr, corr);
  e->shared_corr = false;
  return 0;
}
} // namespace

extern "C" {

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
  const char* who = "set_member_experiments: ";
  DevBuf<unsigned> xsw_dev;
  if (!uniform) {
    HIP_STEP(e, who, "hipMalloc", xsw_dev.alloc(nm));
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(xsw_dev.get(), sw.data(), nm * sizeof(unsigned), hipMemcpyHostToDevice));
    // members that now differ need a correction set each: copies of the shared one
    if (e->shared_corr && nm > 1) if (int rc = own_corrections(e, who)) return rc;
    adopt(e->xsw_dev, xsw_dev);
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
  DevBuf<float> space, season, solar;
  if (n_patterns > 0) {
    std::vector<float> ones;
    if (!co2_season) ones.assign((size_t)n_patterns * kNT, 1.f);
    HIP_STEP(e, who, "hipMalloc", space.alloc((size_t)n_patterns * np));
    HIP_STEP(e, who, "hipMalloc", season.alloc((size_t)n_patterns * kNT));
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(space.get(), co2_space, (size_t)n_patterns * np * sizeof(float), hipMemcpyHostToDevice));
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(season.get(), co2_season ? co2_season : ones.data(), (size_t)n_patterns * kNT * sizeof(float),
                                          hipMemcpyHostToDevice));
  }
  if (n_solar > 0) {
    HIP_STEP(e, who, "hipMalloc", solar.alloc((size_t)n_solar * kNT * ny));
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(solar.get(), sw_solar, (size_t)n_solar * kNT * ny * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream)); // nothing in flight reads the old ones
  adopt(e->f_space, space); adopt(e->f_season, season); adopt(e->f_solar, solar);
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
    DevBuf<MemberForcing> dev; // the new words first; the engine takes them once nothing in flight reads the old ones
    HIP_TRY(e, dev.upload(w.data(), nm));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    adopt(e->force_dev, dev);
  }
  e->h_force.assign(f, f + nm);
  e->forced_members = forced;
  return 0;
}

static_assert(sizeof(greb_member_sst) == sizeof(MemberSst) && sizeof(MemberSst) == 8, "the kernels read greb_member_sst as it is");

int greb_engine_set_sst_tables(greb_engine* e, int n_patterns, const float* anom, const float* weight, const float* season) {
  const char* who = "set_sst_tables: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (n_patterns < 0 || n_patterns > GREB_MAX_SST_PATTERNS)
    return fail(e, GREB_E_INVALID, who + ("n_patterns = " + std::to_string(n_patterns)) + " (0 ... " + std::to_string(GREB_MAX_SST_PATTERNS) + ")");
  if (n_patterns > 0 && !anom) return fail(e, GREB_E_INVALID, std::string(who) + "anom is NULL with n_patterns > 0");
  const size_t np = (size_t)e->np, nx = (size_t)e->nx;
  char buf[200];
  for (int k = 0; k < n_patterns; ++k) {
    for (size_t i = 0; i < np; ++i) {
      const float v = anom[(size_t)k * np + i];
      if (!std::isfinite(v)) {
        std::snprintf(buf, sizeof(buf), "%sanom: pattern %d: value %g at row %zu, column %zu is not finite", who, k, (double)v, i / nx, i % nx);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
    for (size_t i = 0; weight && i < np; ++i) {
      const float v = weight[(size_t)k * np + i];
      if (!(v >= 0.f && v <= 1.f)) { // (a NaN fails both comparisons)
        std::snprintf(buf, sizeof(buf), "%sweight: pattern %d: weight %g at row %zu, column %zu is not in [0, 1]", who, k, (double)v, i / nx,
                      i % nx);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
    for (int t = 0; season && t < kNT; ++t) {
      const float v = season[(size_t)k * kNT + t];
      if (!std::isfinite(v)) {
        std::snprintf(buf, sizeof(buf), "%sseason: pattern %d: value %g at step %d is not finite", who, k, (double)v, t + 1);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
  }
  for (size_t m = 0; m < e->h_sst.size(); ++m) // the members' current indices must stay inside the new tables
    if (e->h_sst[m].pattern >= n_patterns) {
      std::snprintf(buf, sizeof(buf), "%smember %zu is prescribed with pattern %d: outside the new %d patterns (change or clear the member "
                    "SST first)", who, m, e->h_sst[m].pattern, n_patterns);
      return fail(e, GREB_E_INVALID, buf);
    }
  HIP_TRY(e, hipSetDevice(e->device));
  // new buffers first; the engine changes only once they are complete
  DevBuf<float> d_anom, d_weight, d_season;
  if (n_patterns > 0) {
    std::vector<float> ones;
    if (!season) ones.assign((size_t)n_patterns * kNT, 1.f);
    HIP_STEP(e, who, "hipMalloc / hipMemcpy of anom", d_anom.upload(anom, (size_t)n_patterns * np));
    if (weight) HIP_STEP(e, who, "hipMalloc / hipMemcpy of weight", d_weight.upload(weight, (size_t)n_patterns * np));
    HIP_STEP(e, who, "hipMalloc / hipMemcpy of season", d_season.upload(season ? season : ones.data(), (size_t)n_patterns * kNT));
  }
  HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream)); // nothing in flight reads the old ones
  adopt(e->s_anom, d_anom); adopt(e->s_weight, d_weight); adopt(e->s_season, d_season);
  e->n_sst = n_patterns;
  return 0;
}

int greb_engine_set_member_sst(greb_engine* e, const greb_member_sst* s) {
  const char* who = "set_member_sst: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (!s) { // every member {-1, .}: the kernels of an engine without any of this again
    e->h_sst.clear();
    e->sst_members = 0;
    return 0;
  }
  const size_t nm = (size_t)e->nm;
  char buf[200];
  int prescribed = 0;
  for (size_t m = 0; m < nm; ++m) {
    buf[0] = 0;
    if (s[m].pattern < -1 || s[m].pattern >= e->n_sst)
      std::snprintf(buf, sizeof(buf), "%smember %zu: pattern %d is outside -1 ... %d (set_sst_tables gave %d patterns)", who, m, s[m].pattern,
                    e->n_sst - 1, e->n_sst);
    else if (s[m].pattern >= 0 && !std::isfinite(s[m].amp))
      std::snprintf(buf, sizeof(buf), "%smember %zu: amp %g is not finite", who, m, (double)s[m].amp);
    if (buf[0]) return fail(e, GREB_E_INVALID, buf);
    prescribed += s[m].pattern >= 0;
  }
  if (prescribed > 0) {
    std::vector<MemberSst> w(nm);
    for (size_t m = 0; m < nm; ++m) // (amp of a member without a pattern is never read: any bits may stand there)
      w[m] = MemberSst{s[m].pattern, s[m].pattern >= 0 ? s[m].amp : 0.f};
    HIP_TRY(e, hipSetDevice(e->device));
    DevBuf<MemberSst> dev; // the new words first; the engine takes them once nothing in flight reads the old ones
    DevBuf<MemberForcing> neutral; // what the forcing-aware kernels of the launch take when no member is forced
    HIP_STEP(e, who, "hipMalloc / hipMemcpy of the members' words", dev.upload(w.data(), nm));
    if (!e->neutral_force_dev) {
      const std::vector<MemberForcing> n(nm, MemberForcing{-1, 1.f, -1, 1.f});
      HIP_STEP(e, who, "hipMalloc / hipMemcpy of the neutral forcing words", neutral.upload(n.data(), nm));
    }
    HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream));
    if (neutral) adopt(e->neutral_force_dev, neutral);
    adopt(e->sst_dev, dev);
  }
  e->h_sst.assign(s, s + nm);
  e->sst_members = prescribed;
  return 0;
}

static_assert(sizeof(greb_member_noise) == sizeof(MemberNoise) && sizeof(MemberNoise) == 16, "the kernels read greb_member_noise as it is");

int greb_engine_set_noise_tables(greb_engine* e, int n_patterns, const float* sigma, const float* season, const int32_t* cell_x,
                                 const int32_t* cell_y, const int32_t* hold) {
  const char* who = "set_noise_tables: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (n_patterns < 0 || n_patterns > GREB_MAX_NOISE_PATTERNS)
    return fail(e, GREB_E_INVALID, who + ("n_patterns = " + std::to_string(n_patterns)) + " (0 ... " + std::to_string(GREB_MAX_NOISE_PATTERNS) + ")");
  if (n_patterns > 0 && !sigma) return fail(e, GREB_E_INVALID, std::string(who) + "sigma is NULL with n_patterns > 0");
  const size_t np = (size_t)e->np, nx = (size_t)e->nx, ny = (size_t)e->ny;
  char buf[200];
  std::vector<int> cells((size_t)n_patterns * (kNoiseRows + ny));
  for (int k = 0; k < n_patterns; ++k) {
    for (size_t i = 0; i < np; ++i) {
      const float v = sigma[(size_t)k * np + i];
      if (!(v >= 0.f && std::isfinite(v))) { // (a NaN fails the comparison)
        std::snprintf(buf, sizeof(buf), "%ssigma: pattern %d: value %g at row %zu, column %zu is negative or not finite", who, k, (double)v,
                      i / nx, i % nx);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
    for (int t = 0; season && t < kNT; ++t) {
      const float v = season[(size_t)k * kNT + t];
      if (!(v >= 0.f && std::isfinite(v))) {
        std::snprintf(buf, sizeof(buf), "%sseason: pattern %d: value %g at step %d is negative or not finite", who, k, (double)v, t + 1);
        return fail(e, GREB_E_INVALID, buf);
      }
    }
    const int cx = cell_x ? cell_x[k] : 1, cy = cell_y ? cell_y[k] : 1, h = hold ? hold[k] : 1;
    buf[0] = 0;
    if (cx != 1 && cx != 2 && cx != 4) std::snprintf(buf, sizeof(buf), "%scell_x: pattern %d: %d is not 1, 2 or 4", who, k, cx);
    else if (cy < 1 || cy > (int)ny) std::snprintf(buf, sizeof(buf), "%scell_y: pattern %d: %d is outside 1 ... %zu", who, k, cy, ny);
    else if (h < 1) std::snprintf(buf, sizeof(buf), "%shold: pattern %d: %d is less than 1", who, k, h);
    if (buf[0]) return fail(e, GREB_E_INVALID, buf);
    int* c = cells.data() + (size_t)k * (kNoiseRows + ny);
    c[kNoiseShift] = cx == 1 ? 0 : (cx == 2 ? 1 : 2);
    c[kNoiseHold] = h;
    for (size_t j = 0; j < ny; ++j) c[kNoiseRows + j] = (int)((j / (size_t)cy) * (nx / (size_t)cx)); // (nx is a multiple of 4)
  }
  for (size_t m = 0; m < e->h_noise.size(); ++m) // the members' current indices must stay inside the new tables
    if (e->h_noise[m].pattern >= n_patterns) {
      std::snprintf(buf, sizeof(buf), "%smember %zu is noisy with pattern %d: outside the new %d patterns (change or clear the member "
                    "noise first)", who, m, e->h_noise[m].pattern, n_patterns);
      return fail(e, GREB_E_INVALID, buf);
    }
  HIP_TRY(e, hipSetDevice(e->device));
  // new buffers first; the engine changes only once they are complete
  DevBuf<float> d_sigma, d_season;
  DevBuf<int> d_cells;
  if (n_patterns > 0) {
    std::vector<float> ones;
    if (!season) ones.assign((size_t)n_patterns * kNT, 1.f);
    HIP_STEP(e, who, "hipMalloc / hipMemcpy of sigma", d_sigma.upload(sigma, (size_t)n_patterns * np));
    HIP_STEP(e, who, "hipMalloc / hipMemcpy of season", d_season.upload(season ? season : ones.data(), (size_t)n_patterns * kNT));
    HIP_STEP(e, who, "hipMalloc / hipMemcpy of the cell words", d_cells.upload(cells.data(), cells.size()));
  }
  HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream)); // nothing in flight reads the old ones
  adopt(e->n_sigma, d_sigma); adopt(e->n_season, d_season); adopt(e->n_cells, d_cells);
  e->n_noise = n_patterns;
  return 0;
}

int greb_engine_set_member_noise(greb_engine* e, const greb_member_noise* s) {
  const char* who = "set_member_noise: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (!s) { // every member {-1, ...}: the kernels of an engine without any of this again
    e->h_noise.clear();
    e->noisy_members = 0;
    return 0;
  }
  const size_t nm = (size_t)e->nm;
  char buf[200];
  int noisy = 0;
  for (size_t m = 0; m < nm; ++m) {
    buf[0] = 0;
    if (s[m].pattern < -1 || s[m].pattern >= e->n_noise)
      std::snprintf(buf, sizeof(buf), "%smember %zu: pattern %d is outside -1 ... %d (set_noise_tables gave %d patterns)", who, m, s[m].pattern,
                    e->n_noise - 1, e->n_noise);
    else if (s[m].pattern >= 0 && !std::isfinite(s[m].amp))
      std::snprintf(buf, sizeof(buf), "%smember %zu: amp %g is not finite", who, m, (double)s[m].amp);
    if (buf[0]) return fail(e, GREB_E_INVALID, buf);
    noisy += s[m].pattern >= 0;
  }
  if (noisy > 0) {
    std::vector<MemberNoise> w(nm);
    for (size_t m = 0; m < nm; ++m) // (the other words of a member without a pattern are never read)
      w[m] = s[m].pattern >= 0 ? MemberNoise{s[m].pattern, s[m].amp, s[m].seed_lo, s[m].seed_hi} : MemberNoise{-1, 0.f, 0u, 0u};
    HIP_TRY(e, hipSetDevice(e->device));
    DevBuf<MemberNoise> dev; // the new words first; the engine takes them once nothing in flight reads the old ones
    DevBuf<MemberForcing> neutral; // what the forcing-aware kernels of the launch take when no member is forced
    HIP_STEP(e, who, "hipMalloc / hipMemcpy of the members' words", dev.upload(w.data(), nm));
    if (!e->neutral_force_dev) {
      const std::vector<MemberForcing> n(nm, MemberForcing{-1, 1.f, -1, 1.f});
      HIP_STEP(e, who, "hipMalloc / hipMemcpy of the neutral forcing words", neutral.upload(n.data(), nm));
    }
    HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream));
    if (neutral) adopt(e->neutral_force_dev, neutral);
    adopt(e->noise_dev, dev);
  }
  e->h_noise.assign(s, s + nm);
  e->noisy_members = noisy;
  return 0;
}

int greb_engine_get_noise(greb_engine* e, int member, int64_t step, float* out) {
  const char* who = "get_noise: ";
  if (!e) return fail(nullptr, GREB_E_INVALID, std::string(who) + "no engine (greb_engine is NULL)");
  if (!out) return fail(e, GREB_E_INVALID, std::string(who) + "out is NULL");
  if (member < 0 || member >= e->nm)
    return fail(e, GREB_E_INVALID, who + ("member " + std::to_string(member)) + " is outside 0 ... " + std::to_string(e->nm - 1));
  if (step < 0) return fail(e, GREB_E_INVALID, who + ("step " + std::to_string((long long)step)) + " is negative");
  if (e->h_noise.empty() || e->h_noise[(size_t)member].pattern < 0)
    return fail(e, GREB_E_INVALID, who + ("member " + std::to_string(member)) + " names no noise pattern (set_member_noise)");
  const greb_member_noise& s = e->h_noise[(size_t)member];
  HIP_TRY(e, hipSetDevice(e->device));
  DevBuf<float> dev;
  HIP_STEP(e, who, "hipMalloc", dev.alloc((size_t)e->np));
  HIP_STEP(e, who, "the query kernel", launch_noise_field(MemberNoise{s.pattern, s.amp, s.seed_lo, s.seed_hi}, e->n_sigma, e->n_season,
                                                          e->n_cells, e->nx, e->ny, (long long)step, dev.get(), e->stream));
  HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream));
  HIP_STEP(e, who, "hipMemcpy", hipMemcpy(out, dev.get(), (size_t)e->np * sizeof(float), hipMemcpyDeviceToHost));
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
  DevBuf<float> owned[kBoundaryFields], frec; // what the set allocates, its until the set is the engine's
  DevBuf<char> new_table; // kSetTableBytes: the entries and the record pointers behind them
  auto put = [&](int field, const float* host) -> int { // the set's own copy of one field
    HIP_STEP(e, who, "hipMalloc", owned[field].alloc(boundary_floats(field, np)));
    b.dev[field] = owned[field].get(); b.own[field] = true;
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(b.dev[field], host, boundary_floats(field, np) * sizeof(float), hipMemcpyHostToDevice));
    return 0;
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
    HIP_STEP(e, who, "hipMalloc", new_table.alloc(kSetTableBytes));
    table = reinterpret_cast<BoundarySet*>(new_table.get());
    const BoundarySet own = set_entry(e->bound[0]);
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(table, &own, sizeof(own), hipMemcpyHostToDevice));
  }
  const BoundarySet mine = set_entry(b);
  HIP_STEP(e, who, "hipMemcpy", hipMemcpy(table + e->bound.size(), &mine, sizeof(mine), hipMemcpyHostToDevice));
  if (uses_forcing_records(e)) { // (the last step that can fail: a record that fails leaves nothing behind)
    const char* what = "";
    HIP_STEP(e, who, what, make_forcing_record(e, b, table, e->bound.size(), frec, &what));
  }
  // complete: the engine takes the table, the set and what the set owns
  if (new_table) e->bsets_dev = reinterpret_cast<BoundarySet*>(new_table.release());
  for (auto& o : owned) (void)o.release();
  b.frec = frec.release();
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
  DevBuf<int> bset_dev;
  DevBuf<MemberForcing> neutral;
  DevBuf<float> state;
  if (on_sets > 0) {
    HIP_STEP(e, who, "hipMalloc", bset_dev.alloc(nm));
    HIP_STEP(e, who, "hipMemcpy", hipMemcpy(bset_dev.get(), bs.data(), nm * sizeof(int), hipMemcpyHostToDevice));
    if (!e->neutral_force_dev) {
      const std::vector<MemberForcing> w(nm, MemberForcing{-1, 1.f, -1, 1.f});
      HIP_STEP(e, who, "hipMalloc", neutral.alloc(nm));
      HIP_STEP(e, who, "hipMemcpy", hipMemcpy(neutral.get(), w.data(), nm * sizeof(MemberForcing), hipMemcpyHostToDevice));
    }
  }
  if (flags & GREB_BS_REINIT) { // every member's state: the initial state of its set (:190-197) under its own physics
    std::vector<float> st(5 * np);
    HIP_STEP(e, who, "hipMalloc of the members' states", state.alloc(nm * 5 * np));
    for (size_t m = 0; m < nm; ++m) {
      initial_state(e->bound[(size_t)bs[m]], e->h_phys[m], np, st.data());
      HIP_STEP(e, who, "hipMemcpy", hipMemcpy(state.get() + m * 5 * np, st.data(), 5 * np * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  HIP_STEP(e, who, "hipStreamSynchronize", hipStreamSynchronize(e->stream)); // nothing in flight reads what is replaced
  // members whose sets differ need a correction set each (the last step that can fail)
  if (!uniform && e->shared_corr && nm > 1) if (int rc = own_corrections(e, who)) return rc;
  if (state) adopt(e->state, state);
  if (neutral) adopt(e->neutral_force_dev, neutral);
  if (bset_dev) adopt(e->bset_dev, bset_dev);
  if (set) e->h_bset = bs; else e->h_bset.clear();
  e->members_on_sets = on_sets;
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


} // extern "C"
