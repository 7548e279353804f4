// greb_clim.h -- host interface of the climatology output (greb_clim.hip): model years of monthly records summed along
// the time axis, and the sums of a period turned into multi-year means, seasonal means, trends and responses.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace greb {

constexpr int kClimThreads = 256;
constexpr int kClimGroups = 4;  // independent groups of four elements one lane of clim_add_year_kernel keeps in flight
constexpr int kClimMonths = 12;
constexpr int kClimSeasons = 5; // DJF MAM JJA SON ANN

// Year `k` (0-based inside its period) of monthly records x[n] (n % 4 == 0, 16-byte aligned: [n_members][12][n_vars][ny][nx])
// into the fp64 sums: S = S + x and, with T, T = T + k x; the year k = 0 stores S = x, T = 0 instead.
hipError_t launch_clim_add_year(const float* x, double* S, double* T /* or null */, size_t n, int k, hipStream_t s);

struct ClimFinishArgs {
  const double* S;      // [n_members][12][5][np]
  const double* T;      // the same, or null (no trend)
  const int* control;   // [n_members] on the device: each member's control member, -1 = none; null = no responses
  size_t np;            // nx * ny, a multiple of four
  int nv;               // variables per month (the plan's n_vars); [5] below stands for it, [5][5] for [5 seasons][nv]
  int n_years;          // years summed
  float* mean;          // [n_members][12][5][np]; null = skipped (all outputs 16-byte aligned)
  float* seasons;       // [n_members][5][5][np]; null = skipped
  float* trend;         // [n_members][12][5][np]; null = skipped
  float* mean_resp;     // [n_members][12][5][np]: member minus its control (a quiet NaN where it has none); null = skipped
  float* seasons_resp;  // [n_members][5][5][np]; null = skipped
};

hipError_t launch_clim_finish(const ClimFinishArgs& a, int n_members, hipStream_t s);

} // namespace greb
