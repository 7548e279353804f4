// greb_diag.h -- host interface of the on-device diagnostics (greb_diag.hip): one model year of monthly records reduced
// to regional means, zonal means and the annual-mean map.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace greb {

constexpr int kDiagMaxRegions = 15; // caller-supplied regions; the globe is region 0 on top of them
constexpr int kDiagThreads = 256;   // one workgroup: a band of at most 256 groups of four longitudes
constexpr int kDiagMonths = 12;

// rows of one workgroup's band on a grid `nx` wide, and the bands of `ny` rows
inline int diag_band_rows(int nx) { const int r = kDiagThreads / (nx / 4); return r < 1 ? 1 : r; }
inline int diag_bands(int nx, int ny) { const int r = diag_band_rows(nx); return (ny + r - 1) / r; }
// doubles of scratch one batch of `n_members` needs for the per-band partial sums of `nr` regions (globe included) of
// `nv` variables
inline size_t diag_partials(int nx, int ny, int n_members, int nr, int nv) {
  return (size_t)n_members * nv * diag_bands(nx, ny) * kDiagMonths * nr;
}

struct DiagArgs {
  const float* monthly;    // [n_members][12][nv][ny][nx], 16-byte aligned
  int nx, ny, nr, nv;      // nr = 1 + n_regions; nv variables per month (the plan's n_vars)
  const double* w;         // [nr][ny][nx] combined weights w_r * cos(lat_j)
  const double* inv_sum;   // [nr] 1 / sum of the combined weights
  double* partials;        // diag_partials() doubles (regions only)
  float* regions;          // member m at regions + m * regions_stride: [12][nv][nr]; null = skipped
  size_t regions_stride;   // floats between two members' region records
  float* zonal;            // [n_members][12][nv][ny]; null = skipped
  float* annual;           // [n_members][nv][ny][nx], 16-byte aligned; null = skipped
};

hipError_t launch_diag_year(const DiagArgs& a, int n_members, hipStream_t s);

} // namespace greb
