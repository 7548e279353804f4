// greb_lin.h -- host interface of the linear-model output (greb_lin.hip): K linear contrasts along the member axis of each
// element of x[n_members][n], and the residual sum of squares of the fit they are the coefficients of.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace greb {

constexpr int kLinThreads = 256;
constexpr int kLinMaxTerms = 64;
constexpr int kLinChunk = 16; // terms one lane of lin_coef_kernel accumulates: 16 terms x 2 elements = 32 fp64 accumulators
constexpr int kLinRows = 8;   // member rows one lane of lin_coef_kernel keeps in flight (4 with a control map, beside their 4 controls)
constexpr int kLinFit = 4;    // members whose fitted values one lane of lin_rss_kernel forms side by side

// The plan's tables on the device.  The used members in ascending member index: member[k], control[k] beside it (null: no
// control map), and per used member a row of `stride` = 16 * chunks doubles -- its weights [term], zero behind term K - 1
// (a zero weight adds +0.0 to a sum that started from +0.0 and is never stored) -- so a member's weights are consecutive.
struct LinTables {
  const int* member;     // [n_used]
  const int* control;    // [n_used] or null
  const double* weight;  // [n_used][stride]
  const double* design;  // [n_used][stride] or null (no GREB_L_RSS)
  int n_used, n_terms, stride;
};

// coef[K][n]: grid (ceil(ceil(n / 2) / 256), ceil(K / 16)); every used member's row is read once per chunk of 16 terms
hipError_t launch_lin_coef(const float* x, size_t n, const LinTables& t, float* coef, hipStream_t s);
// rss[n]: grid ceil(n / 256); every used member's row is read twice.  Needs t.design.
hipError_t launch_lin_rss(const float* x, size_t n, const LinTables& t, float* rss, hipStream_t s);

} // namespace greb
