// greb_fluxes.h -- host interface of the combination stage of the budget terms (greb_fluxes.hip): a model year of budget
// records turned into linear combinations of its thirteen terms, record by record.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace greb {

constexpr int kFluxThreads = 256;
constexpr int kFluxTerms = 13;   // GREB_NBUDGET
constexpr int kFluxMaxOut = 16;  // GREB_MAX_RECORD_VARS

// The coefficients, by value in the kernel arguments (at most 16 x 13 words).
struct FluxCombo {
  float c[kFluxMaxOut][kFluxTerms]; // rows behind n_out are not read
  int n_out;
  unsigned used;                    // bit j: some row has a non-zero coefficient of term j
};

// in [n_members][12][13][np] -> out [n_members][12][n_out][np]; np % 4 == 0, both 16-byte aligned
hipError_t launch_budget_combine(const FluxCombo& c, const float* in, int n_members, size_t np, float* out, hipStream_t s);

} // namespace greb
