// greb_fluxes.hip -- the combination stage of the budget terms (include/greb_engine.h: greb_budget_combine_dev).
//
// What is wanted of the thirteen flux terms of a budget run are mostly sums of them: the surface net flux, the
// atmospheric net flux, evaporation plus rain -- the right-hand sides of src/greb.f90:258, :260 and :263.  For every
// product that is not linear in its input (a variance, a minimum, a quantile, a residual) the sum has to be formed
// BEFORE the reduction, so it is formed here, while the year's budget records [member][12][13][ny][nx] still sit in HBM,
// into [member][12][n_out][ny][nx] -- the layout the diag, clim, ens and lin kernels read.
//
//   budget_combine_kernel  one streaming pass.  A lane owns four consecutive points of one (member, month): it loads
//                          each term that any output uses once (16-byte loads, all issued before the first multiply)
//                          and stores each output once (16-byte stores).  The coefficients travel by value in the
//                          kernel arguments and are read through the scalar cache.
//
// Per element and output k, over the terms j in ascending order, skipping those with combo[k][j] == 0: the first term
// used gives acc = c * b, every later one acc = acc + c * b -- an fp32 multiply, then an fp32 add.  THE ORDER OF
// OPERATIONS IS THE DEFINITION of the results (budget.combine_reference in Python performs the same IEEE operations):
// this file is built with -ffp-contract=off (build.py: EXTRA_FLAGS), so that no multiply is fused into the add behind
// it.  A row with a single coefficient 1 therefore copies the term's bits, -0.0 included.
#include "greb_fluxes.h"

namespace greb {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kFluxThreads) void budget_combine_kernel(FluxCombo c, const float* __restrict__ in,
                                                                      float* __restrict__ out, size_t np, size_t lanes) {
  const size_t i = (size_t)blockIdx.x * kFluxThreads + threadIdx.x; // [member][month][group of four points]
  if (i >= lanes) return;
  const size_t gp = np >> 2;
  const size_t mm = i / gp, p = 4 * (i % gp); // mm = member * 12 + month
  const float* src = in + mm * kFluxTerms * np + p;
  f4 b[kFluxTerms];
#pragma unroll
  for (int j = 0; j < kFluxTerms; ++j) {
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    b[j] = (c.used >> j) & 1u ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(src + (size_t)j * np)) : zero;
  }
  float* dst = out + mm * (size_t)c.n_out * np + p;
  for (int k = 0; k < c.n_out; ++k) {
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    bool first = true;
#pragma unroll
    for (int j = 0; j < kFluxTerms; ++j) {
      const float cj = c.c[k][j];
      if (cj == 0.f) continue;
      const f4 t = cj * b[j];
      acc = first ? t : acc + t;
      first = false;
    }
    *reinterpret_cast<f4*>(dst + (size_t)k * np) = acc;
  }
}

} // namespace

hipError_t launch_budget_combine(const FluxCombo& c, const float* in, int n_members, size_t np, float* out, hipStream_t s) {
  const size_t lanes = (size_t)n_members * 12 * (np >> 2);
  if (lanes == 0) return hipSuccess;
  hipLaunchKernelGGL(budget_combine_kernel, dim3((unsigned)((lanes + kFluxThreads - 1) / kFluxThreads)), dim3(kFluxThreads), 0, s, c,
                     in, out, np, lanes);
  return hipGetLastError();
}

} // namespace greb
