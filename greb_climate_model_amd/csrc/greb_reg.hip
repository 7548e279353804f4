// greb_reg.hip -- regression output (include/greb_engine.h: greb_reg_*): each member's records per unit of its OWN index.
//
// greb_clim.hip's TREND regresses on the year number, which is known before the run.  Here the regressor g is a scalar
// the run itself produces -- a regional mean of the same member's year, e.g. its annual global-mean warming -- so the
// product sum over the years of g * y is not a function of any sums another plan keeps.  A model year sits in HBM as
// [member][12][n_vars][ny][nx] -- one staging slot of greb_engine_run --; launch_diag_year (greb_diag.hip) has reduced it
// to the regional means [member][12][n_vars][nr], and then
//
//   reg_index_kernel     one thread per (member, index): g from the regional means (a month, or the season formula of
//                        greb_season.h over the twelve means; `rel`: ONE fp32 subtraction of the control's), year 0 STORES
//                        g0 and zero sums, later years add G = (double)g - (double)g0 and G * G; G is left for the update
//                        kernel and g is the year's INDEX.
//   reg_update_kernel    grid (blocks of 256 point quads, member, distinct variable of the terms): year_walk of
//                        greb_yearwalk.h, as cross_update_kernel.  Every term adds Y = (double)y - (double)y0, G * Y and
//                        Y * Y to its sums [member][term][np], one array per word.  G is wave-uniform and comes by a scalar
//                        load.  Year k = 0 STORES y0 and zero sums: no clearing pass.
//   reg_finish_kernel    grid (blocks of point quads, member, term): the sums -> slope, intercept, R2.
//
// One owner per element, no atomics, no LDS: results are deterministic and a member's numbers do not depend on the batch
// it is in.  THE ORDER OF OPERATIONS IS THE DEFINITION (regress.reference in Python performs the same IEEE operations):
// this file is built with -ffp-contract=off (build.py: EXTRA_FLAGS), so that no multiply is fused into the add behind it.
#include "greb_reg.h"

namespace greb {
namespace {

using season::f4;
using season::kMonths;
using season::series_quantity;
typedef double d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kRegThreads) void reg_index_kernel(RegIndexArgs a) {
  const int i = (int)(blockIdx.x * kRegThreads + threadIdx.x);
  if (i >= a.n_members * a.n_indices) return;
  const int m = i / a.n_indices, j = i - m * a.n_indices;
  const RegIndexTable::Ix ix = a.t.ix[j];
  const size_t stride = (size_t)a.n_vars * a.nr, member = (size_t)kMonths * stride, at = (size_t)ix.var * a.nr + ix.region;
  float g = series_quantity(a.regions + (size_t)m * member + at, stride, ix.sel);
  if (ix.rel) {
    const int c = a.control ? a.control[m] : -1;
    if (c >= 0) g = g - series_quantity(a.regions + (size_t)c * member + at, stride, ix.sel); // ONE fp32 subtraction
    else g = __builtin_nanf("");
  }
  if (a.k == 0) {
    a.ix.g0[i] = g; a.ix.G[i] = 0.0; a.ix.sg[i] = 0.0; a.ix.sgg[i] = 0.0;
  } else {
    const double G = (double)g - (double)a.ix.g0[i];
    const double GG = G * G;
    a.ix.G[i] = G;
    a.ix.sg[i] = a.ix.sg[i] + G;
    a.ix.sgg[i] = a.ix.sgg[i] + GG;
  }
  if (a.index) a.index[(size_t)m * a.index_stride + j] = g;
}

// one term's state words of one quad: g = the quad's index in [member][term][np / 4]
template <bool FIRST>
__device__ inline void update_term(const RegState& st, size_t g, const f4 y, double G) {
  f4* p0 = reinterpret_cast<f4*>(st.y0) + g;
  d4* ps = reinterpret_cast<d4*>(st.sy) + g;
  d4* pg = reinterpret_cast<d4*>(st.sgy) + g;
  d4* pq = st.syy ? reinterpret_cast<d4*>(st.syy) + g : nullptr;
  if (FIRST) {
    const d4 z = {0.0, 0.0, 0.0, 0.0};
    *p0 = y; *ps = z; *pg = z;
    if (pq) *pq = z;
    return;
  }
  const f4 y0 = *p0;
  d4 sy = *ps, sgy = *pg, Y;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    Y[e] = (double)y[e] - (double)y0[e];
    const double gy = G * Y[e];
    sy[e] = sy[e] + Y[e];
    sgy[e] = sgy[e] + gy;
  }
  *ps = sy; *pg = sgy;
  if (pq) {
    d4 syy = *pq;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double yy = Y[e] * Y[e];
      syy[e] = syy[e] + yy;
    }
    *pq = syy;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(kRegThreads) void reg_update_kernel(RegUpdateArgs a) {
  const double* G = a.G + (size_t)(int)blockIdx.y * a.n_indices; // the member's (wave-uniform)
  year_walk<kRegThreads>(a.t, a.x, a.control, a.np, a.n_vars, a.n_terms, [st = a.st, G](const RegTerm& t, size_t g, const f4 q) {
    update_term<FIRST>(st, g, q, FIRST ? 0.0 : G[t.index]);
  });
}

__global__ __launch_bounds__(kRegThreads) void reg_finish_kernel(RegFinishArgs a) {
  const size_t gp = a.np >> 2, quad = (size_t)blockIdx.x * kRegThreads + threadIdx.x;
  if (quad >= gp) return;
  const int m = (int)blockIdx.y, t = (int)blockIdx.z;
  const size_t g = ((size_t)m * a.n_terms + t) * gp + quad;
  const size_t ig = (size_t)m * a.n_indices + a.index_of[t]; // (wave-uniform)
  const double n = (double)a.n_years, Sg = a.ix.sg[ig], Sgg = a.ix.sgg[ig], g0 = (double)a.ix.g0[ig];
  // every step a separate fp64 operation
  double tmp = Sg * Sg;
  tmp = tmp / n;
  const double Sxx = Sgg - tmp;
  tmp = Sg / n;
  const double gbar = g0 + tmp;
  const bool ok = a.n_years >= 2 && Sxx > 0.0; // (a NaN is not > 0)
  const f4 y0 = reinterpret_cast<const f4*>(a.st.y0)[g];
  const d4 Sy = reinterpret_cast<const d4*>(a.st.sy)[g], Sgy = reinterpret_cast<const d4*>(a.st.sgy)[g];
  d4 Syy = {0.0, 0.0, 0.0, 0.0};
  if (a.r2) Syy = reinterpret_cast<const d4*>(a.st.syy)[g];
  const float nan = __builtin_nanf("");
  f4 slope, icpt, r2;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double u = Sg * Sy[e];
    u = u / n;
    const double Sxy = Sgy[e] - u;
    const double b = Sxy / Sxx;
    slope[e] = ok ? (float)b : nan;
    u = Sy[e] / n;
    const double ybar = (double)y0[e] + u;
    u = b * gbar;
    icpt[e] = ok ? (float)(ybar - u) : nan;
    u = Sy[e] * Sy[e];
    u = u / n;
    const double Syc = Syy[e] - u;
    const double num = Sxy * Sxy, den = Sxx * Syc;
    r2[e] = ok && Syc > 0.0 ? (float)(num / den) : nan;
  }
  if (a.slope) reinterpret_cast<f4*>(a.slope)[g] = slope;
  if (a.intercept) reinterpret_cast<f4*>(a.intercept)[g] = icpt;
  if (a.r2) reinterpret_cast<f4*>(a.r2)[g] = r2;
}

} // namespace

hipError_t launch_reg_index(const RegIndexArgs& a, hipStream_t s) {
  if (!a.regions || !a.ix.g0 || !a.ix.G || !a.ix.sg || !a.ix.sgg || a.n_members < 1 || a.n_vars < 1 || a.nr < 1 || a.n_indices < 1 ||
      a.n_indices > kRegMaxIndices || a.k < 0 || (a.index && a.index_stride < (size_t)a.n_indices))
    return hipErrorInvalidValue;
  for (int j = 0; j < a.n_indices; ++j) { // what the kernel indexes with: nothing may point outside the regional means
    const RegIndexTable::Ix& ix = a.t.ix[j];
    if (ix.var < 0 || ix.var >= a.n_vars || ix.sel < 0 || ix.sel >= season::kSelectors || ix.region < 0 || ix.region >= a.nr || (ix.rel && !a.control))
      return hipErrorInvalidValue;
  }
  const size_t total = (size_t)a.n_members * a.n_indices;
  hipLaunchKernelGGL(reg_index_kernel, dim3((unsigned)((total + kRegThreads - 1) / kRegThreads)), dim3(kRegThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_reg_update(const RegUpdateArgs& a, hipStream_t s) {
  const RegTable& t = a.t;
  if (!a.x || !a.G || !a.st.y0 || !a.st.sy || !a.st.sgy || a.np < 4 || (a.np & 3) || a.n_members < 1 || a.n_members > kRegMaxMembers ||
      a.n_vars < 1 || a.n_terms < 1 || a.n_terms > kRegMaxTerms || a.n_indices < 1 || a.n_indices > kRegMaxIndices || a.k < 0 ||
      !year_table_ok(t, a.n_vars, a.n_terms, a.control != nullptr))
    return hipErrorInvalidValue;
  for (int i = 0; i < a.n_terms; ++i) // (the G the kernel reads)
    if (t.item[i].index < 0 || t.item[i].index >= a.n_indices) return hipErrorInvalidValue;
  const size_t gp = a.np >> 2;
  const dim3 grid((unsigned)((gp + kRegThreads - 1) / kRegThreads), (unsigned)a.n_members, (unsigned)t.n_vars_used);
  if (a.k == 0) hipLaunchKernelGGL(reg_update_kernel<true>, grid, dim3(kRegThreads), 0, s, a);
  else hipLaunchKernelGGL(reg_update_kernel<false>, grid, dim3(kRegThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_reg_finish(const RegFinishArgs& a, hipStream_t s) {
  if (!a.st.y0 || !a.st.sy || !a.st.sgy || (a.r2 && !a.st.syy) || !a.ix.g0 || !a.ix.sg || !a.ix.sgg || a.np < 4 || (a.np & 3) ||
      a.n_members < 1 || a.n_members > kRegMaxMembers || a.n_terms < 1 || a.n_terms > kRegMaxTerms || a.n_indices < 1 ||
      a.n_indices > kRegMaxIndices || a.n_years < 1)
    return hipErrorInvalidValue;
  for (int t = 0; t < a.n_terms; ++t)
    if (a.index_of[t] < 0 || a.index_of[t] >= a.n_indices) return hipErrorInvalidValue;
  if (!a.slope && !a.intercept && !a.r2) return hipSuccess;
  const size_t gp = a.np >> 2;
  const dim3 grid((unsigned)((gp + kRegThreads - 1) / kRegThreads), (unsigned)a.n_members, (unsigned)a.n_terms);
  hipLaunchKernelGGL(reg_finish_kernel, grid, dim3(kRegThreads), 0, s, a);
  return hipGetLastError();
}

} // namespace greb
