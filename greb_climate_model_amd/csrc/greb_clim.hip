// greb_clim.hip -- climatology output (include/greb_engine.h: greb_clim_*): the reduction along the TIME axis.
//
// The reference leaves multi-year means, seasonal maps and the difference to a control run to R scripts over the output
// files of separate processes.  Here an ensemble's model year sits in HBM as [member][12][n_vars][ny][nx] -- one staging slot
// of greb_engine_run -- with the control member beside the others, so:
//
//   clim_add_year_kernel  adds one model year into per-element fp64 sums S (and, for the trend, T = sum of k x with k the
//                         0-based year of the period), in ascending year order.  A lane owns kClimGroups groups of four
//                         consecutive elements, a block's groups interleaved so that every access of a wavefront is one
//                         contiguous KiB: per group one 16-byte non-temporal load of the record (the slot is not read
//                         again) and two 16-byte loads and stores of each of S and T, all loads of the lane's groups
//                         issued before the first add.  The year k = 0 STORES S = x, T = 0: no clearing pass, and the
//                         8 bytes per element of reading sums that are about to be overwritten are saved.
//   clim_finish_kernel    a lane owns four points of one (member, variable) across the twelve months: mean = S / n,
//                         the day-weighted seasonal means of those, the least-squares slope from S and T, and -- with
//                         the control's means recomputed from the control's sums, not stored -- the responses.
//
// No LDS, no atomics, one owner per element: results are deterministic and do not depend on the batch.  Everything is
// fp64 and rounded to fp32 once.  THE ORDER OF OPERATIONS IS THE DEFINITION of the results (clim.reference in Python
// performs the same IEEE operations): this file is built with -ffp-contract=off (build.py: EXTRA_FLAGS), so that no
// multiply is fused into the add that follows it.
#include "greb_clim.h"

namespace greb {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

template <bool TREND, bool FIRST, bool FULL>
__device__ inline void add_year_body(const f4* __restrict__ x, d2* __restrict__ S, d2* __restrict__ T, size_t n4, size_t g0,
                                     double k) {
  f4 v[kClimGroups];
  d2 sa[kClimGroups], sb[kClimGroups], ta[kClimGroups], tb[kClimGroups];
#pragma unroll
  for (int u = 0; u < kClimGroups; ++u) {
    const size_t g = g0 + (size_t)u * kClimThreads;
    if (FULL || g < n4) v[u] = __builtin_nontemporal_load(x + g);
  }
  if (!FIRST) {
#pragma unroll
    for (int u = 0; u < kClimGroups; ++u) {
      const size_t g = g0 + (size_t)u * kClimThreads;
      if (FULL || g < n4) {
        sa[u] = S[2 * g]; sb[u] = S[2 * g + 1];
        if (TREND) { ta[u] = T[2 * g]; tb[u] = T[2 * g + 1]; }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kClimGroups; ++u) {
    const size_t g = g0 + (size_t)u * kClimThreads;
    if (!(FULL || g < n4)) continue;
    const d2 xa = {(double)v[u].x, (double)v[u].y}, xb = {(double)v[u].z, (double)v[u].w};
    if (FIRST) {
      S[2 * g] = xa; S[2 * g + 1] = xb;
      if (TREND) { const d2 z = {0.0, 0.0}; T[2 * g] = z; T[2 * g + 1] = z; }
    } else {
      S[2 * g] = sa[u] + xa; S[2 * g + 1] = sb[u] + xb;
      if (TREND) { T[2 * g] = ta[u] + k * xa; T[2 * g + 1] = tb[u] + k * xb; } // k x is exact in fp64 (k < 2^29)
    }
  }
}

template <bool TREND, bool FIRST>
__global__ __launch_bounds__(kClimThreads) void clim_add_year_kernel(const float* __restrict__ x, double* __restrict__ S,
                                                                      double* __restrict__ T, size_t n4, double k) {
  const size_t b0 = (size_t)blockIdx.x * (kClimThreads * kClimGroups); // the block's first group of four elements
  const f4* x4 = reinterpret_cast<const f4*>(x);
  d2 *S2 = reinterpret_cast<d2*>(S), *T2 = reinterpret_cast<d2*>(T);
  if (b0 + (size_t)kClimThreads * kClimGroups <= n4) add_year_body<TREND, FIRST, true>(x4, S2, T2, n4, b0 + threadIdx.x, k);
  else add_year_body<TREND, FIRST, false>(x4, S2, T2, n4, b0 + threadIdx.x, k); // (the last block: groups past n4 are skipped)
}

struct Q { double v[4]; }; // a lane's four points

__device__ inline Q load4(const double* p) {
  const d2 a = reinterpret_cast<const d2*>(p)[0], b = reinterpret_cast<const d2*>(p)[1];
  return Q{{a.x, a.y, b.x, b.y}};
}
__device__ inline void store4(float* p, const Q& q) {
  const f4 o = {(float)q.v[0], (float)q.v[1], (float)q.v[2], (float)q.v[3]};
  *reinterpret_cast<f4*>(p) = o;
}
__device__ inline void store4(float* p, float c) {
  const f4 o = {c, c, c, c};
  *reinterpret_cast<f4*>(p) = o;
}

// season s of the twelve monthly means: acc = 0; acc = acc + days[mo] * mean[mo] over the season's months in calendar
// order (DJF: Dec, Jan, Feb of the same years); acc / the season's days
__device__ inline void seasons_of(const Q (&mean)[kClimMonths], Q (&out)[kClimSeasons]) {
  constexpr double days[kClimMonths] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31}; // JDAY_MON, src/greb.f90:42
  constexpr int first[kClimSeasons] = {11, 2, 5, 8, 0}, count[kClimSeasons] = {3, 3, 3, 3, 12};
  constexpr double total[kClimSeasons] = {90, 92, 92, 91, 365};
#pragma unroll
  for (int s = 0; s < kClimSeasons; ++s) {
    Q acc = {{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int j = 0; j < count[s]; ++j) {
      const int mo = (first[s] + j) % kClimMonths;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc.v[e] = acc.v[e] + days[mo] * mean[mo].v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) out[s].v[e] = acc.v[e] / total[s];
  }
}

__global__ __launch_bounds__(kClimThreads) void clim_finish_kernel(ClimFinishArgs a, size_t lanes, double n, double kbar,
                                                                   double sxx) {
  const size_t i = (size_t)blockIdx.x * kClimThreads + threadIdx.x; // [member][variable][group of four points]
  if (i >= lanes) return;
  const size_t gp = a.np >> 2, nv = (size_t)a.nv;
  const size_t member = i / (nv * gp), var = (i / gp) % nv, p = 4 * (i % gp);
  const size_t rec = a.np * nv; // one month of one member
  const size_t at_mon = (member * kClimMonths * nv + var) * a.np + p;   // month mo: + mo * rec
  const size_t at_sea = (member * kClimSeasons * nv + var) * a.np + p;  // season s: + s * rec
  Q mean[kClimMonths], sea[kClimSeasons];
#pragma unroll
  for (int mo = 0; mo < kClimMonths; ++mo) {
    const Q s = load4(a.S + at_mon + mo * rec);
    if (a.trend) {
      Q t = {{0.0, 0.0, 0.0, 0.0}}; // one year has no slope
      if (a.n_years > 1) {
        const Q tt = load4(a.T + at_mon + mo * rec);
#pragma unroll
        for (int e = 0; e < 4; ++e) t.v[e] = (tt.v[e] - kbar * s.v[e]) / sxx;
      }
      store4(a.trend + at_mon + mo * rec, t);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) mean[mo].v[e] = s.v[e] / n;
    if (a.mean) store4(a.mean + at_mon + mo * rec, mean[mo]);
  }
  const bool want_seasons = a.seasons || a.seasons_resp;
  if (want_seasons) seasons_of(mean, sea);
  if (a.seasons) {
#pragma unroll
    for (int s = 0; s < kClimSeasons; ++s) store4(a.seasons + at_sea + s * rec, sea[s]);
  }
  if (!a.mean_resp && !a.seasons_resp) return;
  const int c = a.control[member];
  if (c < 0) { // no control: a quiet NaN -- zero would read as "no response"
    const float nan = __builtin_nanf("");
    if (a.mean_resp)
      for (int mo = 0; mo < kClimMonths; ++mo) store4(a.mean_resp + at_mon + mo * rec, nan);
    if (a.seasons_resp)
      for (int s = 0; s < kClimSeasons; ++s) store4(a.seasons_resp + at_sea + s * rec, nan);
    return;
  }
  const size_t ctl_mon = ((size_t)c * kClimMonths * nv + var) * a.np + p;
  Q cmean[kClimMonths];
#pragma unroll
  for (int mo = 0; mo < kClimMonths; ++mo) { // the control's means again from its sums: the same operations, the same bits
    const Q s = load4(a.S + ctl_mon + mo * rec);
#pragma unroll
    for (int e = 0; e < 4; ++e) cmean[mo].v[e] = s.v[e] / n;
    if (a.mean_resp) {
      Q r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r.v[e] = mean[mo].v[e] - cmean[mo].v[e];
      store4(a.mean_resp + at_mon + mo * rec, r);
    }
  }
  if (a.seasons_resp) {
    Q csea[kClimSeasons];
    seasons_of(cmean, csea);
#pragma unroll
    for (int s = 0; s < kClimSeasons; ++s) {
      Q r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r.v[e] = sea[s].v[e] - csea[s].v[e];
      store4(a.seasons_resp + at_sea + s * rec, r);
    }
  }
}

} // namespace

hipError_t launch_clim_add_year(const float* x, double* S, double* T, size_t n, int k, hipStream_t s) {
  const size_t n4 = n >> 2, per_block = (size_t)kClimThreads * kClimGroups;
  const dim3 grid((unsigned)((n4 + per_block - 1) / per_block)), block(kClimThreads);
  if (n4 == 0) return hipSuccess;
  const double kd = (double)k;
  if (T) {
    if (k == 0) hipLaunchKernelGGL((clim_add_year_kernel<true, true>), grid, block, 0, s, x, S, T, n4, kd);
    else hipLaunchKernelGGL((clim_add_year_kernel<true, false>), grid, block, 0, s, x, S, T, n4, kd);
  } else {
    if (k == 0) hipLaunchKernelGGL((clim_add_year_kernel<false, true>), grid, block, 0, s, x, S, T, n4, kd);
    else hipLaunchKernelGGL((clim_add_year_kernel<false, false>), grid, block, 0, s, x, S, T, n4, kd);
  }
  return hipGetLastError();
}

hipError_t launch_clim_finish(const ClimFinishArgs& a, int n_members, hipStream_t s) {
  const size_t lanes = (size_t)n_members * a.nv * (a.np >> 2);
  if (lanes == 0) return hipSuccess;
  const double n = (double)a.n_years;
  const double kbar = (n - 1.0) / 2.0, sxx = n * (n * n - 1.0) / 12.0; // mean and sum of squares about it of 0 ... n-1 (exact)
  hipLaunchKernelGGL(clim_finish_kernel, dim3((unsigned)((lanes + kClimThreads - 1) / kClimThreads)), dim3(kClimThreads), 0, s, a,
                     lanes, n, kbar, sxx);
  return hipGetLastError();
}

} // namespace greb
