// greb_cross.hip -- crossing output (include/greb_engine.h: greb_cross_*): the NON-LINEAR reduction along the time axis.
//
// greb_clim.hip sums the years; a threshold is not linear in the record, so "in which year does a member's annual-mean
// warming pass 2 K, and does it stay there" cannot be made from its sums.  Here a model year sits in HBM as
// [member][12][n_vars][ny][nx] -- one staging slot of greb_engine_run -- and per (member, event, point) a few state words
// follow the years: the first and the last year that hit, the last year that missed, the number of hits, the peak and
// its year.
//
//   cross_update_kernel    grid (blocks of 256 point quads, member, distinct variable of the events): year_walk of
//                          greb_yearwalk.h, which loads the months the variable's events need once and forms each
//                          selector's quantity once.  Every event updates its state words [member][event][np] with 16-byte
//                          loads and stores, a wavefront's access being one contiguous KiB.  Year k = 0 STORES the state:
//                          no clearing pass.  With FRACTION it also writes the year's hit bytes [member][event][np].
//   cross_fraction_kernel  grid (blocks of point quads, group, event).  Adds the group's hit bytes in ascending member
//                          index, four points per 32-bit load, and stores (float)((double)c / (double)n_g).
//   cross_finish_kernel    the state words -> the selected maps; STAY = last_miss + 1 where that is a year of the period.
//
// One owner per element, no atomics, no LDS: results are deterministic and a member's numbers do not depend on the
// batch it is in.  THE ORDER OF OPERATIONS IS THE DEFINITION of the season quantity (cross.reference in Python performs
// the same IEEE operations; it is seasons_of of greb_clim.hip applied to one year): this file is built with
// -ffp-contract=off (build.py: EXTRA_FLAGS), so that no multiply is fused into the add that follows it.
#include "greb_cross.h"

namespace greb {
namespace {

using season::f4;
typedef int i4 __attribute__((ext_vector_type(4)));

// one event's state words of one quad: g = the quad's index in [member][event][np / 4]
template <bool FIRST>
__device__ inline void update_event(const CrossState& st, size_t g, const f4 q, int dir, float thr, int k) {
  i4 hit;
#pragma unroll
  for (int e = 0; e < 4; ++e) hit[e] = dir > 0 ? q[e] >= thr : q[e] <= thr; // (a NaN never hits)
  if (st.first) {
    i4* p = reinterpret_cast<i4*>(st.first) + g;
    i4 v;
    if (!FIRST) v = *p;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = FIRST ? (hit[e] ? 0 : -1) : (v[e] < 0 && hit[e] ? k : v[e]);
    *p = v;
  }
  if (st.last) {
    i4* p = reinterpret_cast<i4*>(st.last) + g;
    i4 v;
    if (!FIRST) v = *p;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = hit[e] ? k : (FIRST ? -1 : v[e]);
    *p = v;
  }
  if (st.last_miss) {
    i4* p = reinterpret_cast<i4*>(st.last_miss) + g;
    i4 v;
    if (!FIRST) v = *p;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = hit[e] ? (FIRST ? -1 : v[e]) : k;
    *p = v;
  }
  if (st.count) {
    i4* p = reinterpret_cast<i4*>(st.count) + g;
    i4 v = {0, 0, 0, 0};
    if (!FIRST) v = *p;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] + (hit[e] ? 1 : 0);
    *p = v;
  }
  if (st.peak) {
    f4* pp = reinterpret_cast<f4*>(st.peak) + g;
    i4* py = reinterpret_cast<i4*>(st.peak_year) + g;
    if (FIRST) {
      const i4 z = {0, 0, 0, 0};
      *pp = q; *py = z;
    } else {
      f4 v = *pp;
      i4 y = *py;
#pragma unroll
      for (int e = 0; e < 4; ++e) { // strict: a tie keeps the earlier year; a NaN peak gives way to a number
        const bool take = (dir > 0 ? q[e] > v[e] : q[e] < v[e]) || (v[e] != v[e] && q[e] == q[e]);
        v[e] = take ? q[e] : v[e];
        y[e] = take ? k : y[e];
      }
      *pp = v; *py = y;
    }
  }
  if (st.hit)
    reinterpret_cast<unsigned*>(st.hit)[g] = (hit[0] ? 1u : 0u) | (hit[1] ? 1u << 8 : 0u) | (hit[2] ? 1u << 16 : 0u) | (hit[3] ? 1u << 24 : 0u);
}

template <bool FIRST>
__global__ __launch_bounds__(kCrossThreads) void cross_update_kernel(CrossUpdateArgs a) {
  year_walk<kCrossThreads>(a.t, a.x, a.control, a.np, a.n_vars, a.n_events, [st = a.st, k = a.k](const CrossEv& ev, size_t g, const f4 q) {
    update_event<FIRST>(st, g, q, ev.dir, ev.thr, k); // (a member without a control: a quiet NaN, which never hits)
  });
}

__global__ __launch_bounds__(kCrossThreads) void cross_fraction_kernel(const unsigned* __restrict__ hit, const int* __restrict__ offs,
                                                                       const int* __restrict__ member, int n_events, size_t gp,
                                                                       float* __restrict__ fraction) {
  const size_t quad = (size_t)blockIdx.x * kCrossThreads + threadIdx.x;
  if (quad >= gp) return;
  const int g = (int)blockIdx.y, ev = (int)blockIdx.z;
  const int k0 = offs[g], k1 = offs[g + 1];
  unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0; // (byte-wide counts side by side would overflow at 256 members: kept apart)
  for (int k = k0; k < k1; ++k) { // ascending member index
    const unsigned w = hit[((size_t)member[k] * n_events + ev) * gp + quad];
    c0 += w & 1u; c1 += (w >> 8) & 1u; c2 += (w >> 16) & 1u; c3 += (w >> 24) & 1u;
  }
  const double n = (double)(k1 - k0);
  const f4 o = {(float)((double)c0 / n), (float)((double)c1 / n), (float)((double)c2 / n), (float)((double)c3 / n)};
  reinterpret_cast<f4*>(fraction)[((size_t)g * n_events + ev) * gp + quad] = o;
}

__global__ __launch_bounds__(kCrossThreads) void cross_finish_kernel(CrossFinishArgs a) {
  const size_t g = (size_t)blockIdx.x * kCrossThreads + threadIdx.x; // a quad of [member][event][np]
  if (g >= a.n >> 2) return;
  auto copy = [g](int32_t* to, const int32_t* from) { reinterpret_cast<i4*>(to)[g] = reinterpret_cast<const i4*>(from)[g]; };
  if (a.first) copy(a.first, a.st.first);
  if (a.last) copy(a.last, a.st.last);
  if (a.count) copy(a.count, a.st.count);
  if (a.peak_year) copy(a.peak_year, a.st.peak_year);
  if (a.peak) reinterpret_cast<f4*>(a.peak)[g] = reinterpret_cast<const f4*>(a.st.peak)[g];
  if (a.stay) {
    i4 v = reinterpret_cast<const i4*>(a.st.last_miss)[g];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] + 1 <= a.n_years - 1 ? v[e] + 1 : -1; // the year from which it holds to the end
    reinterpret_cast<i4*>(a.stay)[g] = v;
  }
}

} // namespace

hipError_t launch_cross_update(const CrossUpdateArgs& a, hipStream_t s) {
  const CrossTable& t = a.t;
  if (!a.x || a.np < 4 || (a.np & 3) || a.n_members < 1 || a.n_vars < 1 || a.n_events < 1 || a.n_events > kCrossMaxEvents ||
      a.k < 0 || a.n_members > 65535 || (a.st.peak == nullptr) != (a.st.peak_year == nullptr) ||
      !year_table_ok(t, a.n_vars, a.n_events, a.control != nullptr))
    return hipErrorInvalidValue;
  const size_t gp = a.np >> 2;
  const dim3 grid((unsigned)((gp + kCrossThreads - 1) / kCrossThreads), (unsigned)a.n_members, (unsigned)t.n_vars_used);
  if (a.k == 0) hipLaunchKernelGGL(cross_update_kernel<true>, grid, dim3(kCrossThreads), 0, s, a);
  else hipLaunchKernelGGL(cross_update_kernel<false>, grid, dim3(kCrossThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cross_fraction(const unsigned char* hit, const int* offs, const int* member, int n_groups, int n_members,
                                 int n_events, size_t np, float* fraction, hipStream_t s) {
  if (!hit || !offs || !member || !fraction || n_groups < 1 || n_groups > 65535 || n_members < 1 || n_events < 1 ||
      n_events > kCrossMaxEvents || np < 4 || (np & 3))
    return hipErrorInvalidValue;
  const size_t gp = np >> 2;
  const dim3 grid((unsigned)((gp + kCrossThreads - 1) / kCrossThreads), (unsigned)n_groups, (unsigned)n_events);
  hipLaunchKernelGGL(cross_fraction_kernel, grid, dim3(kCrossThreads), 0, s, reinterpret_cast<const unsigned*>(hit), offs, member,
                     n_events, gp, fraction);
  return hipGetLastError();
}

hipError_t launch_cross_finish(const CrossFinishArgs& a, hipStream_t s) {
  if ((a.first && !a.st.first) || (a.last && !a.st.last) || (a.stay && !a.st.last_miss) || (a.count && !a.st.count) ||
      (a.peak && !a.st.peak) || (a.peak_year && !a.st.peak_year) || a.n_years < 1 || (a.n & 3))
    return hipErrorInvalidValue;
  const size_t quads = a.n >> 2;
  if (quads == 0) return hipSuccess;
  hipLaunchKernelGGL(cross_finish_kernel, dim3((unsigned)((quads + kCrossThreads - 1) / kCrossThreads)), dim3(kCrossThreads), 0, s, a);
  return hipGetLastError();
}

} // namespace greb
