// greb_ens.hip -- ensemble output (include/greb_engine.h: greb_ens_*): the reduction along the MEMBER axis, per group.
//
// A many-member run holds a model year as x[member][n] in one staging slot.  What its user wants of, say, 256 perturbed
// members at control CO2 beside the same 256 at 2 x CO2 is the spread of each member's RESPONSE to its partner, per grid
// point: a plan names each member's group and, optionally, its control member, and the sample of member m at element i
// is v = x[m][i], or v = x[m][i] - x[control[m]][i] as ONE fp32 subtraction.  A group's members are taken in ascending
// member index from a small device table (EnsLists), whatever else the launch holds.
//
//   ens_moments_kernel   grid (pairs of elements / 256, groups).  A lane owns two consecutive elements of one group and
//                        walks the group's member list with kEnsRows rows in flight (8-byte loads; with a control map 8
//                        members and their 8 controls).  From the same loads, in fp64: S = sum v (mean = S / n_g); with
//                        K = v of the group's first member and d = v - K, S1 = sum d and S2 = sum d d (var =
//                        (S2 - S1 S1 / n_g) / (n_g - 1), 0 where negative or n_g = 1: the shifted one-pass sample
//                        variance); min and max in fp32.  A row is read once per group it is in, not once per product.
//                        Rows that are not 8-byte aligned (n odd) are loaded element by element, and the lane that owns
//                        the last element owns it alone.
//   ens_quantile_kernel  one launch per group: a tile of P points x the group's members in LDS as [member][P], padded to
//                        a power of two with +INF, the control difference formed on load; bitonic sort along the member
//                        axis; then per probability p: h = (double)p (n_g - 1), lo = floor(h), t = h - lo,
//                        q = a + t (b - a) in fp64 with a = v[lo], b = v[min(lo + 1, n_g - 1)] (numpy's "linear" rule).
//                        P = min(64, 32768 / padded members): the tile stays within 128 KB.  With P = 64 (groups up to
//                        512 members) a wavefront's compare-exchange reads and writes one whole member row, 64 consecutive
//                        dwords: both 32-lane halves conflict-free, whatever the distance j between the rows.  With
//                        P < 64 a wavefront covers 64 / P rows; those are consecutive while j >= 64 / P and 2 j rows
//                        apart in blocks of j below that, where the 32-bank ds_read/write_b32 sees 2-way conflicts in
//                        the last few stages of each merge (accepted for groups above 512 members; not measured).
//                        256 members, 5 probabilities, 276 480 points: 2.2 ms (profiles/ens_numbers.txt).
//
// One owner per output element, no atomics: results are deterministic and a group's numbers depend neither on the other
// groups and members of the launch nor on where its members sit.  Every product is rounded to fp32 once.  THE ORDER OF
// OPERATIONS IS THE DEFINITION of the results (ens.reference in Python performs the same IEEE operations): this file is
// built with -ffp-contract=off (build.py: EXTRA_FLAGS), so that no multiply is fused into the add that follows it.
#include "greb_ens.h"

#include <cmath>
#include <cstdint>

#include "greb_kernels.h"

namespace greb {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// elements i0 and i0 + 1 of a row; `two`: the second one exists (always with VEC, where n is even and rows are aligned)
template <bool VEC>
__device__ inline f2 load2(const float* __restrict__ row, size_t i0, bool two) {
  if (VEC) return *reinterpret_cast<const f2*>(row + i0);
  f2 v;
  v.x = row[i0];
  v.y = two ? row[i0 + 1] : 0.f;
  return v;
}
template <bool VEC>
__device__ inline void store2(float* __restrict__ row, size_t i0, bool two, float a, float b) {
  if (VEC) {
    const f2 o = {a, b};
    *reinterpret_cast<f2*>(row + i0) = o;
    return;
  }
  row[i0] = a;
  if (two) row[i0 + 1] = b;
}

template <bool CTL, bool VEC>
__global__ __launch_bounds__(kEnsThreads) void ens_moments_kernel(EnsMomentArgs a) {
  constexpr int U = CTL ? kEnsRows / 2 : kEnsRows;
  const size_t i0 = 2 * ((size_t)blockIdx.x * kEnsThreads + threadIdx.x);
  if (i0 >= a.n) return;
  const bool two = VEC || i0 + 1 < a.n;
  const int g = blockIdx.y;
  const int k0 = a.l.offs[g], k1 = a.l.offs[g + 1]; // (uniform: the lists are read through the scalar cache)
  const int ng = k1 - k0;
  if (ng < 1) return;
  double S[2] = {0.0, 0.0}, S1[2] = {0.0, 0.0}, S2[2] = {0.0, 0.0}, K[2] = {0.0, 0.0};
  float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  auto row = [&](int m) { return a.x + (size_t)m * a.n; };
  auto take = [&](const f2& v) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double x = (double)v[e];
      S[e] = S[e] + x;
      const double d = x - K[e];
      S1[e] = S1[e] + d;
      S2[e] = S2[e] + d * d;
      lo[e] = fminf(lo[e], v[e]);
      hi[e] = fmaxf(hi[e], v[e]);
    }
  };
  int k = k0;
  for (; k + U <= k1; k += U) {
    f2 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = load2<VEC>(row(a.l.member[k + j]), i0, two);
    if (CTL) {
      f2 c[U];
#pragma unroll
      for (int j = 0; j < U; ++j) c[j] = load2<VEC>(row(a.l.control[k + j]), i0, two);
#pragma unroll
      for (int j = 0; j < U; ++j) v[j] = v[j] - c[j];
    }
    if (k == k0) { K[0] = (double)v[0].x; K[1] = (double)v[0].y; }
#pragma unroll
    for (int j = 0; j < U; ++j) take(v[j]);
  }
  for (; k < k1; ++k) {
    f2 v = load2<VEC>(row(a.l.member[k]), i0, two);
    if (CTL) v = v - load2<VEC>(row(a.l.control[k]), i0, two);
    if (k == k0) { K[0] = (double)v.x; K[1] = (double)v.y; }
    take(v);
  }
  const double n = (double)ng;
  const size_t at = (size_t)g * a.n;
  if (a.mean) store2<VEC>(a.mean + at, i0, two, (float)(S[0] / n), (float)(S[1] / n));
  if (a.var) {
    double var[2] = {0.0, 0.0};
    if (ng > 1) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const double t = (S2[e] - S1[e] * S1[e] / n) / (n - 1.0);
        var[e] = t < 0.0 ? 0.0 : t;
      }
    }
    store2<VEC>(a.var + at, i0, two, (float)var[0], (float)var[1]);
  }
  if (a.mn) store2<VEC>(a.mn + at, i0, two, lo[0], lo[1]);
  if (a.mx) store2<VEC>(a.mx + at, i0, two, hi[0], hi[1]);
}

// tile[mpad][P], P = 1 << lp points; mpad = the power of two >= ng
__global__ __launch_bounds__(kEnsThreads) void ens_quantile_kernel(const float* __restrict__ x, size_t n,
                                                                   const int* __restrict__ member,
                                                                   const int* __restrict__ control, int ng, int mpad, int lp,
                                                                   EnsProbs pr, float* __restrict__ out) {
  extern __shared__ __align__(16) float tile[];
  const int P = 1 << lp, tid = threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x << lp;
  for (int i = tid; i < (mpad << lp); i += kEnsThreads) { // P consecutive elements per member row
    const int m = i >> lp, p = i & (P - 1);
    float v = INFINITY; // padding sorts to the end
    if (m < ng && p0 + p < n) {
      v = x[(size_t)member[m] * n + p0 + p];
      if (control) v = v - x[(size_t)control[m] * n + p0 + p];
    }
    tile[i] = v;
  }
  __syncthreads();
  for (int lk = 1; (1 << lk) <= mpad; ++lk) { // bitonic sort of every column, ascending along the member axis
    for (int lj = lk - 1; lj >= 0; --lj) {
      const int j = 1 << lj;
      for (int t = tid; t < ((mpad >> 1) << lp); t += kEnsThreads) {
        const int p = t & (P - 1), h = t >> lp;               // h-th compare-exchange of the stage
        const int i = ((h >> lj) << (lj + 1)) + (h & (j - 1)); // lower row of the pair, partner i + j
        const bool up = (i & (1 << lk)) == 0;
        float* lo = tile + ((i << lp) + p);
        float* hi = tile + (((i + j) << lp) + p);
        const float u = *lo, w = *hi;
        if (up ? u > w : u < w) { *lo = w; *hi = u; }
      }
      __syncthreads();
    }
  }
  for (int t = tid; t < (pr.n << lp); t += kEnsThreads) {
    const int p = t & (P - 1), qi = t >> lp;
    if (p0 + p >= n) continue;
    const double h = (double)pr.p[qi] * (double)(ng - 1);
    int lo = (int)floor(h);
    lo = lo < 0 ? 0 : (lo > ng - 1 ? ng - 1 : lo);
    const int hi = lo + 1 < ng ? lo + 1 : ng - 1;
    const double f = h - (double)lo;
    const double u = (double)tile[(lo << lp) + p], w = (double)tile[(hi << lp) + p];
    out[(size_t)qi * n + p0 + p] = (float)(u + f * (w - u));
  }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

} // namespace

hipError_t launch_ens_moments(const EnsMomentArgs& a, int n_groups, hipStream_t s) {
  if (a.n == 0 || n_groups < 1) return hipSuccess;
  const size_t pairs = (a.n + 1) / 2;
  const dim3 grid((unsigned)((pairs + kEnsThreads - 1) / kEnsThreads), (unsigned)n_groups), block(kEnsThreads);
  const bool vec = a.n % 2 == 0 && aligned8(a.x) && aligned8(a.mean) && aligned8(a.var) && aligned8(a.mn) && aligned8(a.mx);
  const bool ctl = a.l.control != nullptr;
  if (ctl) {
    if (vec) hipLaunchKernelGGL((ens_moments_kernel<true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ens_moments_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((ens_moments_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ens_moments_kernel<false, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_ens_quantiles(const float* x, size_t n, const int* member, const int* control, int n_g, const EnsProbs& pr,
                                float* out, hipStream_t s) {
  if (n == 0 || pr.n < 1) return hipSuccess;
  if (n_g < 1 || n_g > kEnsMaxSorted || pr.n > kEnsMaxProbs) return hipErrorInvalidValue;
  int mpad = 1;
  while (mpad < n_g) mpad <<= 1;
  int lp = 0;
  while ((2 << lp) <= kEnsMaxPoints && (size_t)mpad * (2 << lp) <= (size_t)kEnsTileFloats) ++lp;
  const size_t lds = ((size_t)mpad << lp) * sizeof(float);
  const size_t tiles = (n + ((size_t)1 << lp) - 1) >> lp;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ens_quantile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kMaxDynamicLds); // (idempotent; set on every launch as elsewhere in the library)
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ens_quantile_kernel, dim3((unsigned)tiles), dim3(kEnsThreads), lds, s, x, n, member, control, n_g, mpad, lp,
                     pr, out);
  return hipGetLastError();
}

} // namespace greb
