// greb_lin.hip -- linear-model output (include/greb_engine.h: greb_lin_*): K linear contrasts along the MEMBER axis.
//
// A many-member run whose members differ by design -- the factorial of the process switches, a perturbed-physics
// ensemble -- is read through a linear model across its members: out_k = sum_m w[k][m] v_m per element of x[member][n],
// with v_m = x[m][i], or x[m][i] - x[control[m]][i] as ONE fp32 subtraction.  Main effects and interactions are such
// contrasts with weights +-1/M, least-squares coefficients are with W = pinv(X).  The used members are taken in
// ascending member index from a small device table (LinTables), whatever else the launch holds.
//
//   lin_coef_kernel  grid (pairs of elements / 256, chunks of 16 terms).  A lane owns two consecutive elements and 16 terms:
//                    32 fp64 accumulators.  It walks the used-member list with kLinRows rows in flight (8-byte loads;
//                    with a control map 4 members and their 4 controls) and per member adds w * (double)v to each
//                    accumulator as an fp64 multiply, then an fp64 add.  The weights are uniform: a member's 16 of the
//                    chunk are consecutive doubles of the table and come through the scalar cache.  A member row is read
//                    once per chunk.  Rows that are not 8-byte aligned (n odd) are loaded element by element, and the
//                    lane that owns the last element owns it alone.
//   lin_rss_kernel   grid (elements / 256).  A lane owns ONE element and keeps all K unrounded b_k of it in registers
//                    (KP = 16, 32, 48 or 64 doubles: the [K][tile] scratch of the fit, one column per lane -- a lane only
//                    ever reads its own): it forms them exactly as lin_coef_kernel does, then walks the members a second
//                    time, kLinFit at a time: f = sum_k design[m][k] b_k in ascending k from +0.0, r = (double)v - f,
//                    R = R + r r.  No scratch array in LDS or device memory, nothing that the two kernels share: either
//                    product alone gives the bits it has beside the other.
//
// Terms behind K - 1 in the last chunk have weight and design 0.0 in the tables: their sums start from +0.0, stay +0.0
// or NaN, and are never stored; in the fit they add design * b = +0.0 to an f that is never -0.0 (it started from +0.0),
// which leaves it as it is.  One owner per output element, no atomics.  THE ORDER OF OPERATIONS IS THE DEFINITION of the
// results (lin.reference in Python performs the same IEEE operations): this file is built with -ffp-contract=off
// (build.py: EXTRA_FLAGS), so that no multiply is fused into the add that follows it.
#include "greb_lin.h"

#include <cstdint>

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

struct LinArgs {
  const float* x; // [n_members][n]
  size_t n;
  LinTables t;
  float* out; // coef [K][n], or rss [n]
};

template <bool CTL, bool VEC>
__global__ __launch_bounds__(kLinThreads) void lin_coef_kernel(LinArgs a) {
  constexpr int U = CTL ? kLinRows / 2 : kLinRows;
  const size_t i0 = 2 * ((size_t)blockIdx.x * kLinThreads + threadIdx.x);
  if (i0 >= a.n) return;
  const bool two = VEC || i0 + 1 < a.n;
  const int t0 = (int)blockIdx.y * kLinChunk; // (uniform: the tables are read through the scalar cache)
  const int nt = a.t.n_terms - t0 < kLinChunk ? a.t.n_terms - t0 : kLinChunk;
  const int n_used = a.t.n_used;
  const double* __restrict__ w = a.t.weight + t0;
  double b[kLinChunk][2];
#pragma unroll
  for (int j = 0; j < kLinChunk; ++j) b[j][0] = b[j][1] = 0.0;
  auto row = [&](int m) { return a.x + (size_t)m * a.n; };
  auto take = [&](int k, const f2& v) {
    const double* __restrict__ wk = w + (size_t)k * a.t.stride;
    const double v0 = (double)v.x, v1 = (double)v.y;
#pragma unroll
    for (int j = 0; j < kLinChunk; ++j) {
      const double wj = wk[j];
      b[j][0] = b[j][0] + wj * v0;
      b[j][1] = b[j][1] + wj * v1;
    }
  };
  int k = 0;
  for (; k + U <= n_used; k += U) {
    f2 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = load2<VEC>(row(a.t.member[k + j]), i0, two);
    if (CTL) {
      f2 c[U];
#pragma unroll
      for (int j = 0; j < U; ++j) c[j] = load2<VEC>(row(a.t.control[k + j]), i0, two);
#pragma unroll
      for (int j = 0; j < U; ++j) v[j] = v[j] - c[j];
    }
#pragma unroll
    for (int j = 0; j < U; ++j) take(k + j, v[j]);
  }
  for (; k < n_used; ++k) {
    f2 v = load2<VEC>(row(a.t.member[k]), i0, two);
    if (CTL) v = v - load2<VEC>(row(a.t.control[k]), i0, two);
    take(k, v);
  }
#pragma unroll
  for (int j = 0; j < kLinChunk; ++j)
    if (j < nt) store2<VEC>(a.out + (size_t)(t0 + j) * a.n, i0, two, (float)b[j][0], (float)b[j][1]);
}

template <bool CTL, int KP>
__global__ __launch_bounds__(kLinThreads) void lin_rss_kernel(LinArgs a) {
  constexpr int U = CTL ? kLinRows / 2 : kLinRows;
  const size_t i = (size_t)blockIdx.x * kLinThreads + threadIdx.x;
  if (i >= a.n) return;
  const int n_used = a.t.n_used;
  auto at = [&](int m) { return a.x[(size_t)m * a.n + i]; };
  auto sample = [&](int k) {
    float v = at(a.t.member[k]);
    if (CTL) v = v - at(a.t.control[k]);
    return v;
  };
  double b[KP];
#pragma unroll
  for (int t = 0; t < KP; ++t) b[t] = 0.0;
  auto take = [&](int k, float v) {
    const double* __restrict__ wk = a.t.weight + (size_t)k * a.t.stride;
    const double vd = (double)v;
#pragma unroll
    for (int t = 0; t < KP; ++t) b[t] = b[t] + wk[t] * vd;
  };
  int k = 0;
  for (; k + U <= n_used; k += U) { // the coefficients, as lin_coef_kernel forms them
    float v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = at(a.t.member[k + j]);
    if (CTL) {
      float c[U];
#pragma unroll
      for (int j = 0; j < U; ++j) c[j] = at(a.t.control[k + j]);
#pragma unroll
      for (int j = 0; j < U; ++j) v[j] = v[j] - c[j];
    }
#pragma unroll
    for (int j = 0; j < U; ++j) take(k + j, v[j]);
  }
  for (; k < n_used; ++k) take(k, sample(k));
  double R = 0.0;
  k = 0;
  for (; k + kLinFit <= n_used; k += kLinFit) { // the fit: kLinFit independent sums side by side, taken in ascending member
    float v[kLinFit];
    double f[kLinFit];
#pragma unroll
    for (int j = 0; j < kLinFit; ++j) { v[j] = sample(k + j); f[j] = 0.0; }
#pragma unroll
    for (int t = 0; t < KP; ++t) {
#pragma unroll
      for (int j = 0; j < kLinFit; ++j) f[j] = f[j] + a.t.design[(size_t)(k + j) * a.t.stride + t] * b[t];
    }
#pragma unroll
    for (int j = 0; j < kLinFit; ++j) {
      const double r = (double)v[j] - f[j];
      R = R + r * r;
    }
  }
  for (; k < n_used; ++k) {
    const float v = sample(k);
    const double* __restrict__ dk = a.t.design + (size_t)k * a.t.stride;
    double f = 0.0;
#pragma unroll
    for (int t = 0; t < KP; ++t) f = f + dk[t] * b[t];
    const double r = (double)v - f;
    R = R + r * r;
  }
  a.out[i] = (float)R;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
bool tables_ok(const LinTables& t) {
  return t.n_used >= 1 && t.n_terms >= 1 && t.n_terms <= kLinMaxTerms && t.stride % kLinChunk == 0 && t.stride >= t.n_terms &&
         t.stride <= kLinMaxTerms && t.member && t.weight;
}

template <bool CTL>
void launch_rss(int kp, dim3 grid, hipStream_t s, const LinArgs& a) {
  const dim3 block(kLinThreads);
  switch (kp) {
    case 16: hipLaunchKernelGGL((lin_rss_kernel<CTL, 16>), grid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL((lin_rss_kernel<CTL, 32>), grid, block, 0, s, a); break;
    case 48: hipLaunchKernelGGL((lin_rss_kernel<CTL, 48>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((lin_rss_kernel<CTL, 64>), grid, block, 0, s, a); break;
  }
}

} // namespace

hipError_t launch_lin_coef(const float* x, size_t n, const LinTables& t, float* coef, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!tables_ok(t) || !x || !coef) return hipErrorInvalidValue;
  const size_t pairs = (n + 1) / 2;
  const int chunks = (t.n_terms + kLinChunk - 1) / kLinChunk; // (<= stride / 16: the table has a row of 16 for each)
  const dim3 grid((unsigned)((pairs + kLinThreads - 1) / kLinThreads), (unsigned)chunks), block(kLinThreads);
  const bool vec = n % 2 == 0 && aligned8(x) && aligned8(coef);
  const LinArgs a{x, n, t, coef};
  if (t.control) {
    if (vec) hipLaunchKernelGGL((lin_coef_kernel<true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((lin_coef_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((lin_coef_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((lin_coef_kernel<false, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_lin_rss(const float* x, size_t n, const LinTables& t, float* rss, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!tables_ok(t) || !t.design || !x || !rss) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + kLinThreads - 1) / kLinThreads));
  const LinArgs a{x, n, t, rss};
  if (t.control) launch_rss<true>(t.stride, grid, s, a);
  else launch_rss<false>(t.stride, grid, s, a);
  return hipGetLastError();
}

} // namespace greb
