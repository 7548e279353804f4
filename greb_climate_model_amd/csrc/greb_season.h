// greb_season.h -- the yearly quantity of a selector (0 ... 11 a month, 12 ... 16 DJF MAM JJA SON ANN) from the twelve months of
// one variable, as include/greb_engine.h states it for greb_cross and greb_reg: ONE statement of the formula for both.
// THE ORDER OF OPERATIONS IS THE DEFINITION: acc = 0.0; acc = acc + days[mo] * (double)x[mo] over the season's months in
// calendar order (DJF = Dec, Jan, Feb of the same model year); (float)(acc / the season's days).  The files that include
// this are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace greb {
namespace season {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kMonths = 12;
constexpr int kSelectors = 17;

// the quantity of selector s (a compile-time constant after unrolling) of four points
__device__ inline f4 quantity(int s, const f4 (&x)[kMonths]) {
  if (s < kMonths) return x[s];
  constexpr double days[kMonths] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31}; // JDAY_MON, src/greb.f90:42
  constexpr int first[5] = {11, 2, 5, 8, 0}, count[5] = {3, 3, 3, 3, 12};
  constexpr double total[5] = {90, 92, 92, 91, 365};
  const int q = s - kMonths;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < count[q]; ++j) {
    const int mo = (first[q] + j) % kMonths;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] + days[mo] * (double)x[mo][e];
  }
  f4 a;
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = (float)(acc[e] / total[q]);
  return a;
}

// the months selector s reads
__host__ __device__ constexpr int months_of(int s) {
  return s < kMonths ? 1 << s : s == 12 ? 0x803 : s == 13 ? 0x01c : s == 14 ? 0x0e0 : s == 15 ? 0x700 : 0xfff;
}

// the same quantity of ONE scalar series r[mo * stride], the selector known only at run time: the twelve values are
// loaded, and the selectors walked with constant s, so that it is quantity() above that forms the value
__device__ inline float series_quantity(const float* r, size_t stride, int s) {
  const int need = months_of(s);
  f4 x[kMonths];
#pragma unroll
  for (int mo = 0; mo < kMonths; ++mo) {
    x[mo] = f4{0.f, 0.f, 0.f, 0.f};
    if (need >> mo & 1) x[mo][0] = r[(size_t)mo * stride];
  }
  float a = 0.f;
#pragma unroll
  for (int c = 0; c < kSelectors; ++c)
    if (c == s) a = quantity(c, x)[0];
  return a;
}

} // namespace season
} // namespace greb
